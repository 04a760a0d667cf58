#!/usr/bin/env python3
"""Map-free MPPI for a nominal unicycle with disc obstacles: the classes that
/root/reference/barebone_mppi_numba.ipynb defines inline (cell 2 `Config`,
cell 3 `MPPI_Numba`), on MI355X.  Same constructor keywords, methods and params
keys ('obstacle_positions', 'obstacle_radius', 'obs_penalty', 'dist_weight').

Stage cost dist_weight*d^2, terminal cost (1-reached)*d^2, obstacle penalty
when the POST-step position lies inside a disc (notebook cell 3).

Not in the notebook: discs that move.  params['obstacle_tracks'] (K, L, 2) in
place of 'obstacle_positions' gives every disc L predicted centres, row j its
centre at time j*dt from "now"; "now" is row `track_offset`, and the state
after step t of a rollout is tested against row min(track_offset + t + 1, L - 1).

Crowd mode, Config(crowd=True) / set_crowd(True): disc sets of any size (the default forms keep a row of disc slots per
step in 64 KiB of LDS: 39 moving discs at 100 steps); same results bit for bit.

Walls (crowd mode only): params['wall_segments'] (W, 2, 2), [[ax, ay], [bx, by]] per wall, and params['wall_halfwidth'],
a scalar or (W,).  Step t of a rollout moves the robot from P to Q (P of step 0 is x0); it hits a wall iff the distance
between the closed segments PQ and AB is <= the half-width -- a step that jumps a thin wall is a hit -- and every hit adds
obs_penalty once, like a disc hit of that step.  polyline_walls() turns a room outline into segments.

Walls that move: params['wall_tracks'] (W, L, 2, 2) in place of 'wall_segments' gives every wall L segments, row j the
segment it occupies during control interval j, from j*dt to (j+1)*dt after "now".  Step t of a rollout is interval
track_offset + t and is tested against row min(track_offset + t, L - 1): a wall row is an interval where a disc row is an
instant, and each kind of track clamps against its own row count.  The half-widths stay static per wall.  A wall that itself
jumps over the robot between two rows is seen only if its rows are sweeps of its motion (swept_walls() makes those of a
disc; the sweep of a translating segment, a parallelogram, is not provided).  constant_velocity_walls() makes the rows of
walls that keep their velocity.  MPPI_Batch.set_wall_sets() gives every problem of a batch its own walls or wall tracks.

A goal that moves: params['goal_track'] (L, 2) in place of 'xgoal' gives the goal L positions, row j its position at time
j*dt from "now" -- an instant, like a disc row, and the same "now": track_offset.  The state after step t of a rollout is
measured against row min(track_offset + t + 1, L - 1): stage cost, goal test, freeze and terminal cost are the notebook's on
a goal that changes with t, and "reached" means within goal_tolerance of where the goal is at that instant (intercept,
rendezvous); a follower sets goal_tolerance = 0 so that nothing freezes.  Past its last row the goal stays at its last
place; a track of one row, or of equal rows, is a static goal to the bit.  No helper is needed to make one:
constant_velocity_tracks(p, v, dt, rows)[0] is the goal track of a target that keeps its velocity, and another robot's
planned states[:, :2] is the goal track of a follower.  goal_now is the goal where it is now; MPPI_Batch.set_goal_tracks()
gives every problem of a batch its own.

A fleet: MPPI_Batch.set_fleet(radii, margin) makes the B problems of a batch in crowd mode robots that avoid each other's
plans, without the host in the middle.  At the head of every solve(), rollout() and control step of closed_loop() -- once
per call, not between the num_opt iterations -- the device rebuilds for every robot a the walls swept_walls() would make of
the OTHER robots' current plans: the plan of b is the noise-free rollout c_0 .. c_T of its control sequence from its start
state (the controls clipped to vrange / wrange, the rollouts' own float32 state step; it goes on past the goal), row j of
its wall the segment [c_j, c_{j+1}], the half-width float32(r_a + r_b + margin).  These rows are always counted from "now":
step t meets row t whatever track_offset is, and the fleet neither advances nor resets track_offset, so disc tracks and
goal tracks keep their meaning beside it.  params['wall_segments'] -- a room, a corridor -- stay in force for every robot;
params['wall_tracks'] and set_wall_sets() are refused while the fleet is on (one owner of the per-problem sets).  All robots
plan at once, each against the others' plans of the previous control step, shifted: a Jacobi sweep, where one planner per
robot planning in turn sees the plans of this step.  Before the first solve the controls are zero and every plan stands at
its start.  closed_loop() parks a robot that has reached its goal (its rows become its final position); in a host-driven
loop the library does not know who has arrived: park a robot by giving it zero controls (set_u), where vrange admits 0.
fleet_walls() fetches the rows of the last refresh, refresh_fleet() refreshes alone (for drawing).

Disc samples (crowd mode only): params['obstacle_track_samples'] (S, K, L, 2), S <= 16, in place of 'obstacle_positions' and
'obstacle_tracks' gives the K discs S sampled futures, as a predictor hands them out (goes straight, turns left, stops);
sample s is an ordinary track set, params['obstacle_radius'] (K,) its radii.  The cost of a rollout under sample s is the cost
the launch gives it with obstacle_tracks = samples[s], bit for bit; walls, wall tracks, a goal track and the fleet stay in
force and do not depend on s.  The rollout's cost is the conditional value at risk over its S costs: params['cvar_alpha'] in
(0, 1], default 1.0 -- the mean of the worst ceil(S * alpha) costs as the reference's CVaR mode forms it (sorted descending
iff alpha < 1, a strided float32 tree, the division in double); alpha = 1 is the mean, alpha <= 1/S the worst case.  Without a
sample set nothing reads cvar_alpha.  In a batch every problem sees the same samples.  record_sample_costs() /
sample_costs() give the (N, S) per-sample costs; sampled_tracks() is the simplest predictor to try it with.

A body footprint (crowd mode only): params['footprint'] (F, 3), 1 <= F <= 8, rows (ox, oy, rho) -- a body disc's centre in the
robot frame (x along the heading, y to the left) and its radius -- makes the robot F discs rigidly attached to its pose, so
that the heading counts in the hit tests: a cart 1.0 m long and 0.4 m wide passes a 0.7 m doorway lengthwise, which its
circumscribed disc cannot.  At a state (x, y, th) body disc i has its centre at x + (ox cos th - oy sin th),
y + (ox sin th + oy cos th), in float64 and rounded once to float32 (body_discs()).  The body touches a disc iff any body disc
does, with the radii added, at the post-step state; it hits a wall iff any body disc's chord, from its centre before the
step to its centre after it, does, with rho added to the half-width.  A step's hits are counted per obstacle, however many
body discs reach one, so a finer cover of the same body does not multiply the penalty; every hit adds obs_penalty once.
Tracks, wall tracks, per-problem sets and disc samples work as before; goal distance, goal test, freeze and terminal
cost are measured at the reference point (x, y).  rectangle_footprint() covers a rectangle with discs on the body axis.
Without the key the robot is the point it always was, to the bit.  Limits: one footprint for every problem of a batch
(per-problem footprints are not provided); params['footprint'] and set_fleet() exclude each other (the disc fleet's
half-widths already contain the reader's body; a fleet of elongated robots is set_fleet_bodies(), below); a point of a
turning body moves on an arc and its chord is what is tested -- the arc leaves the chord by at most
|o| (1 - cos(dt w / 2)), 2.5 mm for |o| = 0.5 m at dt w = 0.2 rad.

A fleet of bodies: MPPI_Batch.set_fleet_bodies(footprint, margin) is the fleet for robots that are not discs -- carts that
pass each other lengthwise in a corridor their circumscribed discs would block.  Every robot of the batch has the body
`footprint` (F, 3), rows as for params['footprint'].  The refresh is the fleet's, with the heading kept: the plan of b is
its noise-free states s_0 .. s_T = (x, y, th); body disc k of b has its centre at body_discs(s_j)[k] and sweeps the segment
from there to body_discs(s_{j+1})[k] in control interval j; reader a is given that segment as a wall of half-width
float32(rho_k + margin), the sum in float64.  The reader's own body meets these walls as a footprint meets any wall (its
discs' chords, rho_i added to the half-width), and a step hits robot b iff ANY body disc of the reader hits ANY wall of b:
one hit, obs_penalty once, however many pairs touch.  params['wall_segments'] stay in force behind the fleet's walls, one
hit per wall.  Discs, disc tracks, disc samples, goal tracks and the goal distance at the reference point are untouched.
A reader's walls lie in (B - 1) * Fp slots, Fp = F rounded up to a power of two (the padding repeats the last disc), so a
step of a rollout costs F * ((B - 1) * Fp + W) wall tests: a body of 3, 5, 6 or 7 discs pays for its padding.  Limits: one
body for the whole fleet; the chord for the arc, as above; the plans are those of the previous control step (the Jacobi
sweep of the disc fleet).  set_fleet_bodies carries its own body: it is refused while params hold 'footprint', and the two
kinds of fleet change into each other through set_fleet(None).  fleet_body_walls() fetches the rows of the last refresh.

Clearance rings (crowd mode only): params['clearance_rings'] (R, 2), 1 <= R <= 4, rows (margin, penalty) rounded once to
float32 -- margins finite, > 0 and strictly increasing, penalties finite and >= 0 -- give a cost that rises on the way in, as
a staircase: an obstacle that a step misses by less than margin_l costs penalty_l, for every ring l it is inside of.  With
m = float64(margin_l), an obstacle of the step is NEAR at ring l iff the step would touch it were it m larger:
  disc k, point robot   the disc test -- the float32 difference widened, fma(ex, ex, ey*ey) - rr, near iff not diff > 0 --
                        with rr = R*R, R = float64(r_k) + m
  disc k, a footprint   the footprint's disc test with R = (float64(r_k) + rho_i) + m; near iff any body disc is
  wall k, point robot   the wall test with hh = H*H, H = float64(h_k) + m
  wall k, a footprint   H = (float64(h_k) + rho_i) + m per body disc chord; near iff any chord is
A step that crosses a wall is inside every ring.  The fleet's walls and the fleet of bodies' walls are walls like any other;
in a fleet of bodies a robot is near at ring l once, however many of its slots are.  n_l(t) counts the obstacles near at
ring l in step t, the hit ones included, so n_l >= hits and n_1 <= n_2 <= ...  The step's cost chain is: the distance term;
`hits` float32-rounded additions of float64(obs_penalty), as ever; for l = 1 .. R, n_l additions
c = float32(float64(c) + float64(penalty_l)); the freeze at the goal, as ever.  Additions and not a product: a ring whose
penalty is obs_penalty costs what a second copy of the obstacles, m larger, costs, to the bit.  Goal distance, goal test,
freeze, terminal cost and control cost do not know about rings.  clearance_staircase() makes the rows that sit on top of
peak * (1 - gap/reach)^2.  Without the key nothing changes anywhere.  Limits: refused together with
'obstacle_track_samples'; one ring set for every problem of a batch; the default kernel family has no rings (a handle that
holds rings always launches the crowd kernel).

Time-correlated control noise: params['noise_smoothing'], a scalar (both components) or (2,) = (beta_v, beta_w), rounded once
to float32, each in [0, 1).  The notebook's noise is an independent draw per step, a jitter whose displacement largely
averages out over the horizon; with the key every generated block is the white block w -- the same Philox counters and
epochs, u_std times the Box-Muller normal -- filtered along t, per rollout and component, in float32:
  g       = float32(sqrt(1 - float64(beta) * float64(beta)))
  e[n, 0] = w[n, 0]
  e[n, t] = float32(float32(beta * e[n, t-1]) + float32(g * w[n, t]))          t = 1 .. T-1
two rounded products and one rounded sum, never an fma.  Step 0 is the white draw and the gain is sqrt(1 - beta^2), so every
step keeps the standard deviation u_std and the lag-k correlation is beta^k; beta = 0 is the white noise.  The recurrence
restarts with every block: nothing is carried from one iteration or control step to the next.  solve(), closed_loop(),
graph replay and sample_noise() draw it on the device; set_noise() stores what it is given, unfiltered.  A change takes
effect with the next call, as if the handle had had the value from the start; without the key -- or with 0 -- every bit is
the notebook's.  Limits: philox only (rng="xoroshiro" is refused: that generator exists for parity with numba from the
seed); one setting for every problem of a batch; first order only; the control-cost term of the rollouts still weighs the
noise by diag(u_std^2), as for white noise.  The map-mode classes do not read the key.

A guide round the walls: params['guide'], a dict with 'origin' (x, y), 'resolution', 'shape' (ny, nx) and optionally
'inflate' (default: the resolution), 'pace' (default vrange[1] * dt) and 'lead' (default 2 * pace), all rounded once to
float32.  The rollouts steer by the straight-line distance to the goal and look T * dt ahead: in a room whose door lies on
the side away from the goal they lean on the wall nearest the goal for ever.  With the key the device computes, per problem,
a shortest-path distance field from params['xgoal'] over a grid of ny * nx <= 36864 cells (192 x 192) -- cell (iy, ix) has
its centre at origin + (ix + 0.5, iy + 0.5) * resolution; a point outside the grid belongs to the nearest border cell; a
cell is blocked iff its centre is within wall_halfwidth + inflate of a wall of params['wall_segments']; a straight move
costs 12 and a diagonal one 17, so one unit is resolution / 12 -- and at the head of every solve(), rollout() and control
step of closed_loop() it walks the descent from the robot's cell and fills a goal table of T + 1 rows with "carrots": row
j is the centre of the first cell on the shortest path that is floor(lead / resolution * 12) + j * floor(pace / resolution
* 12) units nearer to the goal than the start is, or the goal itself once the path ends.  Step t of a rollout is measured
against row t + 1 exactly as against a goal track's row -- stage cost, goal test, freeze and terminal cost -- whatever
track_offset is; the guide neither reads nor advances it.  2 * inflate^2 >= resolution^2 is required: then no move between
two free neighbouring centres touches a wall, diagonal moves included.  Only the static shared walls are rasterised: discs,
disc tracks, wall tracks, per-problem wall sets and the fleet's walls are not in the field -- the rollouts' hit tests deal
with them locally.  A goal in a blocked cell (guide_status() 1) or a start with no way out (2: a sealed pocket) makes every
row the goal; a start inside the inflated band walks out the cheapest way.  Keep lead above goal_tolerance: a rollout that
catches its carrot freezes, as it does with any goal track.  The field is rebuilt only when the guide, the walls or a goal
changed; guide_field(), guide_rows(), guide_status() fetch what the last refresh left, refresh_guide() refreshes alone (for
drawing), goal_now stays the true goal and closed_loop()'s arrival test is against it.  guide_grid() makes origin and shape
from the walls' bounding box.  Limits: 'guide' and 'goal_track' exclude each other (the guide owns the goal rows);
params['xgoal'] is required; one grid for every problem of a batch, whose goals and starts are set_instances()'.

Acceleration limits on the sampled controls: params['accel_limits'], a scalar (both components) or (2,) = (a_v, a_w) in
m/s^2 and rad/s^2, rounded once to float32, each > 0; np.inf leaves a component as drawn.  The notebook's rollouts may
command vrange[1] in one step and vrange[0] in the next, and so may the sequence solve() returns: no base follows that, and
the first control handed out may be out of reach of the velocity the robot has now.  With the key every block an iteration
is about to consume passes through one more kernel, in place: per rollout and component, with u the sequence the rollouts
read, e the block as generated (white or smoothed), (lo, hi) the component's range and a the applied control, in float32,
every operation rounded once:
  d     = float32(float32(accel) * float32(dt))
  p     = clip(a, lo, hi)
  c     = clip(float32(u[t] + e[n, t]), lo, hi)                                 t = 0 .. T-1
  p     = min(max(c, float32(p - d)), float32(p + d))
  e'[n, t] = float32(p - u[t])
and the block holds e', the effective noise: the rollouts simulate feasible sequences, the control-cost term weighs the
deviation actually applied, and the update u + sum(w e') / sum(w) is a convex combination of feasible sequences -- the set
"inside the box, no step larger than d, counted from the anchor" is convex -- and so feasible itself, whatever u was.  What
the rollouts re-form as clip(u + e') differs from p by rounding only: consecutive controls differ by at most d + 2^-20 *
(max(|lo|, |hi|) + d).  The anchor is applied_control, zero at first: set_applied_control(u) sets it -- (2,), or (B, 2) for a
batch --, shift_and_update(x, u_cur, k) sets it to u_cur[k - 1] while the key is in params (a user with odometry calls
set_applied_control(measured) after it), closed_loop() stores every u0 it applies.  The recurrence restarts with every
block from the anchor.  Composes with both kernel families, every crowd form, batches, fleets (whose plans are noise-free
rollouts of u, feasible after the first update), the guide, tracks, disc samples, rings, the footprint, 'noise_smoothing'
(limited after filtering), both generators, math="fast", graph replay (a new anchor needs no new capture) and closed_loop().
sample_noise() limits what it draws; set_noise() stores what it is given and limit_noise() runs the pass alone over it.
Without the key every bit and every call is as before.  Limits: one pair for every problem of a batch; symmetric (no
separate braking bound); first differences only (no jerk bound); the visualisation rollouts read the block as it stands;
the control-cost term weighs e'.  The map-mode classes do not read the key.

Car-like steering: params['drive'] = 'car' ('unicycle' is the key left out; any other string raises ValueError).  The
notebook's vehicle is a unicycle: w is commanded independently of v, so every rollout -- and the sequence solve() returns --
may turn on the spot, which no tugger, forklift or Ackermann cart can follow.  With 'car' the second control is the path
curvature kappa in 1/m instead of the yaw rate: wrange is the curvature range, +-tan(max_steer) / wheelbase
(curvature_of_steering(); steering_of_curvature() goes back), u_std[1] the curvature noise, and the second component of
'accel_limits' a bound on the curvature's rate -- a steering-rate bound.  A step, in float32, every operation rounded once:
  v = clip(float32(u[t][0] + e[n, t][0]), vrange)      kappa = clip(float32(u[t][1] + e[n, t][1]), wrange)
  w = float32(v * kappa)                               never an fma; the unicycle: w = kappa
  x, y                                                 as ever, from the heading BEFORE the step and float32(dt * v)
  th' = float32(th + float32(dt * w))
so the car turns only while it moves, its turning radius is never below 1 / max|kappa|, and reversing with the wheel turned
left swings the heading the other way.  Everything downstream of the pose is untouched: goal distance, discs, walls,
footprint chords, rings, occupancy, disc samples, control cost (on the curvature's noise), the update and the guide.  The
rollouts of both kernel families, get_state_rollout() (row 0: u_cur unclipped, w = float32(v * kappa)), the plans of both
fleets and closed_loop()'s world (float64: th += dt * (float64(v) * float64(kappa))) follow; shift_and_update(),
set_applied_control() and closed_loop() keep their meaning with the second component read as curvature.  The host bounds
the heading increment of a step by dt * max|v| * max|kappa| where it bounded it by dt * max|w|: (cos, sin) by rotation needs
that at 0.36 rad at the most.  last_rollout_kernel() ends in ' drive=car'; the `drive` property reads the library's value
back.  Without the key every bit, every launch and every kernel name is as before.  Limits: kappa is not the steering angle
delta (convert with the two helpers); a steering-rate bound through 'accel_limits' is a bound on kappa's rate, not on
delta's; reverse costs what forward costs (no separate reverse-gear cost: keep vrange[0] >= 0 to forbid it); one drive for
every problem of a batch.  The map-mode classes do not read the key.

Occupancy-grid obstacles: params['occupancy'], a dict with 'origin' (x, y), 'resolution', 'cells' (ny, nx) -- any integer or
bool dtype, non-zero means occupied -- and optionally 'inflate' (default 0; for a point robot its radius) and 'substeps' (an
int in 1 .. 8, default 1); the floats rounded once to float32.  A costmap as it comes from a lidar, without fitting discs or
segments to it: the device keeps the clearance field D2, uint32 (ny, nx), D2[iy, ix] = the least (ix - jx)^2 + (iy - jy)^2
over the occupied cells (jy, jx) -- 0 on an occupied cell, 0xFFFFFFFF everywhere when none is occupied; integers only --,
rebuilt by a kernel of its own at the head of the next solve(), rollout() or control step only when the cells changed, and
the crowd kernel counts the grid as ONE more obstacle.  A point robot is the body of one disc (0, 0, 0); for body disc i of
radius rho_i, A and B are its float32 centres at the pre-step and the post-step state (the footprint's centres; step 0: the
start state, heading included), and with M = substeps test point k = 1 .. M is
  k == M      X = float64(B)                                                   (M = 1: the notebook's post-step test)
  otherwise   X = float64(A) + (float64(k) / float64(M)) * (float64(B) - float64(A))       the product rounded, never an fma
  cell        q = floor((X - float64(origin)) / float64(resolution)) per axis; inside iff 0 <= q <= n - 1 on both axes (a NaN
              is outside); a point outside the grid is free: no hit, and near at no ring
  level l     (0: the hit; l >= 1: clearance ring l of margin m_l) inside and D2[cell] <= thr[i][l],
              thr = min(floor(R * R / (res * res)), 0xFFFFFFFE), R = (float64(inflate) + float64(rho_i)) + m_l
A step whose any test point of any body disc hits adds 1 to the step's hits -- one more float32-rounded addition of
float64(obs_penalty) --, a step near at ring l through any point adds 1 to n_l; goal distance, freeze, terminal term, control
cost and the CVaR tail are as they were.  What a miss means: a chord with no hit keeps every point of it more than
R - |AB| / (2 M) - resolution * sqrt(2) / 2 from every occupied cell's centre -- choose 'inflate' and 'substeps' from that;
with the default substeps = 1 it is the notebook's post-step test, as for discs.  Composes with discs, disc tracks and
per-problem disc sets, walls, wall tracks and per-problem wall sets, goal tracks and the guide, both fleets (a fleet of
bodies: the fleet's body; a disc fleet: the point), 'footprint', 'clearance_rings', 'noise_smoothing', 'accel_limits',
math="fast", graph replay (new cells of the same shape need no new capture) and closed_loop().  With 'guide' as well, a guide
cell is blocked also when its centre lies inside the grid on a cell with D2 <= thr_g, R = inflate_occupancy + inflate_guide;
the two grids need not coincide, and new cells rebuild the guide's field too.  occupancy_field() fetches D2,
refresh_occupancy() builds it alone (for drawing), rasterise_obstacles() makes cells from walls and discs.  Without the key
every bit, every launch and every kernel name is as before.  Limits: crowd mode only (a handle that holds a grid always
launches the crowd kernel); 1 <= nx, ny <= 512, resolution > 0, inflate >= 0, all finite; refused together with
'obstacle_track_samples'; one grid for every problem of a batch; one obs_penalty for the grid as a whole; outside the grid is
free; the grid does not move (a new grid per control step is the way to move it); the fleet's refresh and the simulated
world do not read it; the chord stands in for the arc, as with any footprint.
"""
import collections
import copy
import ctypes as C
import time

import numpy as np

from . import _lib
from . import config as _config
from .device_array import DeviceArray

DEFAULT_OBS_COST = 1e3
DEFAULT_DIST_WEIGHT = 10

rec_max_control_rollouts = int(1e6)  # the notebook raises the cap of config.py
rec_min_control_rollouts = 100


class Config:

    """ Configurations that are typically fixed throughout execution. """

    def __init__(self, T=10, dt=0.1, num_control_rollouts=1024, num_vis_state_rollouts=20, seed=1,
                 enforce_recommended_limits=True, rng="philox", math="exact", device=0, crowd=False):
        assert T > 0
        assert dt > 0
        assert T > dt
        self.seed = seed
        self.T = T
        self.dt = dt
        self.num_steps = int(T / dt)
        assert self.num_steps > 0
        self.max_threads_per_block = _config.max_threads_per_block
        self.rng, self.math, self.device = rng, math, device
        self.crowd = bool(crowd)  # crowd mode: no LDS limit on the disc sets (set_crowd)

        self.num_control_rollouts = num_control_rollouts
        if enforce_recommended_limits:
            if self.num_control_rollouts > rec_max_control_rollouts:
                self.num_control_rollouts = rec_max_control_rollouts
                print("MPPI Config: Clip num_control_rollouts to be recommended max number of {}. (Max={})".format(
                    rec_max_control_rollouts, _config.max_blocks))
            elif self.num_control_rollouts < rec_min_control_rollouts:
                self.num_control_rollouts = rec_min_control_rollouts
                print("MPPI Config: Clip num_control_rollouts to be recommended min number of {}. (Recommended max={})".format(
                    rec_min_control_rollouts, rec_max_control_rollouts))
        self.num_vis_state_rollouts = max(1, min(num_vis_state_rollouts, self.num_control_rollouts))


_TASK_VECTORS = (("x0", 3), ("xgoal", 2), ("vrange", 2), ("wrange", 2), ("u_std", 2))  # params keys -> _lib.Params arrays
_TASK_VECTORS_GOAL_TRACK = tuple(entry for entry in _TASK_VECTORS if entry[0] != "xgoal")


def _f32(values):
    return np.asarray(values, dtype=np.float64).astype(np.float32)


def constant_velocity_tracks(positions, velocities, dt, rows):
    """(K, rows, 2) float32 tracks of discs that keep their velocity: row j is positions + velocities * (j*dt),
    evaluated in float64 and rounded once to float32 (row 0 is float32(positions))."""
    rows = int(rows)
    assert rows >= 1, "a track has at least one row"
    pos = np.asarray(positions, dtype=np.float64).reshape(-1, 1, 2)
    vel = np.asarray(velocities, dtype=np.float64).reshape(-1, 1, 2)
    assert len(pos) == len(vel), "positions and velocities differ in length"
    times = (np.arange(rows, dtype=np.float64) * float(dt)).reshape(1, rows, 1)
    return np.ascontiguousarray((pos + vel * times).astype(np.float32))


def sampled_tracks(positions, velocities, dt, rows, vel_std, samples, seed=0):
    """(S, K, rows, 2) float32 disc samples for params['obstacle_track_samples']: sample 0 is constant_velocity_tracks of the
    nominal velocities, samples 1 .. S-1 the same with the velocities perturbed by
    numpy.random.default_rng(seed).normal(0, vel_std), one (S - 1, K, 2) draw, evaluated in float64 and rounded once to
    float32.  Host only.  The simplest predictor there is -- every disc keeps a velocity drawn once -- and not a model of
    anything."""
    samples = int(samples)
    assert samples >= 1, "a sample set has at least one sample"
    vel = np.asarray(velocities, dtype=np.float64).reshape(-1, 2)
    noise = np.random.default_rng(seed).normal(0.0, float(vel_std), size=(samples - 1,) + vel.shape)
    sets = [constant_velocity_tracks(positions, vel, dt, rows)]
    sets += [constant_velocity_tracks(positions, vel + noise[s], dt, rows) for s in range(samples - 1)]
    return np.ascontiguousarray(np.stack(sets), dtype=np.float32)


MAX_DISC_SAMPLES = 16  # (kCrowdSamplesMax of the library)
MAX_FOOTPRINT_DISCS = 8  # (kCrowdFootprintMax of the library)


def rectangle_footprint(front, rear, width, count=None):
    """(count, 3) float32 footprint rows (ox, oy, rho) for params['footprint']: discs on the body axis that cover the
    rectangle [-rear, front] x [-width/2, width/2] of the robot frame.  The rectangle is cut into `count` equal pieces
    along the axis; disc j has its centre in the middle of piece j, at -rear + (j + 1/2) * len / count, and the radius of
    the piece's circumscribed circle, sqrt((len / (2 count))^2 + (width / 2)^2).  count defaults to ceil(len / width),
    clipped to 1 .. 8.  Evaluated in float64 and rounded once."""
    front, rear, width = float(front), float(rear), float(width)
    length = front + rear
    if not (np.isfinite([front, rear, width]).all() and length > 0.0 and width >= 0.0):
        raise ValueError("rectangle_footprint: front + rear > 0 and width >= 0, all finite")
    if count is None:
        count = int(np.ceil(length / width)) if width > 0.0 else MAX_FOOTPRINT_DISCS
        count = min(max(count, 1), MAX_FOOTPRINT_DISCS)
    count = int(count)
    if not 1 <= count <= MAX_FOOTPRINT_DISCS:
        raise ValueError("rectangle_footprint: count {} is not in 1 .. {}".format(count, MAX_FOOTPRINT_DISCS))
    out = np.zeros((count, 3), dtype=np.float64)
    out[:, 0] = -rear + (np.arange(count, dtype=np.float64) + 0.5) * length / count
    out[:, 2] = np.sqrt((length / (2.0 * count)) ** 2 + (width / 2.0) ** 2)
    return np.ascontiguousarray(out.astype(np.float32))


def _footprint_rows(footprint):
    """params['footprint'] as the library takes it: (F, 3) float32, 1 <= F <= 8 (ValueError otherwise)."""
    fp = np.asarray(footprint)
    if fp.ndim != 2 or fp.shape[1] != 3 or not 1 <= fp.shape[0] <= MAX_FOOTPRINT_DISCS:
        raise ValueError("params['footprint'] has shape (F, 3) with 1 <= F <= {}, got {}".format(MAX_FOOTPRINT_DISCS, fp.shape))
    return np.ascontiguousarray(_f32(fp))


MAX_CLEARANCE_RINGS = 4  # (kCrowdRingsMax of the library)
MAX_GUIDE_CELLS = 36864  # (kGuideCellsMax of the library: 192 x 192)
MAX_OCCUPANCY_DIM = 512  # (kOccupancyDimMax of the library)
MAX_OCCUPANCY_SUBSTEPS = 8  # (kOccupancySubstepsMax of the library)


def clearance_staircase(reach, peak, count):
    """(count, 2) float32 rows (margin, penalty) for params['clearance_rings']: margins reach * l / count, l = 1 .. count,
    and penalties c_l = F_l - F_{l+1} with F_l = peak * (1 - (l - 1) / count)**2 and F_{count+1} = 0, evaluated in float64
    and rounded once.  An obstacle at gap g pays F_l for g in (margin_{l-1}, margin_l] -- every ring from l outwards --: the
    staircase on top of peak * (1 - g / reach)**2.  ValueError for reach <= 0, peak < 0 or a count outside 1 .. 4."""
    reach, peak = float(reach), float(peak)
    if not (np.isfinite(reach) and reach > 0.0):
        raise ValueError("clearance_staircase: reach {} is not finite and positive".format(reach))
    if not (np.isfinite(peak) and peak >= 0.0):
        raise ValueError("clearance_staircase: peak {} is negative or not finite".format(peak))
    if isinstance(count, bool) or int(count) != count or not 1 <= int(count) <= MAX_CLEARANCE_RINGS:
        raise ValueError("clearance_staircase: count {} is not in 1 .. {}".format(count, MAX_CLEARANCE_RINGS))
    count = int(count)
    level = np.arange(1, count + 2, dtype=np.float64)
    steps = peak * (1.0 - (level - 1.0) / count) ** 2  # F_1 .. F_{count+1}; the last is 0
    out = np.zeros((count, 2), dtype=np.float64)
    out[:, 0] = reach * level[:count] / count
    out[:, 1] = steps[:count] - steps[1:]
    return np.ascontiguousarray(out.astype(np.float32))


def _ring_rows(rings):
    """params['clearance_rings'] as the library takes it: (R, 2) float32, 1 <= R <= 4 (ValueError otherwise)."""
    rg = np.asarray(rings)
    if rg.ndim != 2 or rg.shape[1] != 2 or not 1 <= rg.shape[0] <= MAX_CLEARANCE_RINGS:
        raise ValueError("params['clearance_rings'] has shape (R, 2) with 1 <= R <= {}, got {}".format(MAX_CLEARANCE_RINGS, rg.shape))
    return np.ascontiguousarray(_f32(rg))


def body_discs(states, footprint):
    """(..., F, 2) float32: the centres of the body's discs at states (..., 3) = (x, y, th), as the rollouts form them --
    the states rounded to float32 first, s, c the float64 sine and cosine of the float32 heading,
    cx = x + (ox * c - oy * s), cy = y + (ox * s + oy * c) in float64 in this order, rounded once.  For drawing."""
    st = _f32(states)
    if st.shape[-1] < 3:
        raise ValueError("states have shape (..., 3), got {}".format(st.shape))
    fp = _footprint_rows(footprint).astype(np.float64)
    x, y, th = (st[..., i, None].astype(np.float64) for i in range(3))
    s, c = np.sin(th), np.cos(th)
    cx = x + (fp[:, 0] * c - fp[:, 1] * s)
    cy = y + (fp[:, 0] * s + fp[:, 1] * c)
    return np.ascontiguousarray(np.stack([cx, cy], axis=-1).astype(np.float32))


def constant_velocity_walls(segments, velocities, dt, rows, at=0.5):
    """(W, rows, 2, 2) float32 wall tracks of walls that keep their velocity: row j is the wall translated by
    velocities * ((j + at) * dt) -- at = 0.5: where it is in the middle of control interval j -- evaluated in float64 and
    rounded once to float32 (at = 0: row 0 is float32(segments)).  segments (W, 2, 2), velocities (W, 2).  A row is tested
    where it lies: a wall fast enough to jump over the robot within one interval is not seen."""
    rows = int(rows)
    assert rows >= 1, "a track has at least one row"
    seg = np.asarray(segments, dtype=np.float64).reshape(-1, 1, 2, 2)
    vel = np.asarray(velocities, dtype=np.float64).reshape(-1, 1, 1, 2)
    assert len(seg) == len(vel), "segments and velocities differ in length"
    times = ((np.arange(rows, dtype=np.float64) + float(at)) * float(dt)).reshape(1, rows, 1, 1)
    return np.ascontiguousarray((seg + vel * times).astype(np.float32))


def swept_walls(tracks):
    """(K, max(L - 1, 1), 2, 2) float32 wall tracks from (K, L, 2) disc tracks: row j is the segment [c_j, c_{j+1}] the
    disc's centre covers during control interval j (L = 1: the degenerate segment [c_0, c_0]).  With half-width
    r_other + r_own it is the capsule another robot sweeps in that interval, tested against the segment this robot covers
    in the same interval -- which closes the hole of the disc tracks, whose rows are instants: two robots that swap places
    within one control step pass each other unseen there.  Conservative: two bodies that move linearly within the
    interval and come within the half-width of each other at some instant of it always hit (their positions at that
    instant lie on the two segments), and so do some near misses -- bodies that pass the same place at different instants
    of the interval."""
    tr = _f32(tracks)
    if tr.ndim != 3 or tr.shape[2] != 2 or tr.shape[1] < 1:
        raise ValueError("tracks have shape (K, L, 2) with L >= 1, got {}".format(tr.shape))
    starts = tr[:, :-1] if tr.shape[1] > 1 else tr
    ends = tr[:, 1:] if tr.shape[1] > 1 else tr
    return np.ascontiguousarray(np.stack([starts, ends], axis=2), dtype=np.float32)


def polyline_walls(points, closed=False):
    """(W, 2, 2) float32 wall segments [[ax, ay], [bx, by]] along a polyline of (P, 2) points: W = P - 1, or P with
    closed=True (a polygon: the last point is joined to the first; fewer than three points close nothing).  Fewer than two
    points: no walls."""
    pts = _f32(points).reshape(-1, 2)
    if len(pts) < 2:
        return np.zeros((0, 2, 2), dtype=np.float32)
    ends = pts[1:]
    starts = pts[:-1]
    if closed and len(pts) >= 3:
        starts, ends = pts, np.roll(pts, -1, axis=0)
    return np.ascontiguousarray(np.stack([starts, ends], axis=1), dtype=np.float32)


def guide_grid(segments, resolution, margin=None):
    """(origin (x, y), shape (ny, nx)) for params['guide']: the bounding box of the wall segments (W, 2, 2), grown by
    `margin` on every side (default: two cells), cut into cells of `resolution`.  ValueError without walls, for a
    resolution that is not positive, or for more than 36864 cells."""
    seg = np.asarray(segments, dtype=np.float64).reshape(-1, 2)
    resolution = float(resolution)
    if not (len(seg) and np.isfinite(seg).all() and np.isfinite(resolution) and resolution > 0.0):
        raise ValueError("guide_grid: at least one finite wall segment and a resolution > 0")
    margin = 2.0 * resolution if margin is None else float(margin)
    lo, hi = seg.min(axis=0) - margin, seg.max(axis=0) + margin
    nx, ny = (max(1, int(np.ceil((hi[i] - lo[i]) / resolution))) for i in range(2))
    if nx * ny > MAX_GUIDE_CELLS:
        raise ValueError("guide_grid: {} x {} cells, more than {}: a coarser resolution".format(ny, nx, MAX_GUIDE_CELLS))
    return (float(lo[0]), float(lo[1])), (ny, nx)


def rasterise_obstacles(origin, resolution, shape, segments=None, halfwidth=0.0, discs=None, radii=None):
    """Cells for params['occupancy']: (ny, nx) uint8, 1 where the cell's centre -- origin + (ix + 0.5, iy + 0.5) *
    resolution -- lies within its half-width of a wall segment (segments (W, 2, 2); halfwidth a scalar or (W,)) or inside a
    disc (discs (K, 2), radii (K,); the rim included), in float64."""
    ny, nx = int(shape[0]), int(shape[1])
    origin = np.asarray(origin, dtype=np.float64).reshape(2)
    res = float(resolution)
    cx = origin[0] + (np.arange(nx, dtype=np.float64) + 0.5) * res
    cy = origin[1] + (np.arange(ny, dtype=np.float64) + 0.5) * res
    X, Y = np.meshgrid(cx, cy)  # (ny, nx)
    cells = np.zeros((ny, nx), dtype=bool)
    if segments is not None:
        seg = np.asarray(segments, dtype=np.float64).reshape(-1, 2, 2)
        hw = np.broadcast_to(np.asarray(halfwidth, dtype=np.float64), (len(seg),))
        for (a, b), h in zip(seg, hw):
            d = b - a
            LL = float(d @ d)
            wx, wy = X - a[0], Y - a[1]
            t = np.clip((wx * d[0] + wy * d[1]) / LL, 0.0, 1.0) if LL > 0.0 else np.zeros_like(X)
            cells |= (wx - t * d[0]) ** 2 + (wy - t * d[1]) ** 2 <= h * h
    if discs is not None:
        pos = np.asarray(discs, dtype=np.float64).reshape(-1, 2)
        rad = np.broadcast_to(np.asarray(radii, dtype=np.float64), (len(pos),))
        for (px, py), r in zip(pos, rad):
            cells |= (X - px) ** 2 + (Y - py) ** 2 <= r * r
    return cells.astype(np.uint8)


def fleet_others(count):
    """(B, B - 1) int: row a holds the other robots of reader a in ascending order -- the order of a fleet's wall slots."""
    count = int(count)
    return np.array([[b for b in range(count) if b != a] for a in range(count)], dtype=np.int64).reshape(count, max(count - 1, 0))


def curvature_of_steering(steer, wheelbase):
    """The path curvature in 1/m of a car whose front wheel is turned by `steer` rad (the bicycle model): tan(steer) /
    wheelbase.  With params['drive'] = 'car', wrange is +-curvature_of_steering(max_steer, wheelbase)."""
    return np.tan(np.asarray(steer, dtype=np.float64)) / np.asarray(wheelbase, dtype=np.float64)


def steering_of_curvature(kappa, wheelbase):
    """The steering angle in rad that follows a curvature: arctan(wheelbase * kappa) -- what to command from a car plan's
    second component."""
    return np.arctan(np.asarray(wheelbase, dtype=np.float64) * np.asarray(kappa, dtype=np.float64))


def _is_track_set(obstacle_set):
    return np.asarray(obstacle_set[0]).ndim == 3


def _is_wall_track_set(wall_set):
    return np.asarray(wall_set[0]).ndim == 4


def _same_sets(new, now):
    """Whether two lists of per-problem sets -- arrays, or tuples of arrays -- hold the same values."""
    return all(np.array_equal(x, y) for a, b in zip(new, now) for x, y in (zip(a, b) if isinstance(a, tuple) else ((a, b),)))


# ---------------------------------------------------------------------- what the library holds
_STALE = "stale"  # a key: what the library holds of this kind is out of date -- hand the params' value over again, or clear
_NOBODY, _PARAMS, _BATCH = "nobody", "params", "batch"  # who filled a slot (_BATCH: MPPI_Batch's per-problem sets)
_KEEP, _FETCH, _ZERO = "keep", "fetch", "zero"  # what a change of a kind does to the mirror's track offsets
_CTYPES = {np.dtype(np.float32): C.c_float, np.dtype(np.int32): C.c_int, np.dtype(np.uint8): C.c_ubyte}


class _Held:
    """What the library holds of one kind of set.
    key    the bytes of the params value that was handed over (None: nothing of params; _STALE, above)
    owner  who filled the slot: _NOBODY, _PARAMS or -- the three track kinds -- _BATCH, whose per-problem sets win over the
           shared key of params; when they go the slot is free and that key is handed over again at the next solve
    sent   the setter's arguments the library holds, whoever sent them (None: nothing): the rows of the wall tracks, the
           goal tracks and the number of disc samples are read from here"""
    __slots__ = ("key", "owner", "sent")

    def __init__(self):
        self.key, self.owner, self.sent = None, _NOBODY, None


def _pack_sets(sets, what, noun, others, width, prepare, finish=None):
    """The packer of "a list of per-problem sets with a common row count": prepare(b, sets[b]) validates set b and gives
    its array (count_b, L, ...), finish(b, array) validates what is looked at behind the row count; returns
    (counts (len(sets),) int32, L, one contiguous float32 block (sum count_b * L, width))."""
    rows, counts, flat = None, [], []
    for b, one in enumerate(sets):
        tr = prepare(b, one)
        if tr.shape[1] < 1:
            raise ValueError("{} {}: {} has at least one row (L = 0)".format(what, b, noun))
        if rows not in (None, tr.shape[1]):
            raise ValueError("{} {}: {} rows, other {} of this call have {}".format(what, b, tr.shape[1], others, rows))
        rows = tr.shape[1]
        if finish is not None:
            finish(b, tr)
        counts.append(len(tr))
        flat.append(_f32(tr).reshape(-1, width))
    return np.ascontiguousarray(counts, dtype=np.int32), int(rows), np.ascontiguousarray(np.concatenate(flat), dtype=np.float32)


def _pack_disc_tracks(sets):
    """sets: one (tracks (K, L, 2), radii (K,)) pair for every problem, or one per problem."""
    rad = [_f32(np.asarray(orad)).reshape(-1) for _, orad in sets]

    def prepare(b, pair):
        tr = np.asarray(pair[0])
        if tr.ndim != 3 or tr.shape[2] != 2:
            raise ValueError("set {}: tracks have shape (K, L, 2), got {}".format(b, tr.shape))
        if tr.shape[1] >= 1 and len(tr) != len(rad[b]):  # (a set without rows is refused first, by the packer)
            raise ValueError("set {}: {} tracks and {} radii".format(b, len(tr), len(rad[b])))
        return tr
    counts, rows, pos_all = _pack_sets(sets, "set", "a track", "sets", 2, prepare)
    return len(sets), counts, rows, pos_all, np.ascontiguousarray(np.concatenate(rad), dtype=np.float32)


def _pack_wall_tracks(sets, what="wall set"):
    """sets: one (tracks (W, L, 2, 2) or segments (W, 2, 2), half-widths: a scalar or (W,)) pair for every problem, or
    one per problem."""
    halves = []

    def prepare(b, pair):
        tr = np.asarray(pair[0])
        shown = tr.shape
        if tr.ndim == 3:  # a static set: tracks of one row
            tr = tr.reshape(len(tr), 1, *tr.shape[1:])
        if tr.ndim != 4 or (tr.size and tr.shape[2:] != (2, 2)):
            raise ValueError("{} {}: shape (W, L, 2, 2) -- or (W, 2, 2) for static walls --, got {}".format(what, b, shown))
        return tr

    def finish(b, tr):
        hw = np.asarray(sets[b][1])
        if hw.ndim not in (0, 1) or (hw.ndim == 1 and len(hw) != len(tr)):
            raise ValueError("{} {}: the half-width is a scalar or has shape ({},), got {}".format(what, b, len(tr), hw.shape))
        halves.append(np.broadcast_to(_f32(hw), (len(tr),)))
    counts, rows, seg_all = _pack_sets(sets, what, "a wall track", "sets", 4, prepare, finish)
    return len(sets), counts, rows, seg_all, np.ascontiguousarray(np.concatenate(halves), dtype=np.float32)


def _pack_goal_tracks(planner, tracks, what="goal track"):
    """tracks: one (L, 2) goal track for every problem, or one per problem with a common L."""
    def prepare(b, tr):
        tr = np.asarray(tr)
        if tr.ndim != 2 or tr.shape[1] != 2:
            raise ValueError("{} {}: shape (L, 2), got {}".format(what, b, tr.shape))
        return tr[None]
    _, rows, xy = _pack_sets(tracks, what, "a goal track", "tracks", 2, prepare)
    if len(tracks) not in (1, planner.num_instances):
        raise ValueError("{} goal tracks: one for every problem, or one per problem ({})".format(len(tracks), planner.num_instances))
    return len(tracks), rows, xy.reshape(len(tracks), rows, 2)


# The params-owned kinds: what MPPI_Numba._sync_kind needs to know of each.  read(planner, params) runs where the kind's
# key is in params, whether or not its value has changed: it refuses what the kind excludes and gives the arrays whose bytes
# are the key (None: treat the key as absent).  pack(planner, *arrays) runs when those bytes are new: it validates and gives
# the setter's arguments, arrays as arrays.
def _read_one(key):
    return lambda planner, p: (np.asarray(p[key]),)


def _read_goal(planner, p):
    if "xgoal" in p:
        raise ValueError("params hold both 'xgoal' and 'goal_track': the goal is static or has a track, give one of the two")
    tr = np.asarray(p['goal_track'])
    if tr.ndim != 2 or tr.shape[1] != 2:
        raise ValueError("params['goal_track'] has shape (L, 2), got {}".format(tr.shape))
    return (tr,)


def _read_guide(planner, p):
    if "goal_track" in p:
        raise ValueError("params hold both 'goal_track' and 'guide': the guide owns the goal rows, give one of the two")
    if "xgoal" not in p:
        raise ValueError("params['guide'] needs params['xgoal']: the field is measured from it")
    g = p['guide']
    shape = np.asarray(g['shape'])
    if shape.shape != (2,) or shape.dtype.kind not in "iu" or (shape < 1).any() or int(shape[0]) * int(shape[1]) > MAX_GUIDE_CELLS:
        raise ValueError("params['guide']['shape'] is (ny, nx), integers >= 1 with ny * nx <= {}, got {}".format(MAX_GUIDE_CELLS, g['shape']))
    origin = np.asarray(g['origin'], dtype=np.float64).reshape(-1)
    if origin.shape != (2,):
        raise ValueError("params['guide']['origin'] is (x, y), got {}".format(g['origin']))
    res = float(g['resolution'])
    pace = float(g['pace']) if 'pace' in g else float(p['vrange'][1]) * float(p['dt'])
    lead = float(g['lead']) if 'lead' in g else 2.0 * pace
    inflate = float(g['inflate']) if 'inflate' in g else res
    return _f32([origin[0], origin[1], res, inflate, lead, pace]), shape.astype(np.int32)


def _pack_guide(planner, values, shape):
    """Values that are not finite, a resolution <= 0, an inflation below resolution / sqrt(2), goal tracks held per problem:
    the library refuses them (MppiError) and keeps what it had."""
    x, y, res, inflate, lead, pace = (float(v) for v in values)
    return 1, x, y, res, int(shape[1]), int(shape[0]), inflate, lead, pace


def _read_occupancy(planner, p):
    if "obstacle_track_samples" in p:
        raise ValueError("params hold both 'occupancy' and 'obstacle_track_samples': the sample forms look up no grid, give one of the two")
    g = p['occupancy']
    cells = np.asarray(g['cells'])
    if cells.ndim != 2 or cells.dtype.kind not in "iub" or not (1 <= cells.shape[0] <= MAX_OCCUPANCY_DIM and 1 <= cells.shape[1] <= MAX_OCCUPANCY_DIM):
        raise ValueError("params['occupancy']['cells'] is (ny, nx) of an integer or bool dtype with 1 <= ny, nx <= {}, got {} {}".format(
            MAX_OCCUPANCY_DIM, cells.dtype, cells.shape))
    origin = np.asarray(g['origin'], dtype=np.float64).reshape(-1)
    if origin.shape != (2,):
        raise ValueError("params['occupancy']['origin'] is (x, y), got {}".format(g['origin']))
    substeps = g.get('substeps', 1)
    if isinstance(substeps, bool) or not isinstance(substeps, (int, np.integer)) or not 1 <= int(substeps) <= MAX_OCCUPANCY_SUBSTEPS:
        raise ValueError("params['occupancy']['substeps'] is an int in 1 .. {}, got {!r}".format(MAX_OCCUPANCY_SUBSTEPS, substeps))
    values = _f32([origin[0], origin[1], float(g['resolution']), float(g.get('inflate', 0.0))])
    return values, np.asarray([int(substeps)], dtype=np.int32), np.ascontiguousarray(cells != 0, dtype=np.uint8)


def _pack_occupancy(planner, values, substeps, cells):
    """Values that are not finite, a resolution <= 0, a negative inflation, no crowd mode, disc samples held: the library
    refuses them (MppiError) and keeps what it had."""
    x, y, res, inflate = (float(v) for v in values)
    return 1, x, y, res, int(cells.shape[1]), int(cells.shape[0]), inflate, int(substeps[0]), cells


def _pack_smoothing(planner, sm):
    """A wrong shape is refused here; a value outside [0, 1), the xoroshiro generator: the library refuses them (MppiError)
    and keeps what it had."""
    if sm.shape not in ((), (2,)):
        raise ValueError("params['noise_smoothing'] is a scalar or has shape (2,), got {}".format(sm.shape))
    return (np.ascontiguousarray(np.broadcast_to(_f32(sm), (2,))),)


def _pack_limits(planner, acc):
    """A wrong shape is refused here; a value that is NaN or <= 0: the library refuses it (MppiError) and keeps what it had."""
    if acc.shape not in ((), (2,)):
        raise ValueError("params['accel_limits'] is a scalar or has shape (2,), got {}".format(acc.shape))
    return (np.ascontiguousarray(np.broadcast_to(_f32(acc), (2,))),)


_DRIVES = {"unicycle": _lib.DRIVE_UNICYCLE, "car": _lib.DRIVE_CAR}


def _read_drive(planner, p):
    """'unicycle' is the key left out (None): nothing is handed over unless a car was."""
    drive = p['drive']
    if not isinstance(drive, str) or drive not in _DRIVES:
        raise ValueError("params['drive'] is 'unicycle' or 'car', got {!r}".format(drive))
    return None if drive == "unicycle" else (np.asarray([_DRIVES[drive]], dtype=np.int32),)


def _read_wall_tracks(planner, p):
    if planner._held["fleet"].sent is not None or planner._held["fleet_bodies"].sent is not None:
        raise ValueError("params hold 'wall_tracks' while the fleet is on: the fleet makes every problem's wall set "
                         "itself (set_fleet(None) first; 'wall_segments' stay in force beside it)")
    if "wall_segments" in p:
        raise ValueError("params hold both 'wall_segments' and 'wall_tracks': walls are static or have tracks, "
                         "give one of the two")
    tr = np.asarray(p['wall_tracks'])
    if tr.ndim != 4:
        raise ValueError("params['wall_tracks'] has shape (W, L, 2, 2), got {}".format(tr.shape))
    return tr, np.asarray(p.get('wall_halfwidth', 0.0))


def _read_walls(planner, p):
    return np.asarray(p['wall_segments']), np.asarray(p.get('wall_halfwidth', 0.0))


def _pack_walls(planner, seg, hw):
    """Without crowd mode the library refuses walls (MppiError)."""
    if seg.size and seg.shape[1:] != (2, 2):
        raise ValueError("params['wall_segments'] has shape (W, 2, 2), got {}".format(seg.shape))
    segs = np.ascontiguousarray(_f32(seg).reshape(-1, 4))
    if hw.ndim not in (0, 1) or (hw.ndim == 1 and len(hw) != len(segs)):
        raise ValueError("params['wall_halfwidth'] is a scalar or has shape ({},), got {}".format(len(segs), hw.shape))
    return segs, np.ascontiguousarray(np.broadcast_to(_f32(hw), (len(segs),))), len(segs)


def _read_footprint(planner, p):
    if planner._held["fleet"].sent is not None:
        raise ValueError("params hold 'footprint' while the fleet is on: the fleet's half-widths already contain the "
                         "reader's body (set_fleet(None) first, or drop the key)")
    if planner._held["fleet_bodies"].sent is not None:
        raise ValueError("params hold 'footprint' while the fleet of bodies is on: that fleet carries its own body "
                         "(set_fleet(None) first, or drop the key)")
    return (np.asarray(p['footprint']),)


def _pack_rows(rows_of):
    """Footprint and rings: (rows, count).  Without crowd mode -- rings: beside disc samples, or with a bad row -- the
    library refuses them (MppiError)."""
    def pack(planner, value):
        rows = rows_of(value)
        return rows, len(rows)
    return pack


def _read_samples(planner, p):
    others = [k for k in ("obstacle_positions", "obstacle_tracks") if k in p]
    if others:
        raise ValueError("params hold both 'obstacle_track_samples' and '{}': discs are static, have tracks or have "
                         "sampled tracks, give one of the three".format(others[0]))
    if planner._held["problem_discs"].sent is not None:
        raise ValueError("params hold 'obstacle_track_samples' while obstacle_sets are held: disc samples are shared by "
                         "every problem (set_obstacle_sets(None) first)")
    return np.asarray(p['obstacle_track_samples']), np.asarray(p['obstacle_radius'])


def _pack_samples(planner, smp, orad):
    """Once the samples have passed, the plain tracks that params held go, ahead of the samples' own hand-over."""
    if smp.ndim != 4 or smp.shape[3] != 2 or smp.shape[0] < 1 or smp.shape[2] < 1:
        raise ValueError("params['obstacle_track_samples'] has shape (S, K, L, 2) with S, L >= 1, got {}".format(smp.shape))
    if smp.shape[0] > MAX_DISC_SAMPLES:
        raise ValueError("params['obstacle_track_samples'] holds {} samples, more than {}".format(smp.shape[0], MAX_DISC_SAMPLES))
    rad = np.ascontiguousarray(_f32(orad).reshape(-1))
    if len(rad) != smp.shape[1]:
        raise ValueError("params['obstacle_track_samples'] holds {} discs, params['obstacle_radius'] {} radii".format(
            smp.shape[1], len(rad)))
    tracks = planner._held["tracks"]
    if tracks.owner is _PARAMS:  # (the params no longer hold them; "now" is fetched behind the samples)
        _lib.call(_TRACKS.setter, planner._handle, *_TRACKS.clear)
        tracks.key, tracks.owner, tracks.sent = None, _NOBODY, None
    pos = np.ascontiguousarray(_f32(smp))
    return (int(smp.shape[0]), int(smp.shape[1]), int(smp.shape[2]), pos if pos.size else np.zeros(2, np.float32),
            rad if rad.size else np.zeros(1, np.float32))


def _read_tracks(planner, p):
    if "obstacle_positions" in p:
        raise ValueError("params hold both 'obstacle_positions' and 'obstacle_tracks': discs are static or have "
                         "tracks, give one of the two")
    return np.asarray(p['obstacle_tracks']), np.asarray(p['obstacle_radius'])


def _read_discs(planner, p):
    return (np.asarray(p['obstacle_positions']), np.asarray(p['obstacle_radius'])) if "obstacle_radius" in p else None


def _pack_discs(planner, op, orad):
    pos = np.ascontiguousarray(_f32(op).reshape(-1, 2))
    rad = np.ascontiguousarray(_f32(orad).reshape(-1))
    assert len(pos) == len(rad)
    return pos, rad, len(rad)


# One row per hand-over, in hand-over order -- the one place that states it.  The goal's row is walked ahead of the params
# struct (whose xgoal rests on it), the others behind it.
#   name    the kind's record in MPPI_Numba._held        key     the params key whose presence means "there is one"
#   read, pack  above (pack None: this row only clears)  setter  the library's entry point
#   clear   the setter's arguments that clear (None: this row only sets)
#   offsets what a change does to the mirror's track offsets: _KEEP, _FETCH from the library (new rows, or rows that have
#           gone: row 0 is "now", unless other tracks count the rows), _ZERO here (disc tracks: row 0 is "now")
#   over    the kind this one lies over: that kind rests while this one's key is in params, and is stale after a change
#   excludes  kinds the library refuses beside this one: what params no longer hold of them is cleared ahead of this
#           kind's hand-over (the guide owns the goal rows: a guide that has gone makes way for the goal track)
# Rings and disc samples exclude each other in the library: rings that have gone are cleared ahead of the samples'
# hand-over, rings that are there are handed over behind it -- hence two rows.
_Kind = collections.namedtuple("_Kind", "name key read pack setter clear offsets over excludes", defaults=((),))
_KINDS = (
    _Kind("goal", "goal_track", _read_goal, lambda planner, tr: _pack_goal_tracks(planner, [tr], "params['goal_track']"),
          "mppi_planner_set_goal_tracks", (0, 0, None), _FETCH, None, ("guide",)),
    _Kind("smoothing", "noise_smoothing", _read_one("noise_smoothing"), _pack_smoothing,
          "mppi_planner_set_noise_smoothing", (None,), _KEEP, None),
    _Kind("limits", "accel_limits", _read_one("accel_limits"), _pack_limits,
          "mppi_planner_set_control_limits", (None,), _KEEP, None),
    _Kind("drive", "drive", _read_drive, lambda planner, drive: (int(drive[0]),), "mppi_planner_set_drive", (0,), _KEEP, None),
    _Kind("wall_tracks", "wall_tracks", _read_wall_tracks,
          lambda planner, tr, hw: _pack_wall_tracks([(tr, hw)], "params['wall_tracks']"),
          "mppi_planner_set_wall_tracks", (0, None, 0, None, None), _FETCH, None),
    _Kind("walls", "wall_segments", _read_walls, _pack_walls, "mppi_planner_set_walls", (None, None, 0), _KEEP, None),
    _Kind("occupancy", "occupancy", _read_occupancy, _pack_occupancy,
          "mppi_planner_set_occupancy", (0, 0.0, 0.0, 1.0, 1, 1, 0.0, 1, None), _KEEP, None, ("samples",)),
    _Kind("guide", "guide", _read_guide, _pack_guide, "mppi_planner_set_guide", (0, 0.0, 0.0, 1.0, 1, 1, 1.0, 0.0, 0.0), _KEEP, None),
    _Kind("footprint", "footprint", _read_footprint, _pack_rows(_footprint_rows),
          "mppi_planner_set_footprint", (None, 0), _KEEP, None),
    _Kind("rings", "clearance_rings", _read_one("clearance_rings"), None,
          "mppi_planner_set_clearance_rings", (None, 0), _KEEP, None),
    _Kind("samples", "obstacle_track_samples", _read_samples, _pack_samples,
          "mppi_planner_set_disc_track_samples", (0, 0, 0, None, None), _FETCH, "discs"),
    _Kind("rings", "clearance_rings", _read_one("clearance_rings"), _pack_rows(_ring_rows),
          "mppi_planner_set_clearance_rings", None, _KEEP, None),
    _Kind("tracks", "obstacle_tracks", _read_tracks, lambda planner, tr, orad: _pack_disc_tracks([(tr, orad)]),
          "mppi_planner_set_disc_tracks", (0, None, 0, None, None), _ZERO, "discs"),
    _Kind("discs", "obstacle_positions", _read_discs, _pack_discs, "mppi_planner_set_disc_obstacles", (None, None, 0), _KEEP, None),
)
_GOAL, _WALL_TRACKS, _FOOTPRINT, _TRACKS, _DISCS = (
    next(kind for kind in _KINDS if kind.name == name) for name in ("goal", "wall_tracks", "footprint", "tracks", "discs"))
_OPTIONAL_KEYS = frozenset(kind.key for kind in _KINDS if kind is not _DISCS)  # (the discs are there in every solve)
_OPTIONAL_NAMES = tuple(sorted({kind.name for kind in _KINDS if kind is not _DISCS}))
_RESTS_UNDER = {kind.name: tuple(k.key for k in _KINDS if k.over == kind.name) for kind in _KINDS}  # name -> the keys above it


class MPPI_Numba(object):

    """Information-theoretic MPPI (Williams et al., Alg. 2) without maps.
    Workflow: MPPI_Numba(cfg) -> setup(params) -> solve() -> get_state_rollout()
    -> shift_and_update(next_state, useq)."""

    def __init__(self, cfg):
        self.cfg = cfg
        self.num_instances = int(getattr(self, "num_instances", 1))  # (MPPI_Batch sets it first)
        self.T = cfg.T
        self.dt = cfg.dt
        self.num_steps = cfg.num_steps
        self.num_control_rollouts = cfg.num_control_rollouts
        self.num_vis_state_rollouts = cfg.num_vis_state_rollouts
        self.seed = cfg.seed
        self.max_threads_per_block = cfg.max_threads_per_block
        self._handle = None
        self.noise_samples_d = None
        self.u_cur_d = None
        self.u_prev_d = None
        self.costs_d = None
        self.weights_d = None
        self.rng_states_d = None
        self.state_rollout_batch_d = None
        self.device_var_initialized = False
        # what the library holds: a record per kind of _KINDS, and of MPPI_Batch: "problem_discs", the per-problem disc sets
        # of either kind (sent: its obstacle_sets); "fleet", sent = (radii (B,), margin, half-widths (B, B - 1)); "fleet_bodies",
        # sent = (rows (F, 3), margin)
        self._held = {name: _Held() for name in _OPTIONAL_NAMES + ("discs", "problem_discs", "fleet", "fleet_bodies")}
        self._held["discs"].key = _STALE  # (nothing handed over yet: the first solve hands the discs over, or clears)
        self._walk_all = False  # whether something of an optional kind is held of params (or a walk of _KINDS broke off)
        self.reset()

    def __del__(self):
        handle, self._handle = getattr(self, "_handle", None), None
        if handle is not None:
            try:
                _lib.load().mppi_planner_destroy(handle)
            except Exception:
                pass

    def reset(self):
        self.u_seq0 = np.zeros((self.num_steps, 2), dtype=np.float32)
        self.params = None
        self.params_set = False
        self.u_prev_d = None
        self.init_device_vars_before_solving()
        self.set_track_offset(0)

    # ------------------------------------------------------------------ discs that move
    @property
    def track_offset(self):
        """The row of the disc tracks that is "now": an int, a (B,) int32 array for a batch."""
        return int(self._track_offset[0]) if self.num_instances == 1 else self._track_offset.copy()

    def set_track_offset(self, offset):
        """An int (every problem) or one per problem; >= 0.  Past the last row: the discs stay at their last place."""
        off = np.ascontiguousarray(np.broadcast_to(np.asarray(offset, dtype=np.int64), (self.num_instances,)), dtype=np.int32)
        assert (off >= 0).all(), "track offsets are >= 0"
        _lib.call("mppi_planner_set_track_offsets", self._handle, self.num_instances, _lib.ptr(off, C.c_int))
        self._track_offset = off

    def _fetch_track_offset(self):
        off = np.zeros(self.num_instances, dtype=np.int32)
        _lib.call("mppi_planner_get_track_offsets", self._handle, self.num_instances, _lib.ptr(off, C.c_int))
        self._track_offset = off

    # ------------------------------------------------------------------ crowd mode
    @property
    def crowd(self):
        """Whether the handle is in crowd mode (set_crowd)."""
        on = C.c_int(0)
        _lib.call("mppi_planner_get_crowd", self._handle, C.byref(on))
        return bool(on.value)

    def set_crowd(self, on):
        """Crowd mode: disc sets of any size -- the 64 KiB LDS limits of the default forms do not apply -- and, above a
        handful of discs, a rollout kernel that counts every step's hits in parallel; same results bit for bit.
        Turning it off raises MppiError (and stays on) while the handle holds a set the default forms cannot launch."""
        _lib.call("mppi_planner_set_crowd", self._handle, int(bool(on)))

    # ------------------------------------------------------------------ hand-overs
    def _send(self, kind, args, key=None, owner=_NOBODY):
        """One call of a kind's setter -- args None: its clearing form -- and what goes with it: the kind's record, the
        kind it lies over, the track offsets."""
        _lib.call(kind.setter, self._handle, *[_lib.ptr(a, _CTYPES[a.dtype]) if isinstance(a, np.ndarray) else a
                                               for a in (kind.clear if args is None else args)])
        rec = self._held[kind.name]
        rec.key, rec.owner, rec.sent = key, owner, args
        if kind.over is not None:
            self._held[kind.over].key = _STALE
        if kind.offsets is _FETCH:
            self._fetch_track_offset()
        elif kind.offsets is _ZERO:
            self._track_offset = np.zeros(self.num_instances, dtype=np.int32)

    def _sync_kind(self, p, kind):
        """The hand-over of one params-owned kind.  Its key absent: cleared if something of params is held, else nothing.
        Its key there: nothing if the bytes are those held -- or per-problem sets own the slot --, else packed, handed over
        and remembered."""
        rec = self._held[kind.name]
        values = kind.read(self, p) if kind.key in p else None
        if values is None:
            if rec.key is not None and kind.clear is not None:
                self._send(kind, None)
            return
        key = [(v.dtype, v.shape, v.tobytes()) for v in values]  # (dtype.str would cost more than the rest of the key)
        if key != rec.key and rec.owner is not _BATCH and kind.pack is not None:
            args = kind.pack(self, *values)
            for other in (k for k in _KINDS if k.name in kind.excludes and k.clear is not None):
                if self._held[other.name].key is not None and other.key not in p:
                    self._send(other, None)
            self._send(kind, args, key, _PARAMS)

    def _sync(self, p, kinds):
        for kind in kinds:
            if not any(key in p for key in _RESTS_UNDER[kind.name]):
                self._sync_kind(p, kind)

    def _own_slot(self, kind, held, now=None, pack=None):
        """The owner rule of the three track kinds, for MPPI_Batch's per-problem sets `held` (`now`: those of before).
        None: they go -- the slot is free, and the shared key of params is handed over again at the next solve.  Unchanged:
        nothing, "now" stays where it is.  Else they take the slot, and the caller keeps `held`: returns True."""
        rec = self._held[kind.name]
        if held is None:
            if rec.owner is _BATCH:
                self._send(kind, None)
        elif not (rec.owner is _BATCH and now is not None and _same_sets(held, now)):
            self._send(kind, pack(), None, _BATCH)
            return True
        return False

    # ------------------------------------------------------------------ a body footprint
    @property
    def footprint(self):
        """The footprint the library holds: (F, 3) float32, or None (the robot is its reference point).  While a fleet of
        bodies is on: the rows of its body."""
        rows, count = np.zeros((MAX_FOOTPRINT_DISCS, 3), dtype=np.float32), C.c_int(0)
        _lib.call("mppi_planner_get_footprint", self._handle, _lib.ptr(rows, C.c_float), C.byref(count))
        return rows[:count.value].copy() if count.value else None

    # ------------------------------------------------------------------ clearance rings
    @property
    def clearance_rings(self):
        """The clearance rings the library holds: (R, 2) float32 rows (margin, penalty), or None."""
        rows, count = np.zeros((MAX_CLEARANCE_RINGS, 2), dtype=np.float32), C.c_int(0)
        _lib.call("mppi_planner_get_clearance_rings", self._handle, _lib.ptr(rows, C.c_float), C.byref(count))
        return rows[:count.value].copy() if count.value else None

    # ------------------------------------------------------------------ time-correlated noise
    @property
    def noise_smoothing(self):
        """The smoothing coefficients the library holds: (2,) float32 (beta_v, beta_w), or None (white noise)."""
        beta = np.zeros(2, dtype=np.float32)
        _lib.call("mppi_planner_get_noise_smoothing", self._handle, _lib.ptr(beta, C.c_float))
        return beta if beta.any() else None

    # ------------------------------------------------------------------ acceleration limits
    @property
    def accel_limits(self):
        """The acceleration limits the library holds: (2,) float32 (a_v, a_w), or None."""
        acc, held = np.zeros(2, dtype=np.float32), C.c_int(0)
        _lib.call("mppi_planner_get_control_limits", self._handle, _lib.ptr(acc, C.c_float), C.byref(held))
        return acc if held.value else None

    # ------------------------------------------------------------------ car-like steering
    @property
    def drive(self):
        """The vehicle the library holds: 'unicycle', or 'car' (params['drive']: the second control is the curvature)."""
        drive = C.c_int(0)
        _lib.call("mppi_planner_get_drive", self._handle, C.byref(drive))
        return next(name for name, value in _DRIVES.items() if value == drive.value)

    @property
    def applied_control(self):
        """The control in force when the next plan starts -- the anchor the limits count from: (2,) float32, (B, 2) for a
        batch.  Zero at first; set_applied_control(), shift_and_update() while 'accel_limits' is in params, and
        closed_loop() set it."""
        rows = np.zeros((self.num_instances, 2), dtype=np.float32)
        _lib.call("mppi_planner_get_applied_control", self._handle, _lib.ptr(rows, C.c_float))
        return rows[0] if self.num_instances == 1 else rows

    def set_applied_control(self, u):
        """(2,) = (v, w): every problem's; (B, 2): one per problem.  Finite (else MppiError)."""
        rows = np.asarray(u)
        if rows.shape not in ((2,), (1, 2), (self.num_instances, 2)):
            raise ValueError("an applied control has shape (2,) or ({}, 2), got {}".format(self.num_instances, rows.shape))
        rows = np.ascontiguousarray(_f32(rows).reshape(-1, 2))
        _lib.call("mppi_planner_set_applied_control", self._handle, len(rows), _lib.ptr(rows, C.c_float))

    def limit_noise(self):
        """The pass alone, over the block the handle holds (stage level: set_noise() stores what it is given); MppiError
        while no limits are held."""
        self.move_mppi_task_vars_to_device()
        _lib.call("mppi_planner_limit_noise", self._handle)

    def _anchor_after_shift(self, u_cur, num_shifts):
        # the control applied last becomes the anchor of the next plan -- only while the key is there
        if "accel_limits" in self.params:
            u = np.asarray(u_cur, dtype=np.float32).reshape(self.num_instances, self.num_steps, 2)
            self.set_applied_control(u[:, int(num_shifts) - 1])

    # ------------------------------------------------------------------ a goal that moves
    def _goal_track_on(self):
        goal = self._held["goal"]
        return goal.sent is not None and goal.sent[1] > 1  # (sent: count, rows, the tracks (1 or B, L, 2) float32)

    @property
    def goal_now(self):
        """The goal where it is now: row min(track_offset, L - 1) of the goal track -- (2,) float32, (B, 2) for a batch --
        or the static goal when no track is set.  The closed loop's goal test of a new state, after shift_and_update."""
        goal = self._held["goal"]
        tracks = None if goal.sent is None else goal.sent[2]
        if goal.owner is not _BATCH and self.params is not None:  # (params['goal_track'] may not have been handed over yet)
            tracks = _f32(self.params['goal_track'])[None] if "goal_track" in self.params else None
        if tracks is None:
            if self.num_instances > 1:
                return np.array(self.goals, dtype=np.float32)
            return _f32(self.params['xgoal']).reshape(-1)[:2].copy()
        rows = np.minimum(self._track_offset.astype(np.int64), tracks.shape[1] - 1)
        now = tracks[np.arange(self.num_instances) % len(tracks), rows]
        return now[0].copy() if self.num_instances == 1 else now.copy()

    # ------------------------------------------------------------------ a guide round the walls
    def _guide_sent(self, what):
        sent = self._held["guide"].sent
        if sent is None:
            raise ValueError("{}: no guide is held (params['guide'])".format(what))
        return sent  # (on, x_min, y_min, res, nx, ny, inflate, lead, pace)

    def refresh_guide(self):
        """The refresh alone, as solve() makes it at its head: the field if the guide, the walls or a goal changed, then
        the rows from the current start states.  For drawing and for tests; guide_field() / guide_rows() fetch the result."""
        self.move_mppi_task_vars_to_device()
        self._guide_sent("refresh_guide")
        _lib.call("mppi_planner_guide_refresh", self._handle)

    def guide_field(self):
        """The field of the last build: (ny, nx) uint32 -- (B, ny, nx) for a batch --, 0xFFFFFFFF a blocked cell, 0xFFFFFFFE
        a free cell without a path, else the length of the shortest path to the goal's cell in units of resolution / 12."""
        sent = self._guide_sent("guide_field")
        lead = () if self.num_instances == 1 else (self.num_instances,)
        out = np.empty(lead + (sent[5], sent[4]), dtype=np.uint32)
        _lib.call("mppi_planner_get_guide_field", self._handle, _lib.ptr(out, C.c_uint))
        return out

    def _guide_rows_and_status(self, what):
        self._guide_sent(what)
        B = self.num_instances
        xy, status = np.empty((B, self.num_steps + 1, 2), dtype=np.float32), np.empty(B, dtype=np.int32)
        _lib.call("mppi_planner_get_guide_rows", self._handle, _lib.ptr(xy, C.c_float), _lib.ptr(status, C.c_int))
        return (xy[0], int(status[0])) if B == 1 else (xy, status)

    def guide_rows(self):
        """The rows of the last refresh: (T + 1, 2) float32 -- (B, T + 1, 2) for a batch.  Row 0 is the carrot now; step t
        of a rollout is measured against row t + 1."""
        return self._guide_rows_and_status("guide_rows")[0]

    def guide_status(self):
        """Of the last refresh, an int -- (B,) int32 for a batch: 0, or 1 (the goal's cell is blocked) or 2 (no way out of
        the start's cell), where every row is the goal."""
        return self._guide_rows_and_status("guide_status")[1]

    @property
    def guide_fields_built(self):
        """How often the handle has built the field since it was created (0 while no guide is held)."""
        on, nx, ny, built = C.c_int(0), C.c_int(0), C.c_int(0), C.c_ulonglong(0)
        _lib.call("mppi_planner_get_guide", self._handle, C.byref(on), C.byref(nx), C.byref(ny), C.byref(built))
        return int(built.value)

    # ------------------------------------------------------------------ occupancy-grid obstacles
    def _occupancy_sent(self, what):
        sent = self._held["occupancy"].sent
        if sent is None:
            raise ValueError("{}: no occupancy grid is held (params['occupancy'])".format(what))
        return sent  # (on, x_min, y_min, res, nx, ny, inflate, substeps, cells)

    def refresh_occupancy(self):
        """The clearance field's build alone, as solve() makes it at its head when the cells changed.  For drawing and for
        tests; occupancy_field() fetches the result."""
        self.move_mppi_task_vars_to_device()
        self._occupancy_sent("refresh_occupancy")
        _lib.call("mppi_planner_occupancy_refresh", self._handle)

    def occupancy_field(self):
        """The clearance field of the cells held: (ny, nx) uint32, the squared distance in cells to the nearest occupied cell
        -- 0 on an occupied cell, 0xFFFFFFFF everywhere when none is occupied.  Builds it first if the cells are new."""
        self.refresh_occupancy()
        sent = self._occupancy_sent("occupancy_field")
        out = np.empty((sent[5], sent[4]), dtype=np.uint32)
        _lib.call("mppi_planner_get_occupancy_field", self._handle, _lib.ptr(out, C.c_uint))
        return out

    @property
    def occupancy_fields_built(self):
        """How often the handle has built the clearance field since it was created (0 while no grid was ever held)."""
        on, nx, ny, built = C.c_int(0), C.c_int(0), C.c_int(0), C.c_ulonglong(0)
        _lib.call("mppi_planner_get_occupancy", self._handle, C.byref(on), C.byref(nx), C.byref(ny), C.byref(built))
        return int(built.value)

    def _tracks_on(self):
        return self._held["tracks"].sent is not None or self._held["samples"].sent is not None

    def _wall_tracks_on(self):
        walls = self._held["wall_tracks"]
        return walls.sent is not None and walls.sent[2] > 1  # (sent: sets, counts, rows -- 1: static sets --, ...)

    # ------------------------------------------------------------------ disc samples
    def record_sample_costs(self):
        """From the next rollout on the per-sample costs are kept (while disc samples are held); sample_costs() fetches."""
        self.move_mppi_task_vars_to_device()
        _lib.call("mppi_planner_get_sample_costs", self._handle, None)

    def sample_costs(self):
        """(N, S) float32 -- (B, N, S) for a batch: every rollout's cost under each disc sample, before the CVaR tail, in
        sample order."""
        samples = self._held["samples"]
        if samples.sent is None:
            raise ValueError("sample_costs: no disc samples are held (params['obstacle_track_samples'])")
        S = samples.sent[0]
        lead = () if self.num_instances == 1 else (self.num_instances,)
        out = np.empty(lead + (self.num_control_rollouts, S), dtype=np.float32)
        _lib.call("mppi_planner_get_sample_costs", self._handle, _lib.ptr(out, C.c_float))
        return out

    def init_device_vars_before_solving(self):
        if self.device_var_initialized:
            return
        t0 = time.time()
        cfg = _lib.PlannerCfg(
            device=getattr(self.cfg, "device", 0), mode=_lib.MODE_BAREBONE,
            num_control_rollouts=int(self.num_control_rollouts), num_steps=int(self.num_steps),
            num_grid_samples=1, num_vis_state_rollouts=int(self.num_vis_state_rollouts),
            rng=_lib.RNG_XOROSHIRO if getattr(self.cfg, "rng", "philox") == "xoroshiro" else _lib.RNG_PHILOX,
            math=_lib.MATH_FAST if getattr(self.cfg, "math", "exact") == "fast" else _lib.MATH_EXACT,
            rank=0, world_size=1, num_instances=self.num_instances, seed=int(self.seed))
        handle = C.c_void_p()
        _lib.call("mppi_planner_create", C.byref(cfg), C.byref(handle))
        self._handle = handle
        if getattr(self.cfg, "crowd", False):
            self.set_crowd(True)
        B, t, v = self.num_instances, self.num_steps, self.num_vis_state_rollouts
        n = B * self.num_control_rollouts
        lead = () if B == 1 else (B,)
        ushape, cshape = lead + (t, 2), lead + (self.num_control_rollouts,)
        self.noise_samples_d = DeviceArray((n, t, 2), np.float32, lambda: self._fetch("mppi_planner_get_noise", (n, t, 2)))
        self.u_cur_d = DeviceArray(ushape, np.float32, lambda: self._fetch("mppi_planner_get_u", ushape))
        self._u_prev_view = DeviceArray(ushape, np.float32, lambda: self._fetch("mppi_planner_get_u_prev", ushape))
        self.u_prev_d = self._u_prev_view
        self.costs_d = DeviceArray(cshape, np.float32, lambda: self._fetch("mppi_planner_get_costs", cshape))
        self.weights_d = DeviceArray(cshape, np.float32, lambda: self._fetch("mppi_planner_get_weights", cshape))
        self._last_state_rollout = np.zeros((v, t + 1, 3), dtype=np.float32)
        self.state_rollout_batch_d = DeviceArray((v, t + 1, 3), np.float32, lambda: self._last_state_rollout.copy())
        self.device_var_initialized = True
        print("MPPI planner has initialized GPU memory after {} s".format(time.time() - t0))

    def _fetch(self, fn, shape):
        out = np.empty(shape, dtype=np.float32)
        _lib.call(fn, self._handle, _lib.ptr(out, C.c_float))
        return out

    def setup(self, params):
        self.set_params(params)

    def set_params(self, params):
        self.params = copy.deepcopy(params)
        self.params_set = True

    def check_solve_conditions(self):
        if not self.params_set:
            print("MPPI parameters are not set. Cannot solve")
            return False
        if not self.device_var_initialized:
            print("Device variables not initialized. Cannot solve.")
            return False
        return True

    def move_mppi_task_vars_to_device(self):
        """Pack the task description as notebook cell 3 casts it (np.float32 everywhere except dist_weight) and hand it to
        the library.  (Assigning a Python / numpy scalar to a c_float field rounds float64 -> float32 to nearest, which is
        what the np.float32(...) casts do: no numpy temporaries on the control path -- the notebook times solve() as a
        whole, `bench.py --workload bb` likewise.)  Around it, one walk over _KINDS; the path with no optional key in params
        and nothing optional held pays one test of the params' keys for all of them, and the discs' hand-over."""
        p = self.params
        c = _lib.Params()
        walk_all = self._walk_all or not _OPTIONAL_KEYS.isdisjoint(p)
        moving_goal = walk_all and "goal_track" in p
        if walk_all:
            if "drive" in p:  # (a string that names no drive: refused ahead of every call)
                _read_drive(self, p)
            self._walk_all = True  # (until the walk has come to its end)
            self._sync_kind(p, _GOAL)
            if "guide" in p:  # (its refusals -- no 'xgoal' among them -- ahead of the params struct, which reads 'xgoal')
                _read_guide(self, p)
        for name, count in _TASK_VECTORS_GOAL_TRACK if moving_goal else _TASK_VECTORS:
            src, dst = p[name], getattr(c, name)
            for i in range(count):
                dst[i] = float(src[i])
        if moving_goal:  # (the static goal rests: the field holds the track's first row)
            c.xgoal[0], c.xgoal[1] = float(p['goal_track'][0][0]), float(p['goal_track'][0][1])
        c.dt = float(p['dt'])
        c.goal_tolerance = float(p['goal_tolerance'])
        c.v_post_rollout = 0.0
        c.lambda_weight = float(p['lambda_weight'])
        c.cvar_alpha = 1.0
        if 'cvar_alpha' in p:  # (read by the sample forms alone: without disc samples every launch keeps its bits)
            c.cvar_alpha = float(p['cvar_alpha'])
            if not 0.0 < c.cvar_alpha <= 1.0:
                raise ValueError("params['cvar_alpha'] = {}: must lie in (0, 1]".format(p['cvar_alpha']))
        c.obs_cost = float(DEFAULT_OBS_COST if 'obs_penalty' not in p else p['obs_penalty'])
        c.unknown_cost = 0.0
        c.res, c.xlo, c.ylo = 1.0, 0.0, 0.0
        c.dist_weight = float(DEFAULT_DIST_WEIGHT if 'dist_weight' not in p else p['dist_weight'])
        c.alpha_dyn = 1.0
        c.num_opt = int(p['num_opt'])
        _lib.call("mppi_planner_set_params", self._handle, C.byref(c))
        if walk_all:
            self._sync(p, _KINDS[1:])
            self._walk_all = any(self._held[name].key is not None for name in _OPTIONAL_NAMES)
        else:
            self._sync_kind(p, _DISCS)

    def solve(self):
        if not self.check_solve_conditions():
            print("MPPI solve condition not met. Cannot solve. Return")
            return
        return self.solve_with_nominal_dynamics()

    def solve_with_nominal_dynamics(self):
        self.move_mppi_task_vars_to_device()
        useq = np.empty(((self.num_instances,) if self.num_instances > 1 else ()) + (self.num_steps, 2), dtype=np.float32)
        _lib.call("mppi_planner_solve", self._handle, None, None, _lib.ptr(useq, C.c_float))
        self.u_prev_d = self._u_prev_view
        return useq

    def shift_and_update(self, new_x0, u_cur, num_shifts=1):
        self.params["x0"] = new_x0.copy()
        self.shift_optimal_control_sequence(u_cur, num_shifts)
        self._anchor_after_shift(u_cur, num_shifts)
        self._advance_tracks(num_shifts)

    def _advance_tracks(self, num_shifts):
        # disc tracks, wall tracks or a goal track: num_shifts control steps later "now" is that many rows further
        if self._tracks_on() or self._wall_tracks_on() or self._goal_track_on():
            self.set_track_offset(self._track_offset.astype(np.int64) + int(num_shifts))

    def shift_optimal_control_sequence(self, u_cur, num_shifts=1):
        shifted = u_cur.copy()
        shifted[:-num_shifts] = shifted[num_shifts:]
        shifted = np.ascontiguousarray(shifted.astype(np.float32))
        _lib.call("mppi_planner_set_u", self._handle, _lib.ptr(shifted, C.c_float))

    def get_state_rollout(self):
        assert self.params_set, "MPPI parameters are not set"
        if not self.device_var_initialized:
            print("Device variables not initialized. Cannot run mppi.")
            return
        self.move_mppi_task_vars_to_device()
        out = np.empty((self.num_vis_state_rollouts, self.num_steps + 1, 3), dtype=np.float32)
        _lib.call("mppi_planner_get_state_rollout", self._handle, None, None, _lib.ptr(out, C.c_float))
        self._last_state_rollout = out
        return out.copy()

    def closed_loop(self, max_steps, goal_tolerance=None, x_init=None):
        """The notebook's control loop (barebone_mppi_numba.ipynb cell 7) on the device: max_steps times {solve, float64
        Euler step of the nominal unicycle with useq[0], shift_and_update, goal check}, without a host round trip per
        control step.  Returns (xhist (max_steps+1, 3) float64, uhist (max_steps, 2) float32, steps_taken) -- with a
        leading problem axis for a batch; rows never reached are NaN, as in the notebook.  Afterwards params['x0'] and
        the device's control sequence are where the loop left them (see mppi.MPPI_Numba.closed_loop)."""
        if not self.check_solve_conditions():
            print("MPPI solve condition not met. Cannot solve. Return")
            return
        B, single = self.num_instances, self.num_instances == 1
        self.move_mppi_task_vars_to_device()
        if single:
            x0 = np.asarray(self.params["x0"], dtype=np.float64).reshape(1, 3) if x_init is None \
                else np.asarray(x_init, dtype=np.float64).reshape(1, 3)
            x0_f32 = np.ascontiguousarray(x0.astype(np.float32))
            goal = np.ascontiguousarray(np.asarray(self.goal_now, dtype=np.float64).astype(np.float32)).reshape(1, 2)
            _lib.call("mppi_planner_set_instances", self._handle, 1, _lib.ptr(x0_f32, C.c_float),
                      _lib.ptr(goal, C.c_float))
            x_init = x0
        tol = float(self.params["goal_tolerance"] if goal_tolerance is None else goal_tolerance)
        xhist = np.empty((B, max_steps + 1, 3), dtype=np.float64)
        uhist = np.empty((B, max_steps, 2), dtype=np.float32)
        steps = np.zeros(B, dtype=np.int32)
        xi = None
        if x_init is not None:
            xi = np.ascontiguousarray(np.asarray(x_init, dtype=np.float64).reshape(B, 3))
        try:
            _lib.call("mppi_planner_closed_loop", self._handle, None, None, None, int(max_steps), float(self.cfg.dt), tol,
                      None if xi is None else _lib.ptr(xi, C.c_double), _lib.ptr(xhist, C.c_double),
                      _lib.ptr(uhist, C.c_float), _lib.ptr(steps, C.c_int))
        finally:
            if single:
                _lib.call("mppi_planner_set_instances", self._handle, 0, None, None)
        self.u_prev_d = self._u_prev_view
        self._fetch_track_offset()  # (advanced on the device, one row per control step of a problem still running)
        last = np.stack([xhist[b, steps[b]] for b in range(B)])
        if single:
            self.params["x0"] = last[0].copy()
            return xhist[0], uhist[0], int(steps[0])
        self.x0s = np.ascontiguousarray(last.astype(np.float32))
        self.params["x0"] = last[0].copy()
        return xhist, uhist, steps

    def set_graph_replay(self, enabled=True, iterations_per_graph=2):
        """hipGraph replay of the iteration loop (include/mppi_hip.h); same results."""
        _lib.call("mppi_planner_set_graph_replay", self._handle, int(iterations_per_graph) if enabled else 0)

    def graph_stats(self):
        captures, replays = C.c_long(0), C.c_long(0)
        _lib.call("mppi_planner_graph_stats", self._handle, C.byref(captures), C.byref(replays))
        return dict(captures=int(captures.value), replays=int(replays.value))

    # --- stage-level hooks for parity tests (not in the notebook) ---
    def set_u(self, u):
        u = np.ascontiguousarray(u, dtype=np.float32).reshape(self.num_instances * self.num_steps, 2)
        _lib.call("mppi_planner_set_u", self._handle, _lib.ptr(u, C.c_float))

    def set_noise(self, noise):
        noise = np.ascontiguousarray(noise, dtype=np.float32).reshape(
            self.num_instances * self.num_control_rollouts, self.num_steps, 2)
        _lib.call("mppi_planner_set_noise", self._handle, _lib.ptr(noise, C.c_float))

    def sample_noise(self):
        self.move_mppi_task_vars_to_device()
        _lib.call("mppi_planner_sample_noise", self._handle)

    def rollout(self):
        self.move_mppi_task_vars_to_device()
        _lib.call("mppi_planner_rollout", self._handle, None, None)

    def set_costs(self, costs):
        costs = np.ascontiguousarray(costs, dtype=np.float32).reshape(self.num_instances * self.num_control_rollouts)
        _lib.call("mppi_planner_set_costs", self._handle, _lib.ptr(costs, C.c_float))

    def update(self):
        self.move_mppi_task_vars_to_device()
        _lib.call("mppi_planner_update", self._handle)
        self.u_prev_d = self._u_prev_view

    def last_rollout_kernel(self):
        """Which kernel variant the last rollout launch used (diagnostic string)."""
        buf = C.create_string_buffer(512)
        _lib.call("mppi_planner_describe_last_rollout", self._handle, buf, 512)
        return buf.value.decode()

    def set_debug_flags(self, flags):
        """Developer switches (_lib.DEBUG_*): which rollout kernel variant runs; never the costs."""
        _lib.call("mppi_planner_set_debug_flags", self._handle, int(flags))


class MPPI_Batch(MPPI_Numba):

    """B independent barebone problems in one handle (not in the reference; see batch.MPPI_Batch for the map modes).
    One problem of the notebook's shape (N = 1000, T = 50) keeps 16 waves busy; a batch fills the device with one launch
    over (problem, rollout).  Each problem has its own start, goal, control sequence and, optionally, its own disc set
    (e.g. the other robots' predicted positions); its result is bit-identical to a single-problem MPPI_Numba given the
    same discs, controls and noise.

        batch = MPPI_Batch(cfg, num_instances=64)          # cfg.num_control_rollouts: a multiple of 64
        batch.setup(params, x0s, goals, obstacle_sets)     # params as for MPPI_Numba
        useqs = batch.solve()                              # (B, T, 2) float32
        batch.shift_and_update(new_x0s, useqs, num_shifts=1)

    Everything in `params` except 'x0', 'xgoal' (and the discs, when obstacle_sets is given) is shared.  A goal that moves:
    params['goal_track'] is one track for every problem, set_goal_tracks() one per problem."""

    def __init__(self, cfg, num_instances):
        num_instances = int(num_instances)
        assert num_instances >= 1, "num_instances must be >= 1"
        self.num_instances = num_instances
        self.x0s = None
        self.goals = None
        self.obstacle_sets = None
        self.wall_sets = None
        self.goal_tracks = None
        super().__init__(cfg)

    def reset(self):
        super().reset()
        self.u_seq0 = np.zeros((self.num_instances, self.num_steps, 2), dtype=np.float32)

    # ------------------------------------------------------------------ task set-up
    def setup(self, params, x0s=None, goals=None, obstacle_sets=None, wall_sets=None, goal_tracks=None):
        if x0s is None:
            x0s = np.tile(np.asarray(params["x0"], dtype=np.float32), (self.num_instances, 1))
        if goals is None:  # (with a shared goal track and no goals: the static goals, which rest, are its first row)
            first = params["goal_track"][0] if "goal_track" in params else params["xgoal"]
            goals = np.tile(np.asarray(first, dtype=np.float32), (self.num_instances, 1))
        params = dict(params)
        params["x0"] = np.asarray(x0s[0]).copy()
        if "goal_track" not in params:
            params["xgoal"] = np.asarray(goals[0]).copy()
        self.set_params(params)
        self.set_instances(x0s, goals)
        self.set_obstacle_sets(obstacle_sets)
        self.set_wall_sets(wall_sets)
        self.set_goal_tracks(goal_tracks)

    def set_instances(self, x0s, goals=None):
        """(B,3) start states and (B,2) goals (goals=None keeps the current ones)."""
        x0s = np.ascontiguousarray(np.asarray(x0s, dtype=np.float64).astype(np.float32)).reshape(self.num_instances, 3)
        if goals is None:
            goals = self.goals
        goals = np.ascontiguousarray(np.asarray(goals, dtype=np.float64).astype(np.float32)).reshape(self.num_instances, 2)
        self.x0s, self.goals = x0s, goals
        _lib.call("mppi_planner_set_instances", self._handle, self.num_instances,
                  _lib.ptr(x0s, C.c_float), _lib.ptr(goals, C.c_float))

    def set_obstacle_sets(self, obstacle_sets):
        """One disc set per problem: a list of B (positions (K_b, 2), radii (K_b,)) pairs, K_b >= 0 -- or None: every
        problem has the shared set of params['obstacle_positions'] / ['obstacle_radius'].  A set whose first element
        is 3-D, (K_b, L, 2), is a set of tracks (discs that move; L common to the sets of a call); one call is all
        static or all tracks."""
        problem_discs = self._held["problem_discs"]
        if obstacle_sets is None or not _is_track_set(obstacle_sets[0]):
            self._own_slot(_TRACKS, None)
        if obstacle_sets is None:
            _lib.call("mppi_planner_set_instance_disc_obstacles", self._handle, 0, None, None, None)
            self.obstacle_sets = problem_discs.sent = None
            return
        if self._held["samples"].key is not None or (self.params is not None and "obstacle_track_samples" in self.params):
            raise ValueError("set_obstacle_sets while params hold 'obstacle_track_samples': disc samples are shared by every "
                             "problem (drop the key first)")
        assert len(obstacle_sets) == self.num_instances, "one disc set per problem"
        kinds = {_is_track_set(s) for s in obstacle_sets}
        if len(kinds) > 1:
            raise ValueError("obstacle_sets mix static sets and track sets: one call is all static or all tracks")
        if kinds == {True}:
            held = [(_f32(np.asarray(tr)), _f32(np.asarray(r)).reshape(-1)) for tr, r in obstacle_sets]
            if self._own_slot(_TRACKS, held, self.obstacle_sets, lambda: _pack_disc_tracks(obstacle_sets)):
                _lib.call("mppi_planner_set_instance_disc_obstacles", self._handle, 0, None, None, None)
                self.obstacle_sets = problem_discs.sent = held
            return
        pos = [_f32(np.asarray(op)).reshape(-1, 2) for op, _ in obstacle_sets]
        rad = [_f32(np.asarray(orad)).reshape(-1) for _, orad in obstacle_sets]
        for b in range(self.num_instances):
            assert len(pos[b]) == len(rad[b]), "problem {}: positions and radii differ in length".format(b)
        counts = np.ascontiguousarray([len(r) for r in rad], dtype=np.int32)
        pos_all = np.ascontiguousarray(np.concatenate(pos) if counts.sum() else np.zeros((0, 2), np.float32))
        rad_all = np.ascontiguousarray(np.concatenate(rad) if counts.sum() else np.zeros(0, np.float32))
        _lib.call("mppi_planner_set_instance_disc_obstacles", self._handle, self.num_instances,
                  _lib.ptr(counts, C.c_int), _lib.ptr(pos_all, C.c_float), _lib.ptr(rad_all, C.c_float))
        self.obstacle_sets = problem_discs.sent = [(p.copy(), r.copy()) for p, r in zip(pos, rad)]

    def set_wall_sets(self, sets):
        """One wall set per problem (crowd mode): a list of B (segments (W_b, 2, 2), half-width: a scalar or (W_b,)) pairs,
        W_b >= 0 -- or None: every problem has the shared walls of params again.  A set whose first element is 4-D,
        (W_b, Lw, 2, 2), is a set of wall tracks (Lw common to the sets of a call); one call is all static or all tracks.
        Per-problem sets win over the walls of params.  New tracks make row 0 "now"; unchanged ones leave it alone."""
        if sets is None:
            self._own_slot(_WALL_TRACKS, None)
            self.wall_sets = None
            return
        if self._held["fleet"].sent is not None or self._held["fleet_bodies"].sent is not None:
            raise ValueError("set_wall_sets while the fleet is on: the fleet makes every problem's wall set itself "
                             "(set_fleet(None) first)")
        assert len(sets) == self.num_instances, "one wall set per problem"
        kinds = {_is_wall_track_set(s) for s in sets}
        if len(kinds) > 1:
            raise ValueError("wall sets mix static sets and track sets: one call is all static or all tracks")
        held = [(_f32(np.asarray(seg)), _f32(np.asarray(hw))) for seg, hw in sets]
        if self._own_slot(_WALL_TRACKS, held, self.wall_sets, lambda: _pack_wall_tracks(sets)):
            self.wall_sets = held

    def set_goal_tracks(self, tracks):
        """One goal track per problem: (B, L, 2), or a list of B arrays (L, 2) with a common L -- or None: every problem
        has its goal of `goals` again (or the shared track of params['goal_track']).  Per-problem tracks win over
        params['goal_track'].  New tracks of more than one row make row 0 "now"; unchanged ones leave it alone."""
        if tracks is None:
            self._own_slot(_GOAL, None)
            self.goal_tracks = None
            return
        if len(tracks) != self.num_instances:
            raise ValueError("{} goal tracks for {} problems: one per problem".format(len(tracks), self.num_instances))
        held = [_f32(np.asarray(tr)) for tr in tracks]
        if self._own_slot(_GOAL, held, self.goal_tracks, lambda: _pack_goal_tracks(self, tracks)):
            self.goal_tracks = held

    # ------------------------------------------------------------------ a fleet
    def set_fleet(self, radii, margin=0.0):
        """Fleet mode (crowd mode, B >= 2): the problems are robots of body radius `radii` -- a scalar or (B,) -- that avoid
        each other's current plans, kept `margin` apart; None turns it off.  From now on every solve(), rollout() and
        control step of closed_loop() starts by rebuilding, on the device, every robot's walls from the others' plans (the
        module header says which).  The half-width of reader a against b is float32(r_a + r_b + margin), summed in float64
        from the float32 radii.  Raises while per-problem wall sets or params['wall_tracks'] are held."""
        if radii is None:  # (either kind of fleet)
            _lib.call("mppi_planner_set_fleet", self._handle, 0, None)
            self._held["fleet"].sent = self._held["fleet_bodies"].sent = None
            return
        if self._held["fleet_bodies"].sent is not None:
            raise ValueError("set_fleet while the fleet of bodies is on: the two kinds change through off (set_fleet(None) first)")
        B = self.num_instances
        r = np.ascontiguousarray(np.broadcast_to(_f32(radii), (B,)))
        if not (np.isfinite(r).all() and (r >= 0).all() and np.isfinite(margin)):
            raise ValueError("fleet radii are finite and >= 0, the margin finite")
        if self.params is not None and "footprint" in self.params:
            raise ValueError("set_fleet while params hold 'footprint': the fleet's half-widths already contain the reader's "
                             "body (drop the key first)")
        if self._held["footprint"].key is not None:  # (the key has gone and the library has not heard yet)
            self._sync_kind(self.params if self.params is not None else {}, _FOOTPRINT)
        if self._held["wall_tracks"].owner is not _NOBODY:
            raise ValueError("set_fleet while per-problem wall sets or params['wall_tracks'] are held: the fleet makes every "
                             "problem's wall set itself (set_wall_sets(None) / drop the key first)")
        r64 = r.astype(np.float64)
        full = ((r64[:, None] + r64[None, :]) + np.float64(margin)).astype(np.float32)
        half = np.ascontiguousarray(full[np.arange(B)[:, None], fleet_others(B)], dtype=np.float32).reshape(B, max(B - 1, 0))
        _lib.call("mppi_planner_set_fleet", self._handle, B, _lib.ptr(half if half.size else np.zeros(1, np.float32), C.c_float))
        self._held["fleet"].sent = (r.copy(), float(margin), half)

    @property
    def fleet(self):
        """None while fleet mode is off, else (radii (B,) float32, margin)."""
        fleet = self._held["fleet"].sent
        return None if fleet is None else (fleet[0].copy(), fleet[1])

    def set_fleet_bodies(self, footprint, margin=0.0):
        """A fleet of bodies (crowd mode, B >= 2): the fleet of set_fleet() for robots that are the discs of `footprint`
        (F, 3), 1 <= F <= 8, rows (ox, oy, rho) as for params['footprint'] -- one body for every robot --, kept `margin`
        apart; None turns it off.  The module header says what the refresh builds and how hits are counted.  It carries
        its own body: raises while params hold 'footprint', while the disc fleet is on, and while per-problem wall sets
        or params['wall_tracks'] are held."""
        if footprint is None:
            self.set_fleet(None)
            return
        rows = _footprint_rows(footprint)
        margin = float(margin)
        if not (np.isfinite(rows).all() and (rows[:, 2] >= 0).all() and np.isfinite(margin)
                and (rows[:, 2].astype(np.float64) + margin >= 0).all()):
            raise ValueError("a fleet's body has finite rows with rho >= 0, and a finite margin with rho + margin >= 0")
        if self._held["fleet"].sent is not None:
            raise ValueError("set_fleet_bodies while the disc fleet is on: the two kinds change through off (set_fleet(None) first)")
        if self.params is not None and "footprint" in self.params:
            raise ValueError("set_fleet_bodies while params hold 'footprint': the fleet of bodies carries its own body "
                             "(drop the key first)")
        if self._held["footprint"].key is not None:  # (the key has gone and the library has not heard yet)
            self._sync_kind(self.params if self.params is not None else {}, _FOOTPRINT)
        if self._held["wall_tracks"].owner is not _NOBODY:
            raise ValueError("set_fleet_bodies while per-problem wall sets or params['wall_tracks'] are held: the fleet makes "
                             "every problem's wall set itself (set_wall_sets(None) / drop the key first)")
        _lib.call("mppi_planner_set_fleet_bodies", self._handle, self.num_instances, _lib.ptr(rows, C.c_float), len(rows),
                  C.c_double(margin))
        self._held["fleet_bodies"].sent = (rows.copy(), margin)

    @property
    def fleet_bodies(self):
        """None while no fleet of bodies is on, else (rows (F, 3) float32, margin)."""
        bodies = self._held["fleet_bodies"].sent
        return None if bodies is None else (bodies[0].copy(), bodies[1])

    def fleet_body_walls(self):
        """What the last refresh of a fleet of bodies left: (segments (B, B - 1, F, T, 2, 2) float32, half-widths (F,)
        float32, others (B, B - 1) int) -- segments[a, o, k, j] is the segment body disc k of robot others[a, o] covers
        in control interval j from "now", halfwidths[k] = float32(rho_k + margin) the half-width every reader is given it
        with.  The padding slots are left out."""
        if self._held["fleet_bodies"].sent is None:
            raise ValueError("fleet_body_walls: no fleet of bodies is on (set_fleet_bodies)")
        B, t = self.num_instances, self.num_steps
        rows, margin = self._held["fleet_bodies"].sent
        seg = np.empty((B, B - 1, len(rows), t, 2, 2), dtype=np.float32)
        _lib.call("mppi_planner_get_fleet_body_walls", self._handle, _lib.ptr(seg, C.c_float))
        return seg, (rows[:, 2].astype(np.float64) + np.float64(margin)).astype(np.float32), fleet_others(B)

    def refresh_fleet(self):
        """The refresh alone, as solve() makes it at its head: every robot's walls from the others' current controls and
        start states.  For drawing and for tests; fleet_walls() / fleet_body_walls() fetch the result."""
        self.move_mppi_task_vars_to_device()
        _lib.call("mppi_planner_fleet_refresh", self._handle)

    def fleet_walls(self):
        """What the last refresh left: (segments (B, B - 1, T, 2, 2) float32, half-widths (B, B - 1) float32, others
        (B, B - 1) int) -- segments[a, k, j] is the segment robot others[a, k] covers in control interval j from "now",
        as reader a is given it."""
        if self._held["fleet_bodies"].sent is not None:
            raise ValueError("fleet_walls: a fleet of bodies is on, whose walls have one more axis (fleet_body_walls)")
        if self._held["fleet"].sent is None:
            raise ValueError("fleet_walls: the fleet is off (set_fleet)")
        B, t = self.num_instances, self.num_steps
        seg = np.empty((B, B - 1, t, 2, 2), dtype=np.float32)
        _lib.call("mppi_planner_get_fleet_walls", self._handle, _lib.ptr(seg, C.c_float))
        return seg, self._held["fleet"].sent[2].copy(), fleet_others(B)

    def check_solve_conditions(self):
        if self.x0s is None:
            print("Batch instances are not set. Cannot solve")
            return False
        return super().check_solve_conditions()

    # ------------------------------------------------------------------ control loop
    def shift_and_update(self, new_x0s, u_cur, num_shifts=1):
        """Per problem: x0 <- new_x0s[b]; u[b, :-k] = u[b, k:] (tail kept), uploaded."""
        self.set_instances(new_x0s)
        self.params["x0"] = np.asarray(new_x0s[0]).copy()
        self.shift_optimal_control_sequence(u_cur, num_shifts)
        self._anchor_after_shift(u_cur, num_shifts)
        self._advance_tracks(num_shifts)

    def shift_and_update_on_device(self, new_x0s, num_shifts=1):
        self.set_instances(new_x0s)
        self.params["x0"] = np.asarray(new_x0s[0]).copy()
        if "accel_limits" in self.params:  # (the control applied last, fetched ahead of the shift)
            self._anchor_after_shift(self.u_cur_d.copy_to_host(), num_shifts)
        _lib.call("mppi_planner_shift_u", self._handle, int(num_shifts))
        self._advance_tracks(num_shifts)

    def shift_optimal_control_sequence(self, u_cur, num_shifts=1):
        shifted = np.array(u_cur, dtype=np.float32).reshape(self.num_instances, self.num_steps, 2)
        shifted[:, :-num_shifts] = shifted[:, num_shifts:].copy()
        self.set_u(shifted)

    def get_state_rollout(self, instance=0):
        """(V, T+1, 3) state sequences of one problem (see MPPI_Numba.get_state_rollout)."""
        assert self.params_set, "MPPI parameters are not set"
        self.move_mppi_task_vars_to_device()
        out = np.empty((self.num_vis_state_rollouts, self.num_steps + 1, 3), dtype=np.float32)
        _lib.call("mppi_planner_get_instance_state_rollout", self._handle, None, None, int(instance),
                  _lib.ptr(out, C.c_float))
        self._last_state_rollout = out
        return out.copy()
