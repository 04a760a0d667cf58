"""The inputs of the clearance-ring comparisons, shared by tests/test_clearance_model.py (CPU: no disc verdict of these
inputs is near enough to its boundary for the kernel's fma to flip it, and the inputs mean something) and
tests/test_gpu_barebone_rings.py (GPU: the device gives the model's bits).  Nothing here is changed after it is made."""
import functools

import numpy as np

import fleet_body_cases
import fleet_body_model
import fleet_model
from crowd_model import crowd_discs
from test_footprint_model import EIGHT
from test_gpu_barebone_batch import make_params, oracle_params, problem_params, problems
from test_gpu_barebone_crowd import inputs
from test_gpu_barebone_fleet import ROOM, ROOM_HW, ring
from test_gpu_barebone_footprint import scene_params
from test_gpu_barebone_goal_tracks import crossing_goal
from test_gpu_barebone_wall_tracks import moving_building
from test_gpu_barebone_walls import discs_of, task, without_walls
from wall_model import states

TASKS = ((30, 1.0), (37, 1.5))  # more than one chunk, 37 no multiple of the counters; rotation on, off
# rows (margin, penalty): penalties of the size of a step's distance term and of a hit, so that every ring shows in the bits
RINGS = {1: np.float32([[0.15, 2.5e4]]),
         2: np.float32([[0.1, 3e5], [0.3, 4e4]]),
         4: np.float32([[0.05, 7e5], [0.12, 9e4], [0.2, 2.5e4], [0.35, 1100.0]])}
FOOTPRINTS = {1: EIGHT[5:6], 3: EIGHT[[0, 5, 6]]}  # (F = 1: one disc off the axis, so that the heading counts)
NO_DISCS = np.zeros((0, 1, 2), np.float32), np.zeros(0, np.float32)
NO_WALLS = np.zeros((0, 2, 2), np.float32), np.zeros(0, np.float32)


def ring_params(params, rings):
    p = dict(params)
    p["clearance_rings"] = rings
    return p


def without_rings(params):
    return {k: v for k, v in params.items() if k != "clearance_rings"}


@functools.lru_cache(maxsize=None)
def states_of(t, wscale):
    params, u_in, noise = task(t, wscale)
    st = states(oracle_params(without_walls(params)), noise, u_in)
    st.setflags(write=False)
    return st


def scene(K, W, kind, t, wscale):
    """(params with K discs -- static, or tracks of t + 1 rows -- and W static walls, tracks (K, L, 2), radii, seg, hw)."""
    return scene_params(task(t, wscale)[0], K, W, kind, t)


def point_cases():
    """(R, K, W, t, wscale) of the point robot's comparison; each runs static discs, then tracks at offsets 0 and 5."""
    return [(R, K, W, t, wscale) for R in (1, 4) for K in (0, 3, 70) for W in (0, 1, 65) for t, wscale in TASKS]


def body_cases():
    return [(F, t, wscale) for F in (1, 3) for t, wscale in TASKS]


# ---- a batch: B = 3 problems with their own disc sets and wall sets -------------------------------------------------------
@functools.lru_cache(maxsize=None)
def batch_case():
    """Problem 1 has twelve discs and no walls.  The seed is the first of 29 .. 44, found with the model on the CPU, at which
    the rings change the costs of some of its rollouts and not of all (none of them is hit); the other two problems' rollouts
    are all hit (tests/test_gpu_barebone_rings.py asserts that every problem's costs differ from those without rings)."""
    counts, wcounts = [0, 12, 90], [70, 0, 5]
    B, n, t = 3, 64, 30
    rng = np.random.default_rng(37)
    x0s, goals = problems(rng, B)
    sets = [crowd_discs(rng, k, x0s[b], goals[b]) for b, k in enumerate(counts)]
    wall_sets = []
    for b, w in enumerate(wcounts):
        a = x0s[b, :2] + rng.uniform(-1.0, 4.0, (w, 2))
        wall_sets.append((np.stack([a, a + rng.uniform(-1.5, 1.5, (w, 2))], axis=1).astype(np.float32).reshape(w, 2, 2),
                          rng.uniform(0.0, 0.2, w).astype(np.float32)))
    u_in = np.stack([inputs(rng, n, t)[0] for _ in range(B)])
    noise = rng.normal(0, 0.5, (B, n, t, 2)).astype(np.float32)
    return dict(B=B, n=n, t=t, params=make_params(0.1, 1.0), x0s=x0s, goals=goals, sets=sets, wall_sets=wall_sets, u_in=u_in,
                noise=noise, counts=counts, wcounts=wcounts, rings=RINGS[2])


def batch_problem(case, b):
    """(the single planner's params, its oracle parameters, tracks, radii, seg or None, hw) of problem b."""
    pb = problem_params(case["params"], case["x0s"][b], case["goals"][b], case["sets"][b])
    seg, hw = case["wall_sets"][b]
    return pb, oracle_params(pb), case["sets"][b][0][:, None, :], case["sets"][b][1], (seg if len(hw) else None), hw


# ---- the fleets: B = 3, n = 64 -----------------------------------------------------------------------------------------
FLEET_T, FLEET_W = 37, 2
FLEET_RADII, FLEET_MARGIN = (0.2, 0.25, 0.3), 0.02


@functools.lru_cache(maxsize=None)
def disc_fleet_case():
    """The disc fleet of test_gpu_barebone_fleet (three robots on a ring of 1.5 m, two room walls), with two rings."""
    B, n, t, W = 3, 64, FLEET_T, FLEET_W
    x0s, goals, us, noise = ring(B, n, t, 7 * B + t)
    params = make_params(0.1, 1.0)
    hw = fleet_model.halfwidths(np.asarray(FLEET_RADII), FLEET_MARGIN, B)
    walls = fleet_model.fleet_walls(params, x0s, us)
    readers = []
    for b in range(B):
        wt, h = fleet_model.reader_walls(walls[b], hw[b], ROOM[:W], ROOM_HW[:W])
        readers.append((oracle_params(problem_params(params, x0s[b], goals[b])), wt, h))
    return dict(B=B, n=n, t=t, W=W, params=params, x0s=x0s, goals=goals, us=us, noise=noise, readers=readers, rings=RINGS[2])


@functools.lru_cache(maxsize=None)
def body_fleet_case():
    """The (B = 3, F = 3, W = 2) fleet of bodies of fleet_body_cases at T = 37: four slots a robot (the fourth repeats the
    third body disc), eight grouped slots a reader and the two room walls behind them."""
    B, F, W, t = 3, 3, FLEET_W, FLEET_T
    radius, seed = fleet_body_cases.FLEETS[(B, F, W, t)]
    x0s, goals, us, noise = fleet_body_cases.scene(B, t, seed, radius)
    params = make_params(fleet_body_cases.DT, 1.0)
    footprint = fleet_body_cases.body(F)
    walls = fleet_body_model.body_walls(params, x0s, us, footprint)  # (B, B - 1, F, T, 2, 2)
    hw = fleet_body_model.halfwidths(footprint, fleet_body_cases.MARGIN)
    group = fleet_body_model.group_size(F)
    readers = []
    for a in range(B):
        slots, shw = fleet_body_model.padded(walls[a], hw)  # (B - 1, Fp, T, 2, 2), (Fp,)
        seg = np.concatenate([slots.reshape((-1,) + slots.shape[2:]), np.repeat(ROOM[:W, None], t, axis=1)])
        readers.append((fleet_body_cases.reader_params(params, x0s[a], goals[a]), seg, np.concatenate([np.tile(shw, B - 1), ROOM_HW[:W]])))
    return dict(B=B, F=F, W=W, t=t, n=fleet_body_cases.N, params=params, x0s=x0s, goals=goals, us=us, noise=noise, footprint=footprint,
                margin=fleet_body_cases.MARGIN, group=group, grouped=(B - 1) * group, readers=readers, rings=RINGS[2])


# ---- every set of discs a GPU comparison with the model tests against ------------------------------------------------------
def disc_input_sets():
    """(label, states, rings, tracks, radii, footprint or None, offset) of every comparison with the model that has discs."""
    for R, K, W, t, wscale in point_cases():
        if K and W == 0:  # (the walls do not change the disc tests)
            for kind, offsets in (("static", (0,)), ("tracks", (0, 5))):
                _, tracks, rad, _, _ = scene(K, 0, kind, t, wscale)
                for offset in offsets:
                    yield "point R=%d K=%d %s+%d T=%d" % (R, K, kind, offset, t), states_of(t, wscale), RINGS[R], tracks, rad, None, offset
    for F, t, wscale in body_cases():
        for kind, offsets in (("static", (0,)), ("tracks", (0, 5))):
            _, tracks, rad, _, _ = scene(70, 0, kind, t, wscale)
            for offset in offsets:
                yield "body F=%d %s+%d T=%d" % (F, kind, offset, t), states_of(t, wscale), RINGS[2], tracks, rad, FOOTPRINTS[F], offset
    t, wscale = 37, 1.0  # the wall-track case and the goal-track case
    where, rad = wall_track_case(t)[:2]
    for offset in (0, 5):
        yield "wall tracks +%d" % offset, states_of(t, wscale), RINGS[2], where, rad, FOOTPRINTS[3], offset
    _, tracks, rad, _, _ = scene(3, 1, "static", t, wscale)
    yield "goal track", states_of(t, wscale), RINGS[2], tracks, rad, FOOTPRINTS[3], 0
    case = batch_case()
    for b in range(case["B"]):
        _, p, tracks, rad, _, _ = batch_problem(case, b)
        if len(rad):
            yield "batch problem %d" % b, states(p, case["noise"][b], case["u_in"][b]), case["rings"], tracks, rad, None, 0


def wall_track_case(t):
    """70 disc tracks and 65 wall tracks of t + 1 rows, and the goal that crosses the fan of rollouts."""
    params = task(t, 1.0)[0]
    where, rad = discs_of(70, "tracks", t, params)
    wtracks, hw = moving_building(65, t + 1)
    return where, rad, wtracks, hw, crossing_goal(t, t + 1)

