"""The scenes of the occupancy-grid comparisons, shared by tests/test_occupancy_cases.py (CPU: on the model, every scene has
hits and misses, a step near at a ring without a hit, a test point outside the grid and a rollout that reaches the goal --
so no GPU comparison passes vacuously) and tests/test_gpu_barebone_occupancy.py (GPU: the device gives the model's bits).
Nothing here is changed after it is made.

The shapes: N = 70 (a ragged second tile) and 128, T = 37 (a second, partial chunk), K in {0, 70} discs, W in {0, 65} walls.
The two fleets are those of tests/clearance_cases.py (B = 3, n = 64, T = 37), whose walls and models are shared."""
import functools

import numpy as np

import clearance_cases
import occupancy_model as om
from clearance_cases import FOOTPRINTS as _FP, NO_DISCS, RINGS
from crowd_model import crowd_discs
from test_footprint_model import EIGHT
from test_gpu_barebone_batch import make_params, oracle_params, problem_params, problems
from test_gpu_barebone_crowd import inputs
from test_gpu_barebone_walls import GOAL
from wall_model import states

T = 37
FOOTPRINTS = {1: _FP[1], 3: _FP[3], 8: EIGHT}
RES = np.float32(0.1)


def occupancy_params(params, grid):
    p = dict(params)
    p["occupancy"] = dict(origin=(float(grid.x_min), float(grid.y_min)), resolution=float(grid.res), cells=grid.cells.astype(np.uint8),
                          inflate=float(grid.inflate), substeps=grid.substeps)
    return p


def without_occupancy(params):
    return {k: v for k, v in params.items() if k != "occupancy"}


@functools.lru_cache(maxsize=None)
def task(n, wscale):
    """(params, u_in, noise) of n rollouts over T steps: the task of tests/test_gpu_barebone_walls.py at another N."""
    rng = np.random.default_rng(1000 * n + int(10 * wscale))
    params = make_params(0.1, wscale)
    params["xgoal"] = GOAL.copy()
    params["vrange"] = np.array([0.0, 1.8])  # steps of up to 0.18 m
    u_in, noise = inputs(rng, n, T)
    u_in.setflags(write=False)
    noise.setflags(write=False)
    return params, u_in, noise


def scatter(seed, shape, fill, bar=True):
    """Cells: a random scatter of density `fill` and, with `bar`, a bar of occupied cells across the grid's middle."""
    rng = np.random.default_rng(seed)
    cells = rng.uniform(size=shape) < fill
    if bar:
        cells[shape[0] // 2, shape[1] // 4: 3 * shape[1] // 4] = True
    return cells


def grid_over(st, seed, inflate, substeps, fill=0.03, cut=0.25, res=RES, bar=True):
    """A grid of `res` cells over the states' bounding box less `cut` of it at the low end of either axis and a twentieth
    at the high end -- so that steps lie outside it on every side that has any."""
    xy = np.asarray(st, np.float32)[..., :2].reshape(-1, 2).astype(np.float64)
    lo, hi = xy.min(axis=0), xy.max(axis=0)
    lo = lo + cut * (hi - lo)
    hi = hi - 0.05 * (hi - lo)
    shape = (max(1, int(np.ceil((hi[1] - lo[1]) / float(res)))), max(1, int(np.ceil((hi[0] - lo[0]) / float(res)))))
    return om.Grid(lo, res, scatter(seed, shape, fill, bar), inflate, substeps)


# (name, n, wscale, F, R, substeps, K, disc kind, offset, walls: 0, 65 static or "tracks", goal track)
SINGLE = (
    ("point", 70, 1.0, 0, 0, 1, 0, "static", 0, 0, False),
    ("point-discs-walls-M3", 128, 1.5, 0, 0, 3, 70, "static", 0, 65, False),
    ("point-R2-tracks+5", 70, 1.5, 0, 2, 1, 70, "tracks", 5, 0, False),
    ("point-R4-walls-M3", 128, 1.0, 0, 4, 3, 0, "static", 0, 65, False),
    ("F1-M3-discs", 70, 1.0, 1, 0, 3, 70, "static", 0, 0, False),
    ("F3-R2-tracks-walls", 128, 1.5, 3, 2, 1, 70, "tracks", 0, 65, False),
    ("F8-R4-M3", 70, 1.5, 8, 4, 3, 0, "static", 0, 0, False),
    ("F8-discs-walls", 128, 1.0, 8, 0, 1, 70, "static", 0, 65, False),
    ("F3-R2-M3-wall-tracks+5", 70, 1.0, 3, 2, 3, 70, "tracks", 5, "tracks", False),
    ("point-R2-M3-goal-track", 128, 1.0, 0, 2, 3, 0, "static", 0, 0, True),
    ("F3-M1-goal-track-walls", 70, 1.5, 3, 0, 1, 70, "static", 0, 65, True),
)
NAMES = tuple(row[0] for row in SINGLE)


@functools.lru_cache(maxsize=None)
def single_case(name):
    """Everything a comparison needs: the planner's params (without the key), the oracle's, the model's view of discs and
    walls, the grid, rings, footprint, offset, goal track, inputs and the model's states."""
    _, n, wscale, F, R, M, K, kind, offset, walls, goal = SINGLE[NAMES.index(name)]
    params, u_in, noise = task(n, wscale)
    W = walls if isinstance(walls, int) else 0
    full, tracks, rad, seg, hw = clearance_cases.scene(K, W, kind, T, wscale)
    if not K:
        tracks, rad = NO_DISCS
    track = None
    if walls == "tracks":
        _, _, wtracks, whw, _ = clearance_cases.wall_track_case(T)
        from test_gpu_barebone_wall_tracks import track_wall_params
        full, seg, hw = track_wall_params(full, wtracks, whw), wtracks, whw
    base = dict(params)
    if goal:
        from test_gpu_barebone_goal_tracks import goal_params
        track = clearance_cases.wall_track_case(T)[4]
        full = goal_params(full, track)
        base["xgoal"] = track[0]
    p = oracle_params(base)
    st = states(p, noise, u_in)
    st.setflags(write=False)
    grid = grid_over(st, 17 + NAMES.index(name), inflate=0.08 if F else 0.25, substeps=M)  # (a point robot: its radius)
    rings = RINGS[R] if R else None
    if rings is not None:
        full = clearance_cases.ring_params(full, rings)
    fp = FOOTPRINTS[F] if F else None
    if fp is not None:
        full = dict(full, footprint=fp)
    return dict(name=name, n=n, wscale=wscale, F=F, R=R, M=M, K=K, W=(len(hw) if seg is not None else 0), kind=kind, offset=offset,
                walls=walls, params=full, p=p, tracks=tracks, rad=rad, seg=seg, hw=hw, grid=grid, rings=rings, footprint=fp,
                goal_track=track, u_in=u_in, noise=noise, st=st)


def model_costs(case, grid=None):
    c = case
    return om.costs(c["p"], c["grid"] if grid is None else grid, c["rings"], c["tracks"], c["rad"], c["seg"], c["hw"], c["noise"], c["u_in"],
                    footprint=c["footprint"], offset=c["offset"], goal_track=c["goal_track"])


def the_input_means_something(grid, st, rings, footprint, p, goal_rows=None, alone=True):
    """The four conditions on a scene, on the model.  alone False -- one problem of several: whether a rollout reaches the
    goal is returned, for the scene to judge."""
    margins = [0.0] + ([] if rings is None else [float(m) for m in np.asarray(rings, np.float32)[:, 0].astype(np.float64)])
    if rings is None:
        margins.append(float(np.float32(0.3)))  # (a scene without rings: a ring it might have had)
    bits, inside = om.level_bits(grid, st, margins, footprint)
    share = bits[0].mean()
    assert 0.05 <= share <= 0.95, "bad input: %.3f of the (rollout, step) pairs hit" % share
    assert (bits[1:].any(axis=0) & ~bits[0]).any(), "bad input: no pair is near at a ring without hitting"
    assert (~inside).any() and inside.any(), "bad input: no test point lies outside the grid (or none inside)"
    goals = np.broadcast_to(np.float32([p.xgoal[0], p.xgoal[1]]), (st.shape[1] - 1, 2)) if goal_rows is None else np.asarray(goal_rows, np.float32)
    d = (goals[None, :, :].astype(np.float64) - st[:, 1:, :2].astype(np.float64))
    reached = bool(((d * d).sum(axis=-1) <= float(np.float32(p.goal_tolerance)) ** 2).any())
    assert reached or not alone, "bad input: no rollout reaches the goal"
    return share if alone else reached


# ---- a batch: B = 3 problems of n = 128 with their own disc sets and wall sets, one grid ---------------------------------------
@functools.lru_cache(maxsize=None)
def batch_case():
    counts, wcounts = [0, 12, 70], [65, 0, 5]
    B, n = 3, 128  # (a batch wants whole tiles)
    rng = np.random.default_rng(41)
    x0s, goals = problems(rng, B)
    sets = [crowd_discs(rng, k, x0s[b], goals[b]) for b, k in enumerate(counts)]
    wall_sets = []
    for b, w in enumerate(wcounts):
        a = x0s[b, :2] + rng.uniform(-1.0, 4.0, (w, 2))
        wall_sets.append((np.stack([a, a + rng.uniform(-1.5, 1.5, (w, 2))], axis=1).astype(np.float32).reshape(w, 2, 2),
                          rng.uniform(0.0, 0.2, w).astype(np.float32)))
    u_in = np.stack([inputs(rng, n, T)[0] for _ in range(B)])
    noise = rng.normal(0, 0.5, (B, n, T, 2)).astype(np.float32)
    params = make_params(0.1, 1.0)
    sts = [states(oracle_params(problem_params(params, x0s[b], goals[b])), noise[b], u_in[b]) for b in range(B)]
    goals = goals_on_the_way(sts)
    grid = grid_over(np.concatenate(sts), 5, inflate=0.3, substeps=3, fill=0.02, cut=0.15, res=np.float32(0.15))  # (coarser cells: the problems lie metres apart)
    return dict(B=B, n=n, t=T, params=params, x0s=x0s, goals=goals, sets=sets, wall_sets=wall_sets, u_in=u_in, noise=noise,
                counts=counts, wcounts=wcounts, rings=RINGS[2], grid=grid, sts=sts)


def goals_on_the_way(sts):
    """Goals that some rollout reaches: where every problem's rollout 0 is after 25 steps.  (The states do not depend on
    the goal.)"""
    return np.stack([st[0, 25, :2] for st in sts]).astype(np.float32)


# ---- the fleets of tests/clearance_cases.py, with goals that are reached: the walls come from the plans, not from the goals ----
def fleet_scene(case, seed, substeps, inflate, fill, bar=True):
    """(grid, goals (B, 2), the readers' oracle parameters, their states)."""
    B = case["B"]
    sts = [states(case["readers"][b][0], case["noise"][b], case["us"][b]) for b in range(B)]
    goals = goals_on_the_way(sts)
    ps = [oracle_params(problem_params(case["params"], case["x0s"][b], goals[b])) for b in range(B)]
    return grid_over(np.concatenate(sts), seed, inflate, substeps, fill, cut=0.2, bar=bar), goals, ps, sts


@functools.lru_cache(maxsize=None)
def disc_fleet_scene():
    return fleet_scene(clearance_cases.disc_fleet_case(), 23, 3, inflate=0.2, fill=0.03)


@functools.lru_cache(maxsize=None)
def body_fleet_scene():
    return fleet_scene(clearance_cases.body_fleet_case(), 29, 1, inflate=0.0, fill=0.01, bar=False)
