"""The inputs of the sweep over the forms of k_rollout_barebone_crowd, shared by tests/test_form_model.py (CPU: the model is
the feature models' composition, no disc verdict of these inputs is near enough to its boundary for the kernel's fma to flip
it, and the inputs mean something) and tests/test_gpu_barebone_form_models.py (GPU: every form gives the model's bits).
Nothing here is changed after it is made.

The shapes are the smallest at which the count walk can still go wrong: N = 64 rollouts a problem -- one rollout tile, so
that from lane W % 64 on a lane of a partial wall tile holds a rollout and no wall --, T = 18 -- a second, partial chunk --,
and (K, W) = (7, 10), one partial tile of discs and of walls, or (70, 74), a full tile and a partial one of each.  Every
feature counts: disc tracks, wall tracks and a goal track of T + 1 rows, S = 3 distinct samples at cvar_alpha = 0.5 (the tail
sorts, numel = 2), two rings whose penalties show in the bits, a body of three discs off the axis."""
import functools
import itertools

import numpy as np

import form_model
from clearance_cases import FOOTPRINTS, RINGS
from disc_samples_model import cvar_tail
from test_gpu_barebone_batch import oracle_params
from test_gpu_barebone_crowd import inputs
from test_gpu_barebone_disc_samples import sample_set
from test_gpu_barebone_goal_tracks import crossing_goal
from test_gpu_barebone_wall_tracks import moving_building
from test_gpu_barebone_walls import GOAL, building, discs_of, task

N, T, S, B, ALPHA = 64, 18, 3, 2, 0.5
SHAPES = ((7, 10), (70, 74))  # (K, W)
WSCALES = (1.0, 1.5)          # rotation on, off
OFFSETS = (0, 3)              # with T + 1 rows, offset 3 reaches the clamp of every kind of track
RING_ROWS, BODY = RINGS[2], FOOTPRINTS[3]
EXTRAS = (("samples",), ("rings",), ("footprint",), ("samples", "footprint"), ("rings", "footprint"))

# A row of the sweep: (discs, walls, goal, extra, one_row).  The 12 plain forms: TRACKS off and on x walls none, static,
# tracks x goal.  The 20 with samples, rings or a footprint, over walls none or tracks x goal; `one_row` -- every other one,
# a chequerboard over (extra, walls x goal) -- gives the row static discs (samples of one row) and static walls, which
# crowd_form runs as tracks of one row: the form is the same, the arguments reach it through the normalisation.
PLAIN_ROWS = [(discs, walls, goal, (), False) for discs in ("static", "tracks") for walls in ("none", "static", "tracks")
              for goal in (False, True)]
EXTRA_ROWS = [("static" if (i + j) % 2 else "tracks", walls, goal, extra, (i + j) % 2 == 1)
              for i, extra in enumerate(EXTRAS) for j, (walls, goal) in enumerate(itertools.product(("none", "tracks"), (False, True)))]
ROWS = PLAIN_ROWS + EXTRA_ROWS
# (the mixed-count batch: plain, a goal track, rings + footprint, samples + footprint -- nothing of one row)
MIXED_ROWS = [("tracks", "tracks", False, (), False), ("tracks", "tracks", True, (), False),
              ("tracks", "tracks", False, ("rings", "footprint"), False), ("tracks", "tracks", False, ("samples", "footprint"), False)]
MIXED_DISCS, MIXED_WALLS, MIXED_OFFSETS = (70, 7, 0), (10, 74, 0), (0, 3, 1)


def form_of(row):
    """The instantiation a row runs, as crowd_form (csrc/barebone_plan.h) normalises it: (TRACKS, walls kind, goal, samples,
    rings, footprint).  Samples, rings and a footprint run TRACKS forms, static walls as wall tracks of one row."""
    discs, walls, goal, extra, _ = row
    return (discs == "tracks" or bool(extra), "tracks" if extra and walls == "static" else walls, goal,
            "samples" in extra, "rings" in extra, "footprint" in extra)


def moves(row):
    """Whether anything the row holds has more than one row, so that the track offset counts."""
    discs, walls, goal, extra, one_row = row
    return goal or ((discs == "tracks" or walls == "tracks") and not one_row) or ("samples" in extra and not one_row)


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def scene(K, W, wscale):
    """K discs, W walls, rotation on (wscale 1.0) or off (1.5): the first N rollouts of task(T, wscale) as problem 0, and a
    problem 1 with the same start, goal and obstacles and its own controls and noise (seed 500 + 10 * wscale: problem 1 is
    not a copy of problem 0)."""
    params, u0, noise0 = task(T, wscale)
    u1, noise1 = inputs(np.random.default_rng(500 + int(10 * wscale)), N, T)
    pos, rad = discs_of(K, "static", T, params)
    tracks, track_rad = discs_of(K, "tracks", T, params)
    assert (rad == track_rad).all()
    seg, hw = building(W)
    wtracks, track_hw = moving_building(W, T + 1)
    assert (hw == track_hw).all()
    # (the generators' walls in reverse order: of their scattered walls 64 .. 73 the rollouts hit none or one, so their four
    # fixed walls, which every rollout meets, go last -- into the partial tile -- and the scattered ones fill the full tile)
    seg, hw, wtracks = seg[::-1].copy(), hw[::-1].copy(), wtracks[::-1].copy()
    samples, sample_rad = sample_set(K, S, T + 1)
    samples1, sample1_rad = sample_set(K, S, 1)
    u, noise = _frozen(np.stack([u0, u1]), np.stack([noise0[:N], noise1]))
    _frozen(pos, rad, tracks, seg, hw, wtracks)
    return dict(K=K, W=W, wscale=wscale, params=params, u=u, noise=noise, pos=pos, rad=rad, tracks=tracks, seg=seg, hw=hw,
                wtracks=wtracks, goal_track=crossing_goal(T, T + 1), samples=samples, sample_rad=sample_rad, samples1=samples1,
                sample1_rad=sample1_rad)


def scenes():
    return [(K, W, wscale) for K, W in SHAPES for wscale in WSCALES]


def row_params(sc, row, discs=None, walls=None):
    """The planner's params of a row.  discs, walls: False leaves that kind out (a batch with per-problem sets hands them
    over on its own)."""
    kind, wall_kind, goal, extra, one_row = row
    p = {k: v for k, v in sc["params"].items() if k != "xgoal"}
    if "samples" in extra:
        smp, rad = (sc["samples1"], sc["sample1_rad"]) if one_row else (sc["samples"], sc["sample_rad"])
        p["obstacle_track_samples"], p["obstacle_radius"], p["cvar_alpha"] = smp, rad, ALPHA
    elif discs is not False:
        p["obstacle_radius"] = sc["rad"]
        if kind == "tracks":
            p["obstacle_tracks"] = sc["tracks"]
        else:
            p["obstacle_positions"] = sc["pos"]
    if walls is not False and wall_kind != "none":
        p["wall_halfwidth"] = sc["hw"]
        if wall_kind == "tracks" and not one_row:
            p["wall_tracks"] = sc["wtracks"]
        else:
            p["wall_segments"] = sc["seg"]
    if goal:
        p["goal_track"] = sc["goal_track"]
    else:
        p["xgoal"] = GOAL.copy()
    if "rings" in extra:
        p["clearance_rings"] = RING_ROWS
    if "footprint" in extra:
        p["footprint"] = BODY
    return p


def oracle_of(sc, row):
    """The model's parameters: with a goal track the static goal rests and holds the track's first row."""
    p = {k: v for k, v in sc["params"].items() if not k.startswith("wall_")}
    return oracle_params(dict(p, xgoal=sc["goal_track"][0]) if row[2] else p)


def model_args(sc, row, K=None, W=None):
    """(tracks or samples, radii, seg, hw, keywords) of form_model.costs for a row; K, W: the first K discs and the last W walls
    of the scene (a problem's own sets in the mixed-count batch; disc samples are shared by the problems: always the whole set)."""
    kind, wall_kind, goal, extra, one_row = row
    K, W = sc["K"] if K is None else K, sc["W"] if W is None else W
    if "samples" in extra:
        discs, rad = (sc["samples1"], sc["sample1_rad"]) if one_row else (sc["samples"], sc["sample_rad"])
    else:
        discs, rad = (sc["tracks"] if kind == "tracks" else sc["pos"][:, None, :])[:K], sc["rad"][:K]
    seg = hw = None
    if wall_kind != "none" and W:
        seg, hw = (sc["wtracks"] if wall_kind == "tracks" and not one_row else sc["seg"])[sc["W"] - W:], sc["hw"][sc["W"] - W:]
    kw = dict(footprint=BODY if "footprint" in extra else None, rings=RING_ROWS if "rings" in extra else None,
              goal_track=sc["goal_track"] if goal else None)
    if "samples" in extra:
        kw["alpha"] = ALPHA
    return discs, rad, seg, hw, kw


@functools.lru_cache(maxsize=None)
def model(K, W, wscale, row, b=0, offset=0):
    """((N,) float32 costs, (N, S) sample columns or None) of problem b of a row at a track offset: the model, made once."""
    sc = scene(K, W, wscale)
    if not moves(row) and offset:
        return model(K, W, wscale, row, b, 0)
    discs, rad, seg, hw, kw = model_args(sc, row)
    alpha = kw.pop("alpha", None)
    per = form_model.sample_costs(oracle_of(sc, row), discs, rad, seg, hw, sc["noise"][b], sc["u"][b], offset=offset, **kw)
    costs = per[:, 0].copy() if alpha is None else cvar_tail(per, alpha)
    _frozen(costs, per)
    return costs, (per if alpha is not None else None)


@functools.lru_cache(maxsize=None)
def mixed_model(wscale, row, b):
    """Problem b of the mixed-count batch: its own first MIXED_DISCS[b] discs and last MIXED_WALLS[b] walls of the (70, 74) scene
    -- disc samples are shared by the problems of a batch: all 70 --, its own track offset, controls and noise (problem 2:
    seed 520 + 10 * wscale)."""
    sc = scene(70, 74, wscale)
    u, noise = mixed_inputs(wscale)
    discs, rad, seg, hw, kw = model_args(sc, row, MIXED_DISCS[b], MIXED_WALLS[b])
    costs = form_model.costs(oracle_of(sc, row), discs, rad, seg, hw, noise[b], u[b], offset=MIXED_OFFSETS[b], **kw)
    return _frozen(costs)[0]


@functools.lru_cache(maxsize=None)
def mixed_inputs(wscale):
    sc = scene(70, 74, wscale)
    u2, noise2 = inputs(np.random.default_rng(520 + int(10 * wscale)), N, T)
    return _frozen(np.concatenate([sc["u"], u2[None]]), np.concatenate([sc["noise"], noise2[None]]))
