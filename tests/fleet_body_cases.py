"""The inputs of the fleet-of-bodies comparisons, and the model's answers to them, computed once and shared by
tests/test_fleet_body_model.py (CPU: the inputs mean something, and sine and cosine may move) and
tests/test_gpu_barebone_fleet_bodies.py (GPU: the device gives the same bits).  Nothing here is changed after it is made."""
import functools

import numpy as np

import fleet_body_model as M
import wall_model
from test_gpu_barebone_batch import make_params, oracle_params, problem_params
from test_gpu_barebone_fleet import ROOM, ROOM_HW, ring

DT = 0.1
N = 64
MARGIN = 0.05
DYADIC = (0.25, 0.125)  # rho, margin of the one-disc body: every sum of them is exact in float32

# (B, F, W): 8 grouped slots, then singles in one tile | 72 grouped slots: groups span two tiles | 68 slots: a tile
# boundary at a group boundary and statics behind.  Per horizon the ring's (radius, seed): found by a scan over radii in
# steps of 0.1 m and seeds 1 .. 3 with the model on the CPU, the first pair at which, for wscale 1.0 and 1.5 alike, at
# least a tenth of every reader's rollouts hit some robot and at least a tenth hit none (asserted again by
# test_fleet_body_model.py and by every GPU case).
FLEETS = {(3, 3, 2, 12): (2.1, 1), (3, 3, 2, 37): (3.4, 3), (10, 8, 3, 12): (2.8, 1), (10, 8, 3, 37): (6.1, 3),
          (18, 3, 2, 12): (4.0, 1), (18, 3, 2, 37): (9.4, 1)}
COST_CASES = [(B, F, W, t, wscale) for (B, F, W, t) in FLEETS for wscale in (1.0, 1.5)]
WALL_CASES = [(B, F, t, wscale) for (B, F, t) in ((2, 1, 12), (3, 3, 37), (10, 8, 12), (66, 3, 12), (3, 3, 70)) for wscale in (1.0, 1.5)]
EXTRA_CASES = ["disc_tracks", "goal_track", "disc_samples"]
TRACK_OFFSET = 5
ALPHA = 0.5

# two carts in a corridor (test_gpu_barebone_fleet_bodies.test_two_carts_meet_in_a_corridor)
CART = (0.5, 0.5, 0.4)   # front, rear, width: 1.0 m x 0.4 m, three discs of radius 0.26 m; circumscribed radius 0.54 m
CORRIDOR_WIDTH = 1.8     # m between the wall lines
WALL_HW, CART_MARGIN, CIRCUMSCRIBED = 0.05, 0.05, 0.54
LOOP_STEPS = 120
CORRIDOR = np.float32([[[-2.0, CORRIDOR_WIDTH / 2], [8.0, CORRIDOR_WIDTH / 2]], [[-2.0, -CORRIDOR_WIDTH / 2], [8.0, -CORRIDOR_WIDTH / 2]]])


def body(F):
    """The cart of the scenario, 1.0 m x 0.4 m, covered by F discs on its axis (F = 1: its circumscribed disc)."""
    from mppi_numba_amd.barebone import rectangle_footprint
    return rectangle_footprint(0.5, 0.5, 0.4, count=F)


@functools.lru_cache(maxsize=None)
def scene(B, t, seed, radius):
    """B robots on a ring of that radius, aimed at each other through the centre as test_gpu_barebone_fleet.ring(aimed=True)
    aims them (give or take 0.1 rad), bound for the far side.  Controls as ring() draws them, some speeds outside vrange and
    one turn rate outside wrange so that the clip takes part; noise (B, N, t, 2) of deviation 1, so that a reader's rollouts
    fan out and the others' plans are hit by some of them and missed by others.  Shared by the cases, never changed."""
    rng = np.random.default_rng(seed)
    angle = 0.3 + np.arange(B) * (2 * np.pi / B)
    where = radius * np.stack([np.cos(angle), np.sin(angle)], 1)
    heading = angle + np.pi + rng.uniform(-0.1, 0.1, B)
    x0s = np.concatenate([where, heading[:, None]], 1).astype(np.float32)
    goals = (-where).astype(np.float32)
    us = np.stack([rng.uniform(0.8, 1.8, (B, t)), rng.uniform(-0.2, 0.2, (B, t))], 2).astype(np.float32)
    us[:, 4, 0], us[:, 7, 0], us[0, 9, 1] = -1.0, 5.0, -40.0
    noise = rng.normal(0, 1.0, (B, N, t, 2)).astype(np.float32)
    for a in (x0s, goals, us, noise):
        a.setflags(write=False)
    return x0s, goals, us, noise


def reader_params(params, x0, goal):
    return oracle_params(problem_params(params, x0, goal))


def model_of(params, x0s, goals, us, noise, footprint, margin, W, discs=None, rad=None, offset=0, goal_tracks=None, samples=None,
             alpha=None):
    """dict: costs (B, n) float32, hit_some (B, n) bool -- the rollout hits some other robot at some step --, grouped and
    per_slot (B,) int -- the hits of all rollouts and steps counted per robot and per wall slot."""
    B = len(x0s)
    walls = M.body_walls(params, x0s, us, footprint)
    hw = M.halfwidths(footprint, margin)
    costs, some, grouped, per_slot = [], [], [], []
    for a in range(B):
        track = None if goal_tracks is None else goal_tracks[a]
        p = reader_params(params, x0s[a], goals[a] if track is None else track[0])
        st = wall_model.states(p, noise[a], us[a])
        robots, slots = M.robot_hits(st, footprint, walls[a], hw)
        some.append(robots.any(axis=(1, 2)))
        grouped.append(int(robots.sum()))
        per_slot.append(int(slots.sum()))
        if samples is not None:
            costs.append(M.sampled_costs(p, footprint, walls[a], hw, noise[a], us[a], samples, rad, alpha, ROOM[:W], ROOM_HW[:W], offset))
        else:
            costs.append(M.costs(p, footprint, walls[a], hw, noise[a], us[a], ROOM[:W], ROOM_HW[:W], discs, rad, offset, track))
    return dict(costs=np.stack(costs), hit_some=np.stack(some), grouped=np.array(grouped), per_slot=np.array(per_slot), walls=walls, hw=hw)


@functools.lru_cache(maxsize=None)
def cost_case(B, F, W, t, wscale):
    radius, seed = FLEETS[(B, F, W, t)]
    x0s, goals, us, noise = scene(B, t, seed, radius)
    params = make_params(DT, wscale)
    footprint = body(F)
    return dict(params=params, x0s=x0s, goals=goals, us=us, noise=noise, footprint=footprint, margin=MARGIN, W=W,
                model=model_of(params, x0s, goals, us, noise, footprint, MARGIN, W))


@functools.lru_cache(maxsize=None)
def extra_case(kind):
    """(B = 3, F = 3, W = 2), T = 37, with 70 shared disc tracks read at a nonzero offset, with a goal track per problem, or
    with three disc samples (alpha = 0.5)."""
    from mppi_numba_amd.barebone import constant_velocity_tracks, sampled_tracks
    B, F, W, t = 3, 3, 2, 37
    radius, seed = FLEETS[(B, F, W, t)]
    x0s, goals, us, noise = scene(B, t, seed, radius)
    params = make_params(DT, 1.0)
    footprint = body(F)
    rng = np.random.default_rng(len(kind))
    case = dict(params=params, x0s=x0s, goals=goals, us=us, noise=noise, footprint=footprint, margin=MARGIN, W=W, kind=kind)
    if kind == "disc_tracks":
        case["tracks"] = constant_velocity_tracks(rng.uniform(-1.5, 1.5, (70, 2)), rng.normal(0, 0.4, (70, 2)), DT, t + 6)
        case["rad"] = rng.uniform(0.05, 0.15, 70).astype(np.float32)
        case["model"] = model_of(params, x0s, goals, us, noise, footprint, MARGIN, W, case["tracks"], case["rad"], TRACK_OFFSET)
    elif kind == "goal_track":
        case["goal_tracks"] = [constant_velocity_tracks(goals[b][None], rng.normal(0, 0.5, (1, 2)), DT, 20)[0] for b in range(B)]
        case["model"] = model_of(params, x0s, goals, us, noise, footprint, MARGIN, W, goal_tracks=case["goal_tracks"])
    else:
        case["samples"] = sampled_tracks(rng.uniform(-1.5, 1.5, (6, 2)), rng.normal(0, 0.4, (6, 2)), DT, t + 1, 0.5, 3, seed=2)
        case["rad"] = rng.uniform(0.05, 0.15, 6).astype(np.float32)
        case["model"] = model_of(params, x0s, goals, us, noise, footprint, MARGIN, W, rad=case["rad"], samples=case["samples"], alpha=ALPHA)
    return case


@functools.lru_cache(maxsize=None)
def wall_case(B, F, t, wscale):
    """Random start headings, random controls with entries outside vrange / wrange, as the disc fleet's wall test draws them."""
    x0s, goals, us, _ = ring(B, 64, t, 100 * B + t, aimed=False)
    params = make_params(DT, wscale)
    footprint = body(F) if F > 1 else np.float32([[0.0, 0.0, DYADIC[0]]])
    return dict(params=params, x0s=x0s, goals=goals, us=us, footprint=footprint, margin=MARGIN,
                walls=M.body_walls(params, x0s, us, footprint), hw=M.halfwidths(footprint, MARGIN))


def the_input_means_something(model):
    """Of the model's counts (the reference, not the device): at least a tenth of every reader's rollouts hit some robot,
    at least a tenth hit none, and counting per robot gives strictly fewer hits than counting per slot."""
    share = model["hit_some"].mean(axis=1)
    assert (share >= 0.1).all() and (share <= 0.9).all(), "bad input: the share of rollouts that hit some robot, per reader: %s" % share
    assert model["grouped"].sum() < model["per_slot"].sum(), "bad input: no step hits two slots of one robot"
    return share


def moved_counts(case, ds, dc):
    """The wall endpoints and the hit counts of a case with sine and cosine moved by ds, dc everywhere centres are formed."""
    walls = M.body_walls(case["params"], case["x0s"], case["us"], case["footprint"], None, ds, dc)
    hw = M.halfwidths(case["footprint"], case["margin"])
    counts = []
    for a in range(len(case["x0s"])):
        p = reader_params(case["params"], case["x0s"][a], case["goals"][a])
        st = wall_model.states(p, case["noise"][a], case["us"][a])
        counts.append(M.wall_counts(st, case["footprint"], walls[a], hw, ROOM[:case["W"]], ROOM_HW[:case["W"]], ds, dc))
    return walls, np.stack(counts)


