"""Model of the barebone planner's fleet mode (numpy, CPU): robots that avoid each other's plans.  Nothing new in
arithmetic -- the pieces the fleet rests on, put together the way mppi_planner_set_fleet defines it.

The problems of a batch are robots.  The plan of robot b is the noise-free rollout of its control sequence from its start
state: wall_model.states (the oracle's own state rollout: the clip to vrange / wrange, float32 state) with zero noise.  The
wall that stands for b is barebone.swept_walls of that plan -- row j the segment [c_j, c_{j+1}] -- and reader a is given the
walls of the B - 1 others in ascending order, a skipped, with half-width float32(r_a + r_b + margin) summed in float64 from
the float32 radii; behind them the static walls, every row the same segment.  The fleet rows are counted from "now": step t
meets row min(t, T - 1) = t whatever the problem's track offset is, while disc tracks and goal tracks keep the offset.  So
the costs of reader a are wall_model.chain (goal_track_model.chain with a goal track) on
crowd_model.hit_counts(..., offset) + wall_track_model.wall_track_hits_of_states(st, walls_a, hw_a, offset=0)."""
import numpy as np

import crowd_model
import goal_track_model
from track_model import oracle_params
from wall_model import chain, states
from wall_track_model import wall_track_hits_of_states


def others(count):
    """(B, B - 1) int: reader a's others in ascending order, a skipped."""
    return np.array([[b for b in range(count) if b != a] for a in range(count)], dtype=np.int64).reshape(count, count - 1)


def halfwidths(radii, margin, count):
    """(B, B - 1) float32: float32(float64(r_a) + float64(r_b) + float64(margin)) for reader a (rows) and its others."""
    r = np.ascontiguousarray(np.broadcast_to(np.asarray(radii, np.float64).astype(np.float32), (count,))).astype(np.float64)
    full = ((r[:, None] + r[None, :]) + np.float64(margin)).astype(np.float32)
    return full[np.arange(count)[:, None], others(count)]


def plans(params, x0s, us, parked=None):
    """(B, T + 1, 3) float32: every robot's noise-free rollout; params: the shared task (a dict with vrange, wrange, dt
    ...), x0s (B, 3), us (B, T, 2).  parked: (B,) bool -- such a robot stands at float32(x0)."""
    us = np.asarray(us, np.float32)
    B, T = us.shape[:2]
    out = np.empty((B, T + 1, 3), np.float32)
    for b in range(B):
        p = oracle_params(dict(params, x0=np.asarray(x0s[b], np.float64)))
        out[b] = states(p, np.zeros((1, T, 2), np.float32), us[b])[0]
        if parked is not None and parked[b]:
            out[b] = np.asarray(x0s[b], np.float64).astype(np.float32)[None]
    return out


def fleet_walls(params, x0s, us, parked=None):
    """(B, B - 1, T, 2, 2) float32: reader a's walls, swept_walls of the others' plans in ascending order."""
    from mppi_numba_amd.barebone import swept_walls
    st = plans(params, x0s, us, parked)
    B = len(st)
    per_robot = np.stack([swept_walls(st[b][None, :, :2])[0] for b in range(B)])  # (B, T, 2, 2)
    return per_robot[others(B)]


def reader_walls(walls_a, hw_a, static_seg=None, static_hw=None):
    """The wall tracks (B - 1 + W, T, 2, 2) and half-widths of one reader: the others, then the static walls in every row."""
    T = walls_a.shape[1]
    if static_seg is None or len(static_seg) == 0:
        return walls_a, np.asarray(hw_a, np.float32)
    seg = np.asarray(static_seg, np.float32).reshape(-1, 2, 2)
    shw = np.ascontiguousarray(np.broadcast_to(np.asarray(static_hw, np.float32), (len(seg),)))
    return (np.concatenate([walls_a, np.repeat(seg[:, None], T, axis=1)]), np.concatenate([np.asarray(hw_a, np.float32), shw]))


def fleet_hits(st, wtracks, hw):
    """(n, T) int64: the fleet's wall hits of states (n, T + 1, >= 2) -- rows from "now": offset 0."""
    return wall_track_hits_of_states(st, wtracks, hw, offset=0)


def fleet_costs(p, wtracks, hw, noise, u, disc_tracks=None, radii=None, offset=0, goal_track=None):
    """Costs (n,) float32 of one reader; p: its oracle parameters; wtracks, hw: reader_walls; discs (tracks (K, L, 2),
    radii; None: none) and a goal track (L, 2) at `offset`, the fleet rows at 0."""
    if disc_tracks is None:
        disc_tracks, radii = goal_track_model.NO_DISCS
    counts, st = crowd_model.hit_counts(p, disc_tracks, radii, noise, u, offset)
    counts = counts + fleet_hits(st, wtracks, hw)
    if goal_track is None:
        return chain(p, counts, st, noise, u)
    return goal_track_model.chain(p, counts, st, noise, u, goal_track_model.goal_rows(goal_track, st.shape[1] - 1, offset))
