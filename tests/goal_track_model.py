"""Model of the barebone planner's goal tracks (numpy, CPU): a goal that moves, built on wall_model.chain.

A goal track is (L, 2) float32, row j the goal's position at time j*dt from "now" = row `offset` -- an instant, like a disc
row.  The state after step t (t = 0 .. T-1) is measured against row min(offset + t + 1, L - 1); the raw offset is clamped
against the goal track's own row count, as each kind of track does.  Everything else is wall_model.chain, statement for
statement: the stage term dist_weight * d2 of the float32 differences (gx - x, gy - y) widened to double, `count` rounded
additions of obs_cost, the goal test d2 <= gt2 against that step's row, the freeze of cost, d2 and `reached`, the terminal
term (1 - reached) * d2 with the last live d2, and the T control-cost terms.  The hit counts come from crowd_model.hit_counts
and wall_track_model.wall_track_hits_of_states, so discs, disc tracks, walls and wall tracks all combine with it; with
equal rows it gives the bits of wall_model.chain (tests/test_goal_track_model.py), and so of oracle.rollout_barebone."""
import numpy as np

import crowd_model
from wall_track_model import wall_track_hits_of_states


def goal_rows(track, T, offset=0):
    """(T, 2) float32: the goal the state after step t is measured against, t = 0 .. T-1."""
    tr = np.asarray(track, np.float32)
    assert tr.ndim == 2 and tr.shape[0] >= 1 and tr.shape[1] == 2, tr.shape
    return tr[np.minimum(int(offset) + np.arange(T) + 1, len(tr) - 1)]


def goal_d2(goals, st):
    """(n, T) float64: squared distance of the state after step t to that step's goal, goals (T, 2), states (n, T+1, >=2)."""
    dx = (goals[None, :, 0] - st[:, 1:, 0]).astype(np.float64)
    dy = (goals[None, :, 1] - st[:, 1:, 1]).astype(np.float64)
    return dx * dx + dy * dy


def freeze_step(p, goals, st):
    """(n,) int: the first step whose state lies within the tolerance of that step's goal; T: the rollout never does."""
    gt2 = np.float64(np.float32(p.goal_tolerance) * np.float32(p.goal_tolerance))
    at_goal = goal_d2(goals, st) <= gt2
    return np.where(at_goal.any(axis=1), at_goal.argmax(axis=1), at_goal.shape[1])


def chain(p, counts, st, noise, u, goals):
    """wall_model.chain with the goal of each step: hit counts (n, T), states (n, T+1, 3), goals (T, 2) -> (n,) float32."""
    noise = np.ascontiguousarray(noise, np.float32)
    u = np.ascontiguousarray(u, np.float32)
    goals = np.asarray(goals, np.float32)
    n, T = noise.shape[:2]
    assert goals.shape == (T, 2)
    gt2 = np.float64(np.float32(p.goal_tolerance) * np.float32(p.goal_tolerance))
    cost = np.zeros(n, np.float32)
    d2 = np.full(n, 1e9)
    done = np.zeros(n, bool)
    reached = np.zeros(n, bool)
    obs_cost = np.float64(np.float32(p.obs_cost))
    for t in range(T):
        x, y = st[:, t + 1, 0], st[:, t + 1, 1]
        dx, dy = (goals[t, 0] - x).astype(np.float64), (goals[t, 1] - y).astype(np.float64)
        nd2 = dx * dx + dy * dy
        c1 = (cost.astype(np.float64) + p.dist_weight * nd2).astype(np.float32)
        for k in range(int(counts[:, t].max()) if n else 0):
            c1 = np.where(k < counts[:, t], (c1.astype(np.float64) + obs_cost).astype(np.float32), c1)
        act = ~done
        cost = np.where(act, c1, cost)
        d2 = np.where(act, nd2, d2)
        at_goal = nd2 <= gt2
        reached |= act & at_goal
        done |= at_goal
    cost = (cost.astype(np.float64) + (1.0 - reached.astype(np.float64)) * d2).astype(np.float32)
    s0 = np.float64(np.float32(p.u_std[0])) ** 2
    s1 = np.float64(np.float32(p.u_std[1])) ** 2
    lam = np.float64(np.float32(p.lambda_weight))
    for t in range(T):
        a = (np.float64(u[t, 0]) / s0) * noise[:, t, 0].astype(np.float64)
        b = (np.float64(u[t, 1]) / s1) * noise[:, t, 1].astype(np.float64)
        cost = (cost.astype(np.float64) + lam * (a + b)).astype(np.float32)
    return cost


NO_DISCS = np.zeros((0, 1, 2), np.float32), np.zeros(0, np.float32)


def goal_track_costs(p, goal_track, noise, u, offset=0, disc_tracks=None, radii=None, wall_tracks=None, halfwidths=None):
    """Costs (n,) float32 with a goal track (L, 2), discs (tracks (K, Ld, 2), radii (K,); None: none) and walls (tracks
    (W, Lw, 2, 2), half-widths; None: none), all at the one offset, each kind clamped against its own row count."""
    if disc_tracks is None:
        disc_tracks, radii = NO_DISCS
    counts, st = crowd_model.hit_counts(p, disc_tracks, radii, noise, u, offset)
    if wall_tracks is not None:
        counts = counts + wall_track_hits_of_states(st, wall_tracks, halfwidths, offset)
    return chain(p, counts, st, noise, u, goal_rows(goal_track, st.shape[1] - 1, offset))
