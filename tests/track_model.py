"""Cost model of the barebone rollout with discs that move (numpy, CPU): the reference planner has no moving obstacles,
so the reference for them is built from the oracle's own positions plus plain IEEE arithmetic.

A track is (K, L, 2) float32, row j a disc's centre at time j*dt from "now"; "now" is row `offset`.  The state after
step t (t = 0 .. T-1) is tested against row min(offset + t + 1, L - 1).  Everything else is the notebook's cell-3 kernel
as oracle.rollout_barebone restates it: the float32-rounded cost chain, one addition per disc in the order of the discs,
the freeze at the goal, the terminal term and the T control-cost terms.  No fma is needed: the squares of widened
float32 values are exact in float64.  With tracks whose rows are all equal the model gives the bits of
oracle.rollout_barebone (tests/test_track_model.py)."""
import numpy as np

from oracle import oracle as O


def oracle_params(params):
    return O.make_params(params, 1.0, [0, 0], [0, 0], [0.0, 1.0], [0.0, 1.0], default_obs_cost=1e3, default_dist_weight=10)


def track_costs(p, tracks, radii, noise, u, offset=0):
    """p: oracle parameters (oracle_params); tracks (K, L, 2), radii (K,), noise (n, T, 2), u (T, 2) -> (n,) float32."""
    noise = np.ascontiguousarray(noise, np.float32)
    u = np.ascontiguousarray(u, np.float32)
    tracks = np.asarray(tracks, np.float32)
    radii = np.asarray(radii, np.float32)
    assert tracks.ndim == 3 and tracks.shape[0] == len(radii) and tracks.shape[1] >= 1 and tracks.shape[2] == 2
    n, T = noise.shape[:2]
    # rows b >= 1 of the oracle's state rollouts are clip(u_prev + noise[b]); row 0 is u_cur, no noise, no clip
    st = O.state_rollout_barebone(p, np.concatenate([noise[:1] * 0, noise]), u, u, n + 1)[1:]  # (n, T+1, 3)
    xg, yg = np.float32(p.xgoal[0]), np.float32(p.xgoal[1])
    gt2 = np.float64(np.float32(p.goal_tolerance) * np.float32(p.goal_tolerance))
    K, L = tracks.shape[:2]
    cost = np.zeros(n, np.float32)
    d2 = np.full(n, 1e9)
    done = np.zeros(n, bool)
    reached = np.zeros(n, bool)
    obs_cost = np.float64(np.float32(p.obs_cost))
    for t in range(T):
        x, y = st[:, t + 1, 0], st[:, t + 1, 1]
        dx, dy = (xg - x).astype(np.float64), (yg - y).astype(np.float64)
        nd2 = dx * dx + dy * dy
        c1 = (cost.astype(np.float64) + p.dist_weight * nd2).astype(np.float32)
        row = min(offset + t + 1, L - 1)
        for k in range(K):
            ex = (x - tracks[k, row, 0]).astype(np.float64)
            ey = (y - tracks[k, row, 1]).astype(np.float64)
            diff = ex * ex + ey * ey - np.float64(radii[k]) * np.float64(radii[k])
            hit = 1.0 - (diff > 0.0).astype(np.float64)
            c1 = (c1.astype(np.float64) + hit * obs_cost).astype(np.float32)
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


def reached_goal(p, noise, u):
    """Which rollouts get within the goal tolerance at some step (for a test's own sanity checks)."""
    noise = np.ascontiguousarray(noise, np.float32)
    u = np.ascontiguousarray(u, np.float32)
    st = O.state_rollout_barebone(p, np.concatenate([noise[:1] * 0, noise]), u, u, len(noise) + 1)[1:]
    dx = (np.float32(p.xgoal[0]) - st[:, 1:, 0]).astype(np.float64)
    dy = (np.float32(p.xgoal[1]) - st[:, 1:, 1]).astype(np.float64)
    gt2 = np.float64(np.float32(p.goal_tolerance) * np.float32(p.goal_tolerance))
    return ((dx * dx + dy * dy) <= gt2).any(axis=1)
