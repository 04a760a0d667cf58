"""Cost model of the barebone rollout in crowd mode (numpy, CPU): what k_rollout_barebone_crowd does, in its order.

Positions first (the oracle's own state rollouts: a rollout's state never depends on the discs), then for every
(rollout, step) the NUMBER of discs the post-step position touches -- the double-precision test of track_model -- and only
then the cost chain: the distance term, `count` float32-rounded additions of obs_cost, the freeze at the goal; the terminal
term and the T control-cost terms as in track_model.track_costs.  tests/test_crowd_model.py shows that this equals
track_costs -- one rounded addition per DISC, hit or not -- bit for bit: a disc that is not hit adds +0.0, which leaves a
running cost that is never -0.0 as it is, and every disc that is hit adds the same obs_cost."""
import numpy as np

from oracle import oracle as O


def hit_counts(p, tracks, radii, noise, u, offset=0):
    """(n, T) int64: how many discs the state after step t touches; plus the states (n, T+1, 3)."""
    noise = np.ascontiguousarray(noise, np.float32)
    u = np.ascontiguousarray(u, np.float32)
    tracks = np.asarray(tracks, np.float32)
    radii = np.asarray(radii, np.float32)
    assert tracks.ndim == 3 and tracks.shape[0] == len(radii) and tracks.shape[1] >= 1 and tracks.shape[2] == 2
    n, T = noise.shape[:2]
    st = O.state_rollout_barebone(p, np.concatenate([noise[:1] * 0, noise]), u, u, n + 1)[1:]  # (n, T+1, 3)
    K, L = tracks.shape[:2]
    counts = np.zeros((n, T), np.int64)
    rr = radii.astype(np.float64) * radii.astype(np.float64)
    for t in range(T):
        row = min(offset + t + 1, L - 1)
        for k0 in range(0, K, 64):  # (the order the counts are taken in does not matter: integers)
            ex = (st[:, t + 1, 0, None] - tracks[None, k0:k0 + 64, row, 0]).astype(np.float64)  # float32 difference, widened
            ey = (st[:, t + 1, 1, None] - tracks[None, k0:k0 + 64, row, 1]).astype(np.float64)
            diff = ex * ex + ey * ey - rr[None, k0:k0 + 64]
            counts[:, t] += (~(diff > 0.0)).sum(axis=1)
    return counts, st


def crowd_costs(p, tracks, radii, noise, u, offset=0):
    """p: oracle parameters (track_model.oracle_params); tracks (K, L, 2), radii (K,), noise (n, T, 2), u (T, 2) ->
    (n,) float32."""
    noise = np.ascontiguousarray(noise, np.float32)
    u = np.ascontiguousarray(u, np.float32)
    counts, st = hit_counts(p, tracks, radii, noise, u, offset)
    n, T = noise.shape[:2]
    xg, yg = np.float32(p.xgoal[0]), np.float32(p.xgoal[1])
    gt2 = np.float64(np.float32(p.goal_tolerance) * np.float32(p.goal_tolerance))
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
        for h in range(int(counts[:, t].max()) if n else 0):  # to the largest count, predicated per rollout
            c1 = np.where(h < counts[:, t], (c1.astype(np.float64) + obs_cost).astype(np.float32), c1)
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


def crowd_discs(rng, count, x0, goal, overlapping=3):
    """`count` discs around the segment start -> goal, the first `overlapping` of them (as far as there are that many) on
    top of each other ON the segment, so that a rollout that goes straight is inside several discs at one step."""
    x0, goal = np.asarray(x0, np.float64)[:2], np.asarray(goal, np.float64)[:2]
    s = rng.uniform(0.2, 0.9, (count, 1))
    pos = x0 * (1 - s) + goal * s + rng.normal(0, 0.5, (count, 2))
    rad = rng.uniform(0.2, 0.8, count)
    m = min(overlapping, count)
    pos[:m] = x0 * 0.7 + goal * 0.3 + rng.normal(0, 0.05, (m, 2))
    rad[:m] = 0.6
    return pos.astype(np.float32), rad.astype(np.float32)
