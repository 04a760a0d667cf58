"""Model of the barebone planner's wall obstacles (numpy, CPU): the test k_rollout_barebone_crowd<..., WALLS> makes, written
once, and the cost chain of crowd_model run on `disc hits + wall hits`.

A wall is a segment A -> B with a half-width h >= 0, all float32.  Step t of a rollout moves the robot from P (the position
before the step; x0 for t = 0) to Q, and it hits the wall iff the distance between the closed segments PQ and AB is <= h.
`hit` is that statement without a division: every float32 input widened to float64 first, every subtraction, product and
comparison in float64, dot and cross products as ax*bx + ay*by and ax*by - ay*bx, no fma.  The kernel does the same IEEE
operations in the same order, so the verdicts are equal bit for bit; tests/test_wall_model.py compares `hit` with the same
formula in exact rational arithmetic and with a dense-sampling distance."""
import numpy as np

import crowd_model
from oracle import oracle as O


def _near(wx, wy, ux, uy, LL, hh):
    """near(X; U, dU, LL) with w = X - U given: X within sqrt(hh) of the segment U -> U + dU (LL = dU.dU)."""
    s = wx * ux + wy * uy
    before = wx * wx + wy * wy <= hh
    vx, vy = wx - ux, wy - uy
    past = vx * vx + vy * vy <= hh
    c = wx * uy - wy * ux
    beside = c * c <= hh * LL
    return np.where(s <= 0.0, before, np.where(s >= LL, past, beside))


def hit(P, Q, A, B, h):
    """P, Q, A, B: (..., 2) float32 (broadcast against each other), h (...) float32 -> bool: step P -> Q hits wall A -> B."""
    P, Q, A, B = (np.asarray(v, np.float32).astype(np.float64) for v in (P, Q, A, B))
    h = np.asarray(h, np.float32).astype(np.float64)
    px, py, qx, qy = P[..., 0], P[..., 1], Q[..., 0], Q[..., 1]
    ax, ay, bx, by = A[..., 0], A[..., 1], B[..., 0], B[..., 1]
    dx, dy = bx - ax, by - ay
    ex, ey = qx - px, qy - py
    hh, LLd, LLe = h * h, dx * dx + dy * dy, ex * ex + ey * ey
    pax, pay, qax, qay = px - ax, py - ay, qx - ax, qy - ay
    apx, apy, bpx, bpy = ax - px, ay - py, bx - px, by - py
    o1, o2 = dx * pay - dy * pax, dx * qay - dy * qax
    o3, o4 = ex * apy - ey * apx, ex * bpy - ey * bpx
    crossing = (((o1 > 0) & (o2 < 0)) | ((o1 < 0) & (o2 > 0))) & (((o3 > 0) & (o4 < 0)) | ((o3 < 0) & (o4 > 0)))
    return (crossing | _near(pax, pay, dx, dy, LLd, hh) | _near(qax, qay, dx, dy, LLd, hh) |
            _near(apx, apy, ex, ey, LLe, hh) | _near(bpx, bpy, ex, ey, LLe, hh))


def pure_crossing(P, Q, A, B, h):
    """A hit in which neither P nor Q is within h of the wall: the step jumps it (the no-tunnelling case)."""
    return hit(P, Q, A, B, h) & ~hit(P, P, A, B, h) & ~hit(Q, Q, A, B, h)


def _walls(segments, halfwidths):
    seg = np.asarray(segments, np.float32).reshape(-1, 2, 2)
    hw = np.ascontiguousarray(np.broadcast_to(np.asarray(halfwidths, np.float32), (len(seg),)))
    return seg, hw


def states(p, noise, u):
    """(n, T+1, 3) float32: the oracle's own state rollouts (row 0: x0), as crowd_model.hit_counts takes them."""
    noise = np.ascontiguousarray(noise, np.float32)
    u = np.ascontiguousarray(u, np.float32)
    return O.state_rollout_barebone(p, np.concatenate([noise[:1] * 0, noise]), u, u, len(noise) + 1)[1:]


def wall_hits_of_states(st, segments, halfwidths):
    """(n, T) int64: how many walls step t hits, for states (n, T+1, >=2)."""
    seg, hw = _walls(segments, halfwidths)
    n, T = st.shape[0], st.shape[1] - 1
    counts = np.zeros((n, T), np.int64)
    for k0 in range(0, len(seg), 64):  # (integers: the order does not matter)
        A, B, h = seg[None, None, k0:k0 + 64, 0], seg[None, None, k0:k0 + 64, 1], hw[None, None, k0:k0 + 64]
        counts += hit(st[:, :-1, None, :2], st[:, 1:, None, :2], A, B, h).sum(axis=2)
    return counts


def wall_hits(p, segments, halfwidths, noise, u):
    """(n, T) int64 wall hits per (rollout, step); p: oracle parameters (track_model.oracle_params)."""
    return wall_hits_of_states(states(p, noise, u), segments, halfwidths)


def chain(p, counts, st, noise, u):
    """crowd_model.crowd_costs' cost chain on given hit counts (n, T) and states (n, T+1, 3) -> (n,) float32."""
    noise = np.ascontiguousarray(noise, np.float32)
    u = np.ascontiguousarray(u, np.float32)
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


def active_steps(p, st):
    """(n, T) bool: step t still counts -- no EARLIER step ended within the goal tolerance (the freeze)."""
    xg, yg = np.float32(p.xgoal[0]), np.float32(p.xgoal[1])
    gt2 = np.float64(np.float32(p.goal_tolerance) * np.float32(p.goal_tolerance))
    dx, dy = (xg - st[:, 1:, 0]).astype(np.float64), (yg - st[:, 1:, 1]).astype(np.float64)
    at_goal = dx * dx + dy * dy <= gt2
    before = np.cumsum(at_goal, axis=1) - at_goal
    return before == 0


def wall_costs(p, tracks, radii, segments, halfwidths, noise, u, offset=0):
    """Costs (n,) float32 with discs (tracks (K, L, 2), radii (K,); K = 0: none) and walls: the cost chain of
    crowd_model.crowd_costs on disc hits + wall hits."""
    disc_counts, st = crowd_model.hit_counts(p, tracks, radii, noise, u, offset)
    return chain(p, disc_counts + wall_hits_of_states(st, segments, halfwidths), st, noise, u)
