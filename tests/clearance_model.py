"""Model of the barebone planner's clearance rings (numpy, CPU): params['clearance_rings'], built on the existing models only
-- crowd_model's disc arithmetic, wall_model's wall test, states and chain, footprint_model's centres, goal_track_model's rows;
the fleets hand it their walls (fleet_model.reader_walls, fleet_body_model.padded: tests/clearance_cases.py).

Rings are (R, 2) float32, rows (margin, penalty), margins ascending.  With m = (double)margin_l, obstacle k of a step is NEAR
at ring l iff the step would touch it were it m larger:

    disc k, point robot    crowd_model's test with rr = R * R, R = (double)r_k + m
    disc k, a footprint    footprint_model's with R = ((double)r_k + (double)rho_i) + m; near iff ANY body disc is
    wall k, point robot    wall_model.hit with hh = H * H, H = (double)h_k + m
    wall k, a footprint    H = ((double)h_k + (double)rho_i) + m per body disc chord; near iff any chord is

and a step that crosses a wall is inside every ring.  The wall test is written the way the kernel runs it for 1 + R sizes at
once: `wall_parts` gives the crossing bit and, of each of wall_model._near's four calls, the pair (num, den) of the branch
taken -- (wx^2 + wy^2, 1), (vx^2 + vy^2, 1) or (c^2, LL) --, and the verdict at hh is crossing | any(num_i <= hh * den_i).
tests/test_clearance_model.py shows that this is wall_model.hit at margin 0 and footprint_model.hit with rho for a margin.

n_l(t) counts the obstacles near at ring l in step t, the hit ones included.  The chain: the distance term, `hits` rounded
additions of obs_cost, for l = 1 .. R n_l rounded additions of penalty_l, the freeze."""
import numpy as np

import footprint_model
import goal_track_model
import wall_model

MAX_RINGS = 4


def rows_of(rings):
    rg = np.asarray(rings, np.float64).astype(np.float32)
    assert rg.ndim == 2 and rg.shape[1] == 2 and 1 <= len(rg) <= MAX_RINGS, rg.shape
    assert np.isfinite(rg).all() and (rg[:, 0] > 0).all() and (np.diff(rg[:, 0]) > 0).all() and (rg[:, 1] >= 0).all(), rg
    return rg


def near_parts(wx, wy, ux, uy, LL):
    """wall_model._near with the half-width left open: (num, den) of the branch taken; near(hh) is num <= hh * den."""
    s = wx * ux + wy * uy
    vx, vy = wx - ux, wy - uy
    c = wx * uy - wy * ux
    before, past = s <= 0.0, s >= LL
    num = np.where(before, wx * wx + wy * wy, np.where(past, vx * vx + vy * vy, c * c))
    den = np.where(before | past, 1.0, LL)
    return num, den


def wall_parts(P, Q, A, B):
    """P, Q, A, B: (..., 2) float32 (broadcast) -> (crossing (...) bool, num (4, ...), den (4, ...)): wall_model.hit,
    statement for statement, up to where the half-width comes in."""
    P, Q, A, B = (np.asarray(v, np.float32).astype(np.float64) for v in (P, Q, A, B))
    px, py, qx, qy = P[..., 0], P[..., 1], Q[..., 0], Q[..., 1]
    ax, ay, bx, by = A[..., 0], A[..., 1], B[..., 0], B[..., 1]
    dx, dy = bx - ax, by - ay
    ex, ey = qx - px, qy - py
    LLd, LLe = dx * dx + dy * dy, ex * ex + ey * ey
    pax, pay, qax, qay = px - ax, py - ay, qx - ax, qy - ay
    apx, apy, bpx, bpy = ax - px, ay - py, bx - px, by - py
    o1, o2 = dx * pay - dy * pax, dx * qay - dy * qax
    o3, o4 = ex * apy - ey * apx, ex * bpy - ey * bpx
    crossing = (((o1 > 0) & (o2 < 0)) | ((o1 < 0) & (o2 > 0))) & (((o3 > 0) & (o4 < 0)) | ((o3 < 0) & (o4 > 0)))
    parts = [near_parts(pax, pay, dx, dy, LLd), near_parts(qax, qay, dx, dy, LLd),
             near_parts(apx, apy, ex, ey, LLe), near_parts(bpx, bpy, ex, ey, LLe)]
    shape = np.broadcast(crossing, *[v for pair in parts for v in pair]).shape
    num = np.stack([np.broadcast_to(pair[0], shape) for pair in parts])
    den = np.stack([np.broadcast_to(pair[1], shape) for pair in parts])
    return np.broadcast_to(crossing, shape), num, den


def wall_verdict(parts, H):
    """The verdict at the half-width H (float64, broadcast against the parts): crossing | any(num_i <= H * H * den_i)."""
    crossing, num, den = parts
    hh = np.asarray(H, np.float64) * np.asarray(H, np.float64)
    return crossing | (num <= hh * den).any(axis=0)


def _rows(seg):
    seg = np.asarray(seg, np.float32)
    if seg.ndim == 3:
        seg = seg[:, None]
    assert seg.ndim == 4 and seg.shape[2:] == (2, 2), seg.shape
    return seg


def fold(mask, group=1, grouped=0):
    """(..., W) bool -> (...) int64: the first `grouped` walls count once per aligned group of `group` (a body fleet: the
    slots of one other robot), the rest one each."""
    mask = np.asarray(mask, bool)
    assert grouped % group == 0 and grouped <= mask.shape[-1]
    robots = mask[..., :grouped].reshape(mask.shape[:-1] + (grouped // group, group)).any(axis=-1)
    return robots.sum(axis=-1).astype(np.int64) + mask[..., grouped:].sum(axis=-1).astype(np.int64)


def level_masks(st, margins, tracks, radii, seg, hw, footprint=None, offset=0, wall_offset=None):
    """((M, n, T, K) bool, (M, n, T, W) bool): disc k / wall k is near at margin margins[l] (float64; 0.0: it is hit) in
    step t of states (n, T+1, 3).  tracks (K, L, 2) with radii (K,) -- static discs are tracks of one row; seg None: no walls,
    (W, 2, 2) static walls, (W, Lw, 2, 2) wall tracks -- step t meets row min(wall_offset + t, Lw - 1)."""
    st = np.asarray(st, np.float32)
    margins = np.asarray(margins, np.float64)
    tracks, radii = np.asarray(tracks, np.float32), np.asarray(radii, np.float32)
    assert tracks.ndim == 3 and tracks.shape[0] == len(radii) and tracks.shape[1] >= 1 and tracks.shape[2] == 2
    n, T = st.shape[0], st.shape[1] - 1
    K, L = tracks.shape[:2]
    if footprint is None:
        ctr = st[:, :, None, :2]  # (n, T+1, 1, 2): the one "body disc" is the reference point, and nothing is added
        rho = None
    else:
        ctr = footprint_model.centres(st, footprint)  # (n, T+1, F, 2)
        rho = footprint_model.rows_of(footprint)[:, 2].astype(np.float64)
    F = ctr.shape[2]

    def sizes(own):  # (M, F, count) float64: (own (+ rho_i)) + m, in this order
        base = own.astype(np.float64)[None, :] if rho is None else own.astype(np.float64)[None, :] + rho[:, None]
        return np.stack([base if m == 0.0 else base + m for m in margins]) * np.ones((1, F, 1))

    discs = np.zeros((len(margins), n, T, K), bool)
    R = sizes(radii)
    rr = R * R
    for t in range(T):
        row = min(offset + t + 1, L - 1)
        ex = (ctr[:, t + 1, :, None, 0] - tracks[None, None, :, row, 0]).astype(np.float64)  # float32 difference, widened
        ey = (ctr[:, t + 1, :, None, 1] - tracks[None, None, :, row, 1]).astype(np.float64)
        d2 = ex * ex + ey * ey  # (n, F, K)
        discs[:, :, t] = (~(d2[None] - rr[:, None] > 0.0)).any(axis=2)
    if seg is None or len(seg) == 0:
        return discs, np.zeros((len(margins), n, T, 0), bool)
    seg = _rows(seg)
    W, Lw = seg.shape[:2]
    hw = np.ascontiguousarray(np.broadcast_to(np.asarray(hw, np.float32), (W,)))
    H = sizes(hw)  # (M, F, W)
    woff = offset if wall_offset is None else wall_offset
    walls = np.zeros((len(margins), n, T, W), bool)
    for t in range(T):
        row = min(woff + t, Lw - 1)
        parts = wall_parts(ctr[:, t, :, None], ctr[:, t + 1, :, None], seg[None, None, :, row, 0], seg[None, None, :, row, 1])
        for l in range(len(margins)):
            walls[l, :, t] = wall_verdict(parts, H[l][None]).any(axis=1)
    return discs, walls


def level_counts(st, margins, tracks, radii, seg, hw, footprint=None, offset=0, wall_offset=None, group=1, grouped=0):
    """(M, n, T) int64: the obstacles near at each margin."""
    discs, walls = level_masks(st, margins, tracks, radii, seg, hw, footprint, offset, wall_offset)
    return discs.sum(axis=-1).astype(np.int64) + fold(walls, group, grouped)


def hit_counts(st, tracks, radii, seg, hw, footprint=None, offset=0, wall_offset=None, group=1, grouped=0):
    """(n, T) int64: the step's hits -- margin 0."""
    return level_counts(st, [0.0], tracks, radii, seg, hw, footprint, offset, wall_offset, group, grouped)[0]


def ring_counts(st, rings, tracks, radii, seg, hw, footprint=None, offset=0, wall_offset=None, group=1, grouped=0):
    """(R, n, T) int64: n_l(t), the obstacles near at ring l in step t (the hit ones among them)."""
    margins = rows_of(rings)[:, 0].astype(np.float64)
    return level_counts(st, margins, tracks, radii, seg, hw, footprint, offset, wall_offset, group, grouped)


def chain(p, hits, ring_counts, rings, st, noise, u, goal_rows=None):
    """wall_model.chain (goal_track_model.chain with goal_rows (T, 2)) with the rings' additions behind the hits':
    hits (n, T), ring_counts (R, n, T), states (n, T+1, 3) -> (n,) float32."""
    rg = rows_of(rings)
    noise = np.ascontiguousarray(noise, np.float32)
    u = np.ascontiguousarray(u, np.float32)
    n, T = noise.shape[:2]
    assert np.shape(ring_counts) == (len(rg), n, T) and np.shape(hits) == (n, T)
    if goal_rows is None:
        goals = np.broadcast_to(np.float32([p.xgoal[0], p.xgoal[1]]), (T, 2))
    else:
        goals = np.asarray(goal_rows, np.float32)
        assert goals.shape == (T, 2)
    gt2 = np.float64(np.float32(p.goal_tolerance) * np.float32(p.goal_tolerance))
    cost = np.zeros(n, np.float32)
    d2 = np.full(n, 1e9)
    done = np.zeros(n, bool)
    reached = np.zeros(n, bool)
    obs_cost = np.float64(np.float32(p.obs_cost))
    penalties = rg[:, 1].astype(np.float64)
    for t in range(T):
        x, y = st[:, t + 1, 0], st[:, t + 1, 1]
        dx, dy = (goals[t, 0] - x).astype(np.float64), (goals[t, 1] - y).astype(np.float64)
        nd2 = dx * dx + dy * dy
        c1 = (cost.astype(np.float64) + p.dist_weight * nd2).astype(np.float32)
        for k in range(int(hits[:, t].max()) if n else 0):
            c1 = np.where(k < hits[:, t], (c1.astype(np.float64) + obs_cost).astype(np.float32), c1)
        for l in range(len(rg)):
            for k in range(int(ring_counts[l][:, t].max()) if n else 0):
                c1 = np.where(k < ring_counts[l][:, t], (c1.astype(np.float64) + penalties[l]).astype(np.float32), c1)
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


def costs(p, rings, tracks, radii, seg, hw, noise, u, footprint=None, offset=0, wall_offset=None, group=1, grouped=0,
          goal_track=None):
    """(n,) float32: the chain on the hits and the ring counts of the oracle's own states."""
    st = wall_model.states(p, noise, u)
    hits = hit_counts(st, tracks, radii, seg, hw, footprint, offset, wall_offset, group, grouped)
    near = ring_counts(st, rings, tracks, radii, seg, hw, footprint, offset, wall_offset, group, grouped)
    rows = None if goal_track is None else goal_track_model.goal_rows(goal_track, st.shape[1] - 1, offset)
    return chain(p, hits, near, rings, st, noise, u, rows)


def smallest_disc_margin(st, rings, tracks, radii, footprint=None, offset=0):
    """The smallest |diff| of any disc test at any level (0: the hit) -- how far every verdict is from flipping."""
    st = np.asarray(st, np.float32)
    tracks, radii = np.asarray(tracks, np.float32), np.asarray(radii, np.float32)
    if len(radii) == 0:
        return np.inf
    margins = np.concatenate([[0.0], rows_of(rings)[:, 0].astype(np.float64)])
    if footprint is None:
        ctr, rho = st[:, :, None, :2], np.zeros(1)
    else:
        ctr, rho = footprint_model.centres(st, footprint), footprint_model.rows_of(footprint)[:, 2].astype(np.float64)
    base = radii.astype(np.float64)[None, :] + rho[:, None] if footprint is not None else radii.astype(np.float64)[None, :]
    R = np.stack([base if m == 0.0 else base + m for m in margins])
    rr = R * R
    T, L = st.shape[1] - 1, tracks.shape[1]
    least = np.inf
    for t in range(T):
        row = min(offset + t + 1, L - 1)
        ex = (ctr[:, t + 1, :, None, 0] - tracks[None, None, :, row, 0]).astype(np.float64)
        ey = (ctr[:, t + 1, :, None, 1] - tracks[None, None, :, row, 1]).astype(np.float64)
        least = min(least, np.abs((ex * ex + ey * ey)[None] - rr[:, None]).min())
    return least
