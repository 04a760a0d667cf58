"""Model of the barebone planner's body footprint (numpy, CPU): params['footprint'], built on the existing models only --
crowd_model.hit_counts' disc arithmetic, wall_model.hit's and wall_model.chain, disc_samples_model's tail.

A footprint is (F, 3) float32, rows (ox, oy, rho): a body disc's centre in the robot frame (x along the heading, y to the
left) and its radius.  At a float32 state (x, y, th), with s, c the float64 sine and cosine of (double)th,

    cx = (float)((double)x + ((double)ox * c - (double)oy * s))
    cy = (float)((double)y + ((double)ox * s + (double)oy * c))

products and sums in double in the order written, one rounding.  Body disc i touches disc k at step t iff crowd_model's test
says so with the centre at the post-step state in place of the position and rr = R * R, R = (double)r_k + (double)rho_i; the
body touches disc k iff ANY of its discs does, and the step's disc hits are the number of discs touched.  During step t body
disc i moves from its centre at the pre-step state (step 0: x0, heading included) to its centre at the post-step state, and
wall_model.hit is applied to that segment with hh = H * H, H = (double)h_k + (double)rho_i; the body hits wall k iff any of
its discs does.  Everything else -- the goal distance, the freeze, the chain -- is the reference point's: wall_model.chain on
the counts."""
import numpy as np

import disc_samples_model
import goal_track_model
import wall_model


def rows_of(footprint):
    fp = np.asarray(footprint, np.float64).astype(np.float32)
    assert fp.ndim == 2 and fp.shape[1] == 3 and 1 <= len(fp) <= 8, fp.shape
    return fp


def centres(st, footprint, ds=0.0, dc=0.0):
    """(..., F, 2) float32: the body discs' centres at float32 states (..., 3).  ds, dc: added to the sine and the cosine
    (the robustness test moves them by what a device's sincos may differ from libm's)."""
    st = np.asarray(st, np.float32)
    fp = rows_of(footprint).astype(np.float64)
    x, y, th = (st[..., i, None].astype(np.float64) for i in range(3))
    s, c = np.sin(th) + ds, np.cos(th) + dc
    cx = x + (fp[:, 0] * c - fp[:, 1] * s)
    cy = y + (fp[:, 0] * s + fp[:, 1] * c)
    return np.stack([cx, cy], axis=-1).astype(np.float32)


def hit(P, Q, A, B, h, rho):
    """wall_model.hit, statement for statement, with hh = (h + rho)^2, the sum in double (wall_model.hit squares a float32
    half-width, and h + rho need not be one): P, Q the chord of a body disc of radius rho (float32)."""
    P, Q, A, B = (np.asarray(v, np.float32).astype(np.float64) for v in (P, Q, A, B))
    H = np.asarray(h, np.float32).astype(np.float64) + np.asarray(rho, np.float32).astype(np.float64)
    px, py, qx, qy = P[..., 0], P[..., 1], Q[..., 0], Q[..., 1]
    ax, ay, bx, by = A[..., 0], A[..., 1], B[..., 0], B[..., 1]
    dx, dy = bx - ax, by - ay
    ex, ey = qx - px, qy - py
    hh, LLd, LLe = H * H, dx * dx + dy * dy, ex * ex + ey * ey
    pax, pay, qax, qay = px - ax, py - ay, qx - ax, qy - ay
    apx, apy, bpx, bpy = ax - px, ay - py, bx - px, by - py
    o1, o2 = dx * pay - dy * pax, dx * qay - dy * qax
    o3, o4 = ex * apy - ey * apx, ex * bpy - ey * bpx
    crossing = (((o1 > 0) & (o2 < 0)) | ((o1 < 0) & (o2 > 0))) & (((o3 > 0) & (o4 < 0)) | ((o3 < 0) & (o4 > 0)))
    near = wall_model._near
    return (crossing | near(pax, pay, dx, dy, LLd, hh) | near(qax, qay, dx, dy, LLd, hh) |
            near(apx, apy, ex, ey, LLe, hh) | near(bpx, bpy, ex, ey, LLe, hh))


def disc_touches(ctr, footprint, tracks, radii, offset=0):
    """(n, T, F, K) bool: body disc i touches disc k at step t.  ctr (n, T+1, F, 2) centres, tracks (K, L, 2)."""
    fp = rows_of(footprint)
    tracks = np.asarray(tracks, np.float32)
    radii = np.asarray(radii, np.float32)
    assert tracks.ndim == 3 and tracks.shape[0] == len(radii) and tracks.shape[1] >= 1 and tracks.shape[2] == 2
    n, T, F = ctr.shape[0], ctr.shape[1] - 1, len(fp)
    K, L = tracks.shape[:2]
    R = radii.astype(np.float64)[None, :] + fp[:, 2].astype(np.float64)[:, None]  # (F, K)
    rr = R * R
    out = np.zeros((n, T, F, K), bool)
    for t in range(T):
        row = min(offset + t + 1, L - 1)
        ex = (ctr[:, t + 1, :, None, 0] - tracks[None, None, :, row, 0]).astype(np.float64)  # float32 difference, widened
        ey = (ctr[:, t + 1, :, None, 1] - tracks[None, None, :, row, 1]).astype(np.float64)
        diff = ex * ex + ey * ey - rr[None]
        out[:, t] = ~(diff > 0.0)
    return out


def wall_touches(ctr, footprint, seg, hw, offset=0):
    """(n, T, F, W) bool: the chord of body disc i during step t hits wall k.  seg: static walls (W, 2, 2) or wall tracks
    (W, Lw, 2, 2) -- step t meets row min(offset + t, Lw - 1)."""
    fp = rows_of(footprint)
    seg = np.asarray(seg, np.float32)
    if seg.ndim == 3:
        seg = seg[:, None]
    assert seg.ndim == 4 and seg.shape[2:] == (2, 2), seg.shape
    W, Lw = seg.shape[:2]
    hw = np.ascontiguousarray(np.broadcast_to(np.asarray(hw, np.float32), (W,)))
    n, T, F = ctr.shape[0], ctr.shape[1] - 1, len(fp)
    out = np.zeros((n, T, F, W), bool)
    for t in range(T):
        row = min(offset + t, Lw - 1)
        out[:, t] = hit(ctr[:, t, :, None], ctr[:, t + 1, :, None], seg[None, None, :, row, 0], seg[None, None, :, row, 1],
                        hw[None, None, :], fp[None, :, None, 2])
    return out


def footprint_hits(st, footprint, tracks, radii, seg=None, hw=None, offset=0, wall_offset=None, ds=0.0, dc=0.0):
    """((n, T) int64 disc hits, (n, T) int64 wall hits) of states (n, T+1, 3): obstacles touched, the "any" rule over the
    body's discs.  tracks (K, L, 2) with radii (K,) -- static discs are tracks of one row; seg None: no walls."""
    ctr = centres(st, footprint, ds, dc)
    discs = disc_touches(ctr, footprint, tracks, radii, offset).any(axis=2).sum(axis=2).astype(np.int64)
    walls = np.zeros_like(discs)
    if seg is not None and len(seg):
        walls = wall_touches(ctr, footprint, seg, hw, offset if wall_offset is None else wall_offset).any(axis=2).sum(axis=2).astype(np.int64)
    return discs, walls


def costs(p, footprint, tracks, radii, seg, hw, noise, u, offset=0, goal_track=None, wall_offset=None):
    """(n,) float32: wall_model.chain (goal_track_model.chain with a goal track) on the body's disc hits + wall hits."""
    st = wall_model.states(p, noise, u)
    discs, walls = footprint_hits(st, footprint, tracks, radii, seg, hw, offset, wall_offset)
    if goal_track is None:
        return wall_model.chain(p, discs + walls, st, noise, u)
    return goal_track_model.chain(p, discs + walls, st, noise, u, goal_track_model.goal_rows(goal_track, st.shape[1] - 1, offset))


def sample_costs(p, footprint, samples, radii, seg, hw, noise, u, offset=0):
    """(n, S) float32: the cost under every disc sample (S, K, L, 2) -- the body against that sample's discs, the walls
    counted once."""
    st = wall_model.states(p, noise, u)
    samples = np.asarray(samples, np.float32)
    walls = footprint_hits(st, footprint, samples[0], radii, seg, hw, offset)[1]
    out = [wall_model.chain(p, footprint_hits(st, footprint, samples[s], radii, None, None, offset)[0] + walls, st, noise, u)
           for s in range(len(samples))]
    return np.stack(out, axis=1)


def sampled_costs(p, footprint, samples, radii, seg, hw, noise, u, alpha, offset=0):
    return disc_samples_model.cvar_tail(sample_costs(p, footprint, samples, radii, seg, hw, noise, u, offset), alpha)


def rectangle_clearance(states, front, rear, width, seg):
    """Float64 geometry, for the closed loop's check: the smallest distance between the rectangle [-rear, front] x
    [-width/2, width/2] at each of the states (m, 3) and the wall segments (W, 2, 2) -- negative when a wall crosses an
    edge of the rectangle or ends inside it (then minus a depth).  Per state: (m,)."""
    st = np.asarray(states, np.float64)
    seg = np.asarray(seg, np.float64).reshape(-1, 2, 2)
    corners = np.array([[front, width / 2], [-rear, width / 2], [-rear, -width / 2], [front, -width / 2]], np.float64)
    c, s = np.cos(st[:, 2]), np.sin(st[:, 2])
    R = np.stack([np.stack([c, -s], -1), np.stack([s, c], -1)], -2)  # (m, 2, 2)
    world = st[:, None, :2] + np.einsum("mij,kj->mki", R, corners)  # (m, 4, 2)
    out = np.full(len(st), np.inf)

    def seg_seg(p1, q1, p2, q2):  # distance between two segments (broadcast); when they cross: minus the nearest endpoint's
        def pt_seg(x, a, b):
            d = b - a
            LL = (d * d).sum(-1)
            tt = np.clip(((x - a) * d).sum(-1) / np.where(LL > 0, LL, 1.0), 0.0, 1.0)
            return np.linalg.norm(x - (a + tt[..., None] * d), axis=-1)

        def orient(a, b, x):
            return (b[..., 0] - a[..., 0]) * (x[..., 1] - a[..., 1]) - (b[..., 1] - a[..., 1]) * (x[..., 0] - a[..., 0])
        cross = (orient(p1, q1, p2) * orient(p1, q1, q2) < 0) & (orient(p2, q2, p1) * orient(p2, q2, q1) < 0)
        d = np.minimum(np.minimum(pt_seg(p1, p2, q2), pt_seg(q1, p2, q2)), np.minimum(pt_seg(p2, p1, q1), pt_seg(q2, p1, q1)))
        return np.where(cross, -d, d)

    for e in range(4):
        a, b = world[:, e, None], world[:, (e + 1) % 4, None]  # (m, 1, 2)
        out = np.minimum(out, seg_seg(a, b, seg[None, :, 0], seg[None, :, 1]).min(axis=1))
    # a wall endpoint inside the rectangle (no edge crossed: a wall wholly inside): negative depth
    for k in range(len(seg)):
        for end in range(2):
            local = np.einsum("mji,mj->mi", R, seg[k, end][None] - st[:, :2])  # R^T (x - pos)
            depth = np.minimum(np.minimum(front - local[:, 0], local[:, 0] + rear), np.minimum(width / 2 - local[:, 1], local[:, 1] + width / 2))
            out = np.where(depth > 0, np.minimum(out, -depth), out)
    return out
