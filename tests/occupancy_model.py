"""Model of the barebone planner's occupancy-grid obstacles (numpy, CPU): params['occupancy'], as csrc/occupancy_grid.h,
occupancy_kernels.h and the grid forms of the crowd kernel compute them -- built on clearance_model's counts and chain,
footprint_model's centres and guide_model's field.

The clearance field D2 is uint32 (ny, nx): the least (ix - jx)^2 + (iy - jy)^2 over the occupied cells (jy, jx), 0xFFFFFFFF
everywhere when none is occupied -- here by brute force over the occupied cells; `field_separable` is the second formulation
(per row the distance to the nearest occupied cell of that row, then the column minimum).

A point robot is the body of one disc (0, 0, 0).  For body disc i, A and B are its float32 centres at the pre-step and the
post-step state; with M = substeps test point k = 1 .. M is float64(B) for k == M, else
float64(A) + (float64(k) / float64(M)) * (float64(B) - float64(A)) -- the product rounded, numpy never fuses.  The cell of a
point is q = floor((X - float64(origin)) / float64(res)) per axis, inside iff 0 <= q <= n - 1 on both (a NaN is outside).
The verdict at level l (0: the hit; l >= 1: ring l of margin m_l) is inside and D2[cell] <= thr[i][l],
thr = min(floor(R * R / (res * res)), 0xFFFFFFFE), R = (float64(inflate) + float64(rho_i)) + m_l.  The grid is ONE obstacle:
a step adds 1 to the count of every level at which any test point of any body disc gives the verdict."""
import numpy as np

import clearance_model
import footprint_model
import goal_track_model
import guide_model
import wall_model

FAR = np.uint32(0xFFFFFFFF)
THR_MAX = 0xFFFFFFFE
POINT = np.zeros((1, 3), np.float32)  # the point robot as a body


class Grid:
    """origin, resolution and inflate rounded once to float32; cells (ny, nx), non-zero = occupied."""

    def __init__(self, origin, resolution, cells, inflate=0.0, substeps=1):
        self.x_min, self.y_min = np.float32(origin[0]), np.float32(origin[1])
        self.res = np.float32(resolution)
        self.cells = np.asarray(cells) != 0
        assert self.cells.ndim == 2
        self.ny, self.nx = self.cells.shape
        self.inflate = np.float32(inflate)
        self.substeps = int(substeps)
        assert 1 <= self.substeps <= 8
        self._field = None

    @property
    def field(self):
        if self._field is None:
            self._field = field_of(self.cells)
            self._field.setflags(write=False)
        return self._field


def field_of(cells):
    """(ny, nx) uint32 by brute force over the occupied cells."""
    cells = np.asarray(cells) != 0
    ny, nx = cells.shape
    jy, jx = np.nonzero(cells)
    out = np.full((ny, nx), int(FAR), np.int64)
    iy, ix = np.arange(ny, dtype=np.int64)[:, None], np.arange(nx, dtype=np.int64)[None, :]
    for k0 in range(0, len(jy), 256):  # (in slices: 512 x 512 cells against a few thousand occupied ones)
        for y, x in zip(jy[k0:k0 + 256], jx[k0:k0 + 256]):
            np.minimum(out, (ix - x) ** 2 + (iy - y) ** 2, out=out)
    return out.astype(np.uint32)


def field_separable(cells):
    """The same field the other way: g(y', x), the distance along row y' to its nearest occupied cell (none: the row is
    empty), then D2[y][x] = min over y' of (y - y')^2 + g(y', x)^2."""
    cells = np.asarray(cells) != 0
    ny, nx = cells.shape
    none = 1 << 40
    g = np.full((ny, nx), none, np.int64)
    for y in range(ny):
        xs = np.nonzero(cells[y])[0]
        if len(xs):
            g[y] = np.abs(np.arange(nx)[:, None] - xs[None, :]).min(axis=1)
    out = np.full((ny, nx), int(FAR), np.int64)
    for y in range(ny):
        dy2 = (np.arange(ny, dtype=np.int64) - y)[:, None] ** 2
        cand = np.where(g < none, dy2 + g * g, int(FAR))
        out[y] = cand.min(axis=0)
    return out.astype(np.uint32)


def test_points(A, B, M):
    """(M, ...) float64: the test points k = 1 .. M of the chords A -> B (float32, any shape), one axis."""
    A, B = np.asarray(A, np.float32).astype(np.float64), np.asarray(B, np.float32).astype(np.float64)
    out = []
    for k in range(1, M + 1):
        if k == M:
            out.append(np.broadcast_to(B, np.broadcast(A, B).shape).copy())
        else:
            f = np.float64(k) / np.float64(M)
            out.append(A + f * (B - A))
    return np.stack(out)


def cell_of(X, lo, res, n):
    """(inside bool, cell int64 -- 0 where outside) of float64 points X along one axis of n cells."""
    X = np.asarray(X, np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        q = np.floor((X - np.float64(np.float32(lo))) / np.float64(np.float32(res)))
        inside = (q >= 0.0) & (q <= float(n - 1))
    return inside, np.where(inside, q, 0.0).astype(np.int64)


def threshold(inflate, rho, margin, res):
    """uint32 thresholds (broadcast over rho and margin, float64): min(floor(R * R / (res * res)), 0xFFFFFFFE)."""
    R = (np.float64(np.float32(inflate)) + np.asarray(rho, np.float64)) + np.asarray(margin, np.float64)
    r = np.float64(np.float32(res))
    with np.errstate(over="ignore"):
        v = np.floor((R * R) / (r * r))
    return np.minimum(v, float(THR_MAX)).astype(np.uint32)


def thresholds(grid, footprint, margins):
    """(F, len(margins)) uint32: thr[i][l] for the margins given (0.0: the hit)."""
    rho = footprint_model.rows_of(footprint)[:, 2].astype(np.float64)
    return np.stack([threshold(grid.inflate, rho, 0.0 if m == 0.0 else np.float64(m), grid.res) for m in margins], axis=1)


def point_levels(grid, X, Y, thr):
    """(L, ...) bool: the verdict of float64 points (X, Y) at the thresholds thr (L,) uint32 (broadcast against the points
    when it has more axes: (L, ...))."""
    in_x, ix = cell_of(X, grid.x_min, grid.res, grid.nx)
    in_y, iy = cell_of(Y, grid.y_min, grid.res, grid.ny)
    inside = in_x & in_y
    d2 = grid.field[iy, ix]
    thr = np.asarray(thr, np.uint32)
    thr = thr.reshape(thr.shape + (1,) * (d2.ndim - (thr.ndim - 1)))
    return inside[None] & (d2[None] <= thr)


def level_bits(grid, st, margins, footprint=None):
    """(len(margins), n, T) bool: the grid is touched at the level in step t of the float32 states (n, T+1, 3).
    Also returns (inside (n, T, F, M) bool) for the tests of the inputs."""
    st = np.asarray(st, np.float32)
    fp = POINT if footprint is None else footprint
    ctr = footprint_model.centres(st, fp)  # (n, T+1, F, 2); the point: the position itself
    thr = thresholds(grid, fp, margins)  # (F, L)
    M = grid.substeps
    X = test_points(ctr[:, :-1, :, 0], ctr[:, 1:, :, 0], M)  # (M, n, T, F)
    Y = test_points(ctr[:, :-1, :, 1], ctr[:, 1:, :, 1], M)
    in_x, ix = cell_of(X, grid.x_min, grid.res, grid.nx)
    in_y, iy = cell_of(Y, grid.y_min, grid.res, grid.ny)
    inside = in_x & in_y
    d2 = grid.field[iy, ix]  # (M, n, T, F)
    bits = inside[None] & (d2[None] <= thr.T[:, None, None, None, :])  # (L, M, n, T, F)
    return bits.any(axis=(1, 4)), np.moveaxis(inside, 0, -1)


def counts(grid, st, rings, tracks, radii, seg, hw, footprint=None, offset=0, wall_offset=None, group=1, grouped=0):
    """(hits (n, T), near (R, n, T)) int64: clearance_model's counts with the grid's bit added at every level."""
    margins = [0.0] + ([] if rings is None else [float(m) for m in clearance_model.rows_of(rings)[:, 0].astype(np.float64)])
    lv = clearance_model.level_counts(st, margins, tracks, radii, seg, hw, footprint, offset, wall_offset, group, grouped)
    lv = lv + level_bits(grid, st, margins, footprint)[0].astype(np.int64)
    return lv[0], lv[1:]


FREE_RING = np.float32([[1.0, 0.0]])  # the chain without rings: one ring that is never counted


def costs(p, grid, rings, tracks, radii, seg, hw, noise, u, footprint=None, offset=0, wall_offset=None, group=1, grouped=0,
          goal_track=None, goal_rows=None):
    """(n,) float32: clearance_model.chain on the counts with the grid's bits, over the oracle's own states."""
    st = wall_model.states(p, noise, u)
    hits, near = counts(grid, st, rings, tracks, radii, seg, hw, footprint, offset, wall_offset, group, grouped)
    rows = goal_rows
    if goal_track is not None:
        rows = goal_track_model.goal_rows(goal_track, st.shape[1] - 1, offset)
    if rings is None:
        return clearance_model.chain(p, hits, np.zeros((1,) + hits.shape, np.int64), FREE_RING, st, noise, u, rows)
    return clearance_model.chain(p, hits, near, rings, st, noise, u, rows)


def guide_blocked(guide, grid, segments=None, halfwidths=None):
    """(ny, nx) bool of the guide's grid: blocked by a wall (guide_model.blocked_cells) or by the occupancy grid -- the centre
    inside it on a cell with D2 <= thr_g, R = float64(inflate_occ) + float64(inflate_guide)."""
    out = np.zeros((guide.ny, guide.nx), bool)
    if segments is not None and len(segments):
        out |= guide_model.blocked_cells(guide, segments, halfwidths)
    cx = guide_model.centres(guide.x_min, guide.res, guide.nx)[None, :] + np.zeros((guide.ny, 1))
    cy = guide_model.centres(guide.y_min, guide.res, guide.ny)[:, None] + np.zeros((1, guide.nx))
    thr = threshold(grid.inflate, np.float64(guide.inflate), 0.0, grid.res)
    return out | point_levels(grid, cx, cy, np.asarray([thr]))[0]


def guide_field(guide, grid, goal, segments=None, halfwidths=None):
    return guide_model.field_of(guide_blocked(guide, grid, segments, halfwidths), guide_model.goal_cell(guide, goal))
