"""Model of the barebone planner's guide round the walls (numpy and heapq, CPU): blocked cells, the shortest-path field, the
descent and the rows of mppi_planner_set_guide, as csrc/guide_grid.h and guide_kernels.h compute them.

The grid: cell (iy, ix) has the centre cx = float64(x_min) + (ix + 0.5) * float64(res) (the product rounded, then the sum);
cell_of(x) = clamp(floor((float64(x) - float64(x_min)) / float64(res)), 0, n - 1).  A cell is blocked iff its centre is
within h_k + inflate of some wall k -- wall_model._near, the crowd kernel's crowd_near, with d = B - A, d.d and
hh = (float64(h) + float64(inflate))**2.  The field D is uint32: BLOCKED, UNREACHED, or the length of the shortest path to
the goal cell over free cells, 12 a straight move and 17 a diagonal one -- integers, so any relaxation order gives the same
bits; here Dijkstra.  The descent from the start cell takes the in-grid neighbour with D < UNREACHED that minimises
D[n] + w, the first minimum in the order NEIGHBOURS; R_i is the remaining length, and row j is the centre of the first
cell with R_0 - R_i >= lead_u + j * pace_u, or the goal itself where there is none or that cell is the goal's."""
import heapq

import numpy as np

import wall_model

BLOCKED = np.uint32(0xFFFFFFFF)
UNREACHED = np.uint32(0xFFFFFFFE)
NEIGHBOURS = ((1, 0), (0, 1), (-1, 0), (0, -1), (1, 1), (-1, 1), (-1, -1), (1, -1))
COSTS = (12, 12, 12, 12, 17, 17, 17, 17)
NO_MOVE = 255
CELLS_MAX = 36864
STATUS_OK, STATUS_GOAL_BLOCKED, STATUS_NO_WAY_OUT = 0, 1, 2


class Grid:
    """x_min, y_min, res, inflate rounded once to float32; shape (ny, nx)."""

    def __init__(self, origin, resolution, shape, inflate=None):
        self.x_min, self.y_min = np.float32(origin[0]), np.float32(origin[1])
        self.res = np.float32(resolution)
        self.ny, self.nx = int(shape[0]), int(shape[1])
        self.inflate = np.float32(resolution if inflate is None else inflate)


def centres(lo, res, n):
    """(n,) float64 cell centres along one axis."""
    return np.float64(np.float32(lo)) + (np.arange(n, dtype=np.float64) + 0.5) * np.float64(np.float32(res))


def cell_of(x, lo, res, n):
    """Cell indices of float32 coordinates x (any shape) along one axis, clamped into the grid."""
    x = np.asarray(x, np.float32).astype(np.float64)
    with np.errstate(over="ignore"):
        q = np.floor((x - np.float64(np.float32(lo))) / np.float64(np.float32(res)))
    return np.clip(q, 0.0, float(n - 1)).astype(np.int64)


def blocked_by(cx, cy, A, B, h, inflate):
    """Is the point (cx, cy) (float64, broadcast) within h + inflate of the wall A -> B (float32)?"""
    A, B = (np.asarray(v, np.float32).astype(np.float64) for v in (A, B))
    ax, ay = A[..., 0], A[..., 1]
    dx, dy = B[..., 0] - ax, B[..., 1] - ay
    H = np.asarray(h, np.float32).astype(np.float64) + np.float64(np.float32(inflate))
    return wall_model._near(cx - ax, cy - ay, dx, dy, dx * dx + dy * dy, H * H)


def blocked_cells(grid, segments, halfwidths):
    """(ny, nx) bool."""
    seg = np.asarray(segments, np.float32).reshape(-1, 2, 2)
    hw = np.broadcast_to(np.asarray(halfwidths, np.float32), (len(seg),))
    cx = centres(grid.x_min, grid.res, grid.nx)[None, :, None]
    cy = centres(grid.y_min, grid.res, grid.ny)[:, None, None]
    out = np.zeros((grid.ny, grid.nx), bool)
    for k0 in range(0, len(seg), 64):
        out |= blocked_by(cx, cy, seg[None, None, k0:k0 + 64, 0], seg[None, None, k0:k0 + 64, 1], hw[None, None, k0:k0 + 64],
                          grid.inflate).any(axis=2)
    return out


def goal_cell(grid, goal):
    goal = np.asarray(goal, np.float32)
    return int(cell_of(goal[1], grid.y_min, grid.res, grid.ny)), int(cell_of(goal[0], grid.x_min, grid.res, grid.nx))


def field_of(blocked, gcell):
    """(ny, nx) uint32 from the blocked cells and the goal cell (iy, ix): Dijkstra over the free cells."""
    ny, nx = blocked.shape
    D = np.where(blocked, BLOCKED, UNREACHED).astype(np.uint32)
    if blocked[gcell]:
        return D
    dist = {gcell: 0}
    heap = [(0, gcell)]
    while heap:
        d, (iy, ix) = heapq.heappop(heap)
        if d > dist[(iy, ix)]:
            continue
        for (dx, dy), w in zip(NEIGHBOURS, COSTS):
            jy, jx = iy + dy, ix + dx
            if 0 <= jy < ny and 0 <= jx < nx and not blocked[jy, jx] and d + w < dist.get((jy, jx), 1 << 62):
                dist[(jy, jx)] = d + w
                heapq.heappush(heap, (d + w, (jy, jx)))
    for (iy, ix), d in dist.items():
        D[iy, ix] = d
    return D


def field(grid, segments, halfwidths, goal):
    return field_of(blocked_cells(grid, segments, halfwidths), goal_cell(grid, goal))


def next_move(D, iy, ix):
    """(k, D[n] + w) of the neighbour a descent moves to from (iy, ix); (NO_MOVE, UNREACHED) without one."""
    ny, nx = D.shape
    best, move = int(UNREACHED), NO_MOVE
    for k, ((dx, dy), w) in enumerate(zip(NEIGHBOURS, COSTS)):
        jy, jx = iy + dy, ix + dx
        if 0 <= jy < ny and 0 <= jx < nx and D[jy, jx] < UNREACHED and int(D[jy, jx]) + w < best:
            best, move = int(D[jy, jx]) + w, k
    return move, best


def moves_of(D):
    """(ny, nx) uint8: next_move of every cell -- the table the field kernel stores beside the field."""
    return np.array([[next_move(D, iy, ix)[0] for ix in range(D.shape[1])] for iy in range(D.shape[0])], np.uint8).reshape(D.shape)


def units(m, res):
    return int(np.floor(np.float64(np.float32(m)) / np.float64(np.float32(res)) * 12.0))


def descent(D, c0, reach):
    """The cells c_i (iy, ix) and remaining lengths R_i from the start cell until R_i = 0 or R_0 - R_i >= reach.
    status 2 (and nothing): no admissible neighbour at a start cell that is blocked or unreached."""
    cells, R = [c0], []
    if D[c0] < UNREACHED:
        R.append(int(D[c0]))
    else:
        k, best = next_move(D, *c0)
        if k == NO_MOVE:
            return [], [], STATUS_NO_WAY_OUT
        R.append(best)
    while R[-1] != 0 and R[0] - R[-1] < reach and len(cells) <= D.size:
        k, best = next_move(D, *cells[-1])
        assert k != NO_MOVE
        cells.append((cells[-1][0] + NEIGHBOURS[k][1], cells[-1][1] + NEIGHBOURS[k][0]))
        R.append(int(D[cells[-1]]))
        assert R[-1] == best - COSTS[k] and R[-1] < R[-2], "the field is its own fixed point"
    return cells, R, STATUS_OK


def pick_rows(cells, R, count, lead_u, pace_u):
    """For j = 0 .. count - 1: the index i* of the first cell with R_0 - R_i >= lead_u + j * pace_u, or -1 (the goal: there
    is none, or R_i* = 0)."""
    out = []
    gains = [R[0] - r for r in R]
    for j in range(count):
        a = lead_u + j * pace_u
        i = next((i for i, g in enumerate(gains) if g >= a), None)
        out.append(-1 if i is None or R[i] == 0 else i)
    return out


def rows(grid, D, start, goal, T, lead, pace, parked=False):
    """((T + 1, 2) float32 rows, status, remaining (T + 1,) int64: the length still to go from each row's point)."""
    goal = np.asarray(goal, np.float32)[:2]
    out = np.tile(goal, (T + 1, 1)).astype(np.float32)
    left = np.zeros(T + 1, np.int64)
    if D[goal_cell(grid, goal)] == BLOCKED:
        return out, STATUS_GOAL_BLOCKED, left
    if parked:
        return out, STATUS_OK, left
    start = np.asarray(start, np.float32)
    c0 = int(cell_of(start[1], grid.y_min, grid.res, grid.ny)), int(cell_of(start[0], grid.x_min, grid.res, grid.nx))
    lead_u, pace_u = units(lead, grid.res), units(pace, grid.res)
    cells, R, status = descent(D, c0, lead_u + T * pace_u)
    if status != STATUS_OK:
        return out, status, left
    cx, cy = centres(grid.x_min, grid.res, grid.nx), centres(grid.y_min, grid.res, grid.ny)
    for j, i in enumerate(pick_rows(cells, R, T + 1, lead_u, pace_u)):
        if i >= 0:
            out[j] = (np.float32(cx[cells[i][1]]), np.float32(cy[cells[i][0]]))
            left[j] = R[i]
    return out, status, left


def guide(grid, segments, halfwidths, start, goal, T, lead, pace):
    """Field, rows and status of one problem."""
    D = field(grid, segments, halfwidths, goal)
    r, status, _ = rows(grid, D, start, goal, T, lead, pace)
    return D, r, status
