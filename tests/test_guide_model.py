"""The guide round the walls on the host: the numpy and heapq model (tests/guide_model.py) against a brute-force
Bellman-Ford, against the wall test of the rollouts (no move between free neighbouring centres touches a wall), against its
own edge cases, and against csrc/guide_grid.h compiled with g++ on its own -- the arithmetic the kernels call -- bit for bit."""
import os
import re
import subprocess

import numpy as np
import pytest

import guide_model as model
import wall_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "mppi_numba_amd", "csrc", "guide_grid.h")


def random_walls(rng, grid, count):
    lo = np.array([grid.x_min, grid.y_min], np.float64)
    size = np.array([grid.nx, grid.ny], np.float64) * float(grid.res)
    A = lo + rng.uniform(-0.1, 1.1, (count, 2)) * size
    B = A + rng.normal(0, 0.35, (count, 2)) * size
    seg = np.stack([A, B], axis=1).astype(np.float32)
    return seg, rng.uniform(0, 0.6 * float(grid.res), count).astype(np.float32)


def bellman_ford(blocked, gcell):
    ny, nx = blocked.shape
    D = np.where(blocked, model.BLOCKED, model.UNREACHED).astype(np.uint32)
    if blocked[gcell]:
        return D
    D[gcell] = 0
    for _ in range(ny * nx + 1):
        changed = False
        for iy in range(ny):
            for ix in range(nx):
                if D[iy, ix] == model.BLOCKED:
                    continue
                _, best = model.next_move(D, iy, ix)
                if best < D[iy, ix]:
                    D[iy, ix] = best
                    changed = True
        if not changed:
            return D
    raise AssertionError("no fixed point within nx * ny sweeps")


# ---------------------------------------------------------------------- (a) the field
def test_the_field_is_its_own_fixed_point_and_equals_bellman_ford():
    rng = np.random.default_rng(0)
    reached = 0
    for trial in range(60):
        ny, nx = int(rng.integers(1, 8)), int(rng.integers(1, 10))
        blocked = rng.uniform(0, 1, (ny, nx)) < rng.uniform(0, 0.5)
        gcell = (int(rng.integers(0, ny)), int(rng.integers(0, nx)))
        D = model.field_of(blocked, gcell)
        assert (D == bellman_ford(blocked, gcell)).all(), (trial, blocked, gcell)
        assert ((D == model.BLOCKED) == blocked).all()
        for iy in range(ny):
            for ix in range(nx):
                if D[iy, ix] < model.UNREACHED and (iy, ix) != gcell:
                    assert model.next_move(D, iy, ix)[1] == D[iy, ix]  # the least D[n] + w over the neighbours is D[c]
                    reached += 1
                elif D[iy, ix] == model.UNREACHED:
                    assert model.next_move(D, iy, ix)[0] == model.NO_MOVE
    assert reached > 500


def test_the_descent_ends_at_the_goal_cell_from_every_reached_cell():
    rng = np.random.default_rng(1)
    grid = model.Grid((-1.0, 2.0), 0.25, (7, 9), 0.25 * 0.7072)
    seg, hw = random_walls(rng, grid, 4)
    goal = (0.3, 2.9)
    D = model.field(grid, seg, hw, goal)
    assert (D < model.UNREACHED).sum() > 10
    for iy in range(grid.ny):
        for ix in range(grid.nx):
            if D[iy, ix] < model.UNREACHED:
                cells, R, status = model.descent(D, (iy, ix), 1 << 40)
                assert status == 0 and R[-1] == 0 and cells[-1] == model.goal_cell(grid, goal) and R[0] == D[iy, ix]


# ---------------------------------------------------------------------- (b) no move touches a wall
def test_no_move_between_free_neighbouring_centres_touches_a_wall():
    rng = np.random.default_rng(2)
    moves = 0
    for trial in range(30):
        res = float(rng.uniform(0.05, 0.5))
        grid = model.Grid(rng.uniform(-3, 3, 2), res, (int(rng.integers(8, 20)), int(rng.integers(8, 20))), np.float32(res) * np.float32(0.7072))
        assert 2.0 * np.float64(grid.inflate) ** 2 >= np.float64(grid.res) ** 2
        seg, hw = random_walls(rng, grid, int(rng.integers(1, 7)))
        free = ~model.blocked_cells(grid, seg, hw)
        cx = model.centres(grid.x_min, grid.res, grid.nx).astype(np.float32)
        cy = model.centres(grid.y_min, grid.res, grid.ny).astype(np.float32)
        for dx, dy in model.NEIGHBOURS[:1] + model.NEIGHBOURS[1:2] + model.NEIGHBOURS[4:6]:  # (the other four are these reversed)
            ys, xs = np.nonzero(free)
            ok = (ys + dy >= 0) & (ys + dy < grid.ny) & (xs + dx >= 0) & (xs + dx < grid.nx)
            ys, xs = ys[ok], xs[ok]
            ok = free[ys + dy, xs + dx]
            ys, xs = ys[ok], xs[ok]
            P = np.stack([cx[xs], cy[ys]], axis=1)
            Q = np.stack([cx[xs + dx], cy[ys + dy]], axis=1)
            for way in ((P, Q), (Q, P)):
                hits = wall_model.hit(way[0][:, None], way[1][:, None], seg[None, :, 0], seg[None, :, 1], hw[None])
                assert not hits.any(), (trial, dx, dy)
            moves += 2 * len(P)
    assert moves > 10000


# ---------------------------------------------------------------------- (c) edge cases
ROOM = np.array([[[1.0, 0.0], [1.0, 1.5]]], np.float32)  # one wall across the lower part of a 2 x 2 room


def room_grid(shape=(8, 8)):
    return model.Grid((0.0, 0.0), 0.25, shape, 0.25)


@pytest.mark.parametrize("shape", [(1, 1), (1, 7), (7, 1)])
def test_degenerate_grids(shape):
    grid = model.Grid((0.0, 0.0), 0.5, shape, 0.5)
    goal = (0.5 * shape[1] - 0.1, 0.5 * shape[0] - 0.1)
    D, rows, status = model.guide(grid, np.zeros((0, 2, 2), np.float32), np.zeros(0, np.float32), (0.1, 0.1, 0.0), goal, 5, 0.5, 0.5)
    assert status == 0 and D.shape == shape and D.max() == 12 * (max(shape) - 1) and D[model.goal_cell(grid, goal)] == 0
    assert (rows[-1] == np.asarray(goal, np.float32)).all()
    if max(shape) > 1:
        assert (rows[0] != np.asarray(goal, np.float32)).any()


def test_goal_or_start_outside_the_grid_belong_to_the_border_cell():
    grid = room_grid()
    assert model.goal_cell(grid, (9.0, -4.0)) == (0, 7) and model.goal_cell(grid, (-1e30, 1e30)) == (7, 0)
    D = model.field(grid, ROOM, [0.0], (9.0, -4.0))
    assert D[0, 7] == 0
    rows, status, left = model.rows(grid, D, (-5.0, 0.1, 0.0), (9.0, -4.0), 6, 0.25, 0.25)
    assert status == 0 and left[0] == D[0, 0] - 12


def test_goal_in_a_blocked_cell_is_status_1_and_every_row_is_the_goal():
    grid = room_grid()
    D, rows, status = model.guide(grid, ROOM, [0.0], (0.1, 0.1, 0.0), (1.0, 0.6), 4, 0.25, 0.25)
    assert status == 1 and (D >= model.UNREACHED).all() and (D == model.UNREACHED).any()
    assert (rows == np.float32([1.0, 0.6])).all()


def test_start_in_a_sealed_pocket_is_status_2():
    grid = model.Grid((0.0, 0.0), 0.25, (12, 12), 0.25)
    box = np.array([[[0.5, 0.5], [1.5, 0.5]], [[1.5, 0.5], [1.5, 1.5]], [[1.5, 1.5], [0.5, 1.5]], [[0.5, 1.5], [0.5, 0.5]]], np.float32)
    D, rows, status = model.guide(grid, box, [0.0], (1.0, 1.0, 0.0), (2.6, 2.6), 4, 0.25, 0.25)
    assert D[4, 4] == model.UNREACHED and status == 2 and (rows == np.float32([2.6, 2.6])).all()


def test_start_inside_the_inflated_band_walks_out_the_cheapest_way():
    grid = room_grid()
    goal = (1.9, 0.1)
    D = model.field(grid, ROOM, [0.0], goal)
    start = (0.8, 0.6, 0.0)  # cell (2, 3): its centre 0.125 from the wall
    c0 = (2, 3)
    assert D[c0] == model.BLOCKED
    cells, R, status = model.descent(D, c0, 1 << 40)
    k, best = model.next_move(D, *c0)
    assert status == 0 and R[0] == best and R[1] == D[cells[1]] == best - model.COSTS[k] and R[-1] == 0
    rows, status, left = model.rows(grid, D, start, goal, 8, 0.0, 0.25)
    assert status == 0 and left[0] == R[0] and (np.diff(left) <= 0).all()


def test_lead_and_pace_zero_every_row_is_the_start_cell():
    grid = room_grid()
    D = model.field(grid, ROOM, [0.0], (1.9, 0.1))
    rows, status, _ = model.rows(grid, D, (0.1, 0.1, 0.0), (1.9, 0.1), 5, 0.0, 0.0)
    assert status == 0 and (rows == np.float32([0.125, 0.125])).all()
    rows, status, _ = model.rows(grid, D, (1.9, 0.1, 0.0), (1.9, 0.1), 5, 0.0, 0.0)  # in the goal's cell: the goal itself
    assert status == 0 and (rows == np.float32([1.9, 0.1])).all()


def test_a_short_path_ends_in_the_goal_exactly_and_rows_never_move_away():
    grid = room_grid()
    goal = (1.9, 0.1)
    D = model.field(grid, ROOM, [0.0], goal)
    rows, status, left = model.rows(grid, D, (0.1, 0.1, 0.0), goal, 40, 0.5, 0.25)
    assert status == 0 and (np.diff(left) <= 0).all() and left[0] > 0
    tail = left == 0
    assert tail[-10:].all() and (rows[tail] == np.asarray(goal, np.float32)).all() and (rows[~tail] != np.asarray(goal, np.float32)).any(axis=1).all()
    # the path goes round the wall's upper end: it is longer than the straight line
    assert D[0, 0] > 12 * 7 and model.units(0.5, grid.res) == 24 and model.units(0.3, 0.25) == 14


# ---------------------------------------------------------------------- (d) guide_grid.h against the model
PROGRAM = r"""
#include <cstdio>
#include <cstring>
#include <cstdint>
#include <vector>
#include "%s"
using namespace mppi;
template <typename T> static bool get(T* v, size_t n) { return std::fread(v, sizeof(T), n, stdin) == n; }
template <typename T> static void put(const T* v, size_t n) { std::fwrite(v, sizeof(T), n, stdout); }
int main() {
  int32_t op;
  while (get(&op, 1)) {
    int32_t n;
    if (!get(&n, 1)) return 1;
    if (op == 0) {  // centres and cells: n times (lo, res, x, i, cells) -> (centre, cell_of)
      for (int i = 0; i < n; ++i) {
        float f[3]; int32_t k[2];
        if (!get(f, 3) || !get(k, 2)) return 1;
        const double c = guide_centre(f[0], f[1], k[0]);
        const int64_t cell = guide_cell_of(f[2], f[0], f[1], k[1]);
        put(&c, 1); put(&cell, 1);
      }
    } else if (op == 1) {  // the block test: n times (cx, cy doubles; ax, ay, bx, by, h, inflate floats) -> byte
      for (int i = 0; i < n; ++i) {
        double c[2]; float f[6];
        if (!get(c, 2) || !get(f, 6)) return 1;
        const uint8_t hit = guide_blocked(c[0], c[1], guide_wall(f[0], f[1], f[2], f[3], f[4], f[5]));
        put(&hit, 1);
      }
    } else if (op == 2) {  // units: n times (m, res) -> double
      for (int i = 0; i < n; ++i) {
        float f[2];
        if (!get(f, 2)) return 1;
        const double u = guide_units(f[0], f[1]);
        put(&u, 1);
      }
    } else if (op == 3) {  // the neighbour choice: a field of n = ny rows, nx columns -> per cell (move, best)
      int32_t nx;
      if (!get(&nx, 1)) return 1;
      std::vector<uint32_t> D((size_t)n * nx);
      if (!get(D.data(), D.size())) return 1;
      for (int iy = 0; iy < n; ++iy)
        for (int ix = 0; ix < nx; ++ix) {
          uint32_t out[2];
          out[0] = (uint32_t)guide_next(D.data(), nx, n, ix, iy, &out[1]);
          put(out, 2);
        }
    } else if (op == 4) {  // the row choice: R[0 .. n), then m values a -> m indices
      std::vector<uint32_t> R((size_t)n);
      int32_t m;
      if (!get(R.data(), R.size()) || !get(&m, 1)) return 1;
      for (int j = 0; j < m; ++j) {
        int64_t a;
        if (!get(&a, 1)) return 1;
        const int32_t i = guide_first_reach(R.data(), n, R[0], (long long)a);
        put(&i, 1);
      }
    } else if (op == 5) {  // the moves and their costs
      for (int k = 0; k < 8; ++k) {
        const int32_t out[3] = {guide_dx(k), guide_dy(k), (int32_t)guide_move_cost(k)};
        put(out, 3);
      }
    }
  }
  return 0;
}
"""


@pytest.fixture(scope="module")
def header(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("guide_grid")
    src = tmp / "guide.cpp"
    src.write_text(PROGRAM % os.path.abspath(HEADER))
    exe = tmp / "guide"
    # -O2 with fused multiply-add available to the compiler: the header must not let it contract a product into a sum
    flags = ["-O2", "-ffp-contract=fast"] + (["-mfma"] if os.uname().machine in ("x86_64", "AMD64") else [])
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror"] + flags + ["-o", str(exe), str(src)])

    def run(request):
        return subprocess.run([str(exe)], input=request, stdout=subprocess.PIPE, check=True).stdout
    return run


def i32(*values):
    return np.asarray(values, np.int32).tobytes()


def test_the_header_forms_centres_and_cells_as_the_model_does(header):
    rng = np.random.default_rng(3)
    n = 20000
    lo = rng.uniform(-50, 50, n).astype(np.float32)
    res = rng.uniform(0.01, 2.0, n).astype(np.float32)
    cells = rng.integers(1, 193, n).astype(np.int32)
    i = (rng.integers(0, 192, n) % cells).astype(np.int32)
    x = (lo + rng.uniform(-0.2, 1.2, n) * cells * res).astype(np.float32)
    # on a cell's edge, where the quotient's rounding decides; far outside; res tiny and huge
    x[:4000] = (lo[:4000].astype(np.float64) + res[:4000].astype(np.float64) * rng.integers(0, 193, 4000)).astype(np.float32)
    x[4000:4008] = [1e30, -1e30, 3e38, -3e38, 0.0, -0.0, 1e-45, -1e-45]
    res[4008:4012] = [1e-30, 1e30, 2.0 ** -149, 3e38]
    want_c = np.array([model.centres(lo[k], res[k], i[k] + 1)[i[k]] for k in range(n)])
    want_cell = np.array([model.cell_of(x[k], lo[k], res[k], cells[k]) for k in range(n)], np.int64)
    body = b"".join(np.asarray([lo[k], res[k], x[k]], np.float32).tobytes() + i32(i[k], cells[k]) for k in range(n))
    out = np.frombuffer(header(i32(0, n) + body), dtype=np.uint8).reshape(n, 16)
    got_c = out[:, :8].copy().view(np.float64).ravel()
    got_cell = out[:, 8:].copy().view(np.int64).ravel()
    assert (got_c.view(np.uint64) == want_c.view(np.uint64)).all()
    assert (got_cell == want_cell).all()
    assert (want_cell == 0).sum() > 100 and (want_cell == cells - 1).sum() > 100
    # ... and a fused centre would not have passed everywhere
    import math
    fused = np.array([math.fma(float(i[k]) + 0.5, float(res[k]), float(lo[k])) for k in range(2000)]) if hasattr(math, "fma") else None
    if fused is not None:
        assert (fused.view(np.uint64) != want_c[:2000].view(np.uint64)).any()


def test_the_header_blocks_the_cells_the_model_blocks(header):
    rng = np.random.default_rng(4)
    n = 40000
    c = rng.uniform(-2, 2, (n, 2))
    A = rng.uniform(-2, 2, (n, 2)).astype(np.float32)
    B = (A + rng.normal(0, 1, (n, 2))).astype(np.float32)
    h = rng.uniform(0, 0.3, n).astype(np.float32)
    inflate = rng.uniform(0, 0.3, n).astype(np.float32)
    B[:500] = A[:500]  # degenerate walls
    # points at the half-width exactly (to rounding), beside the segment and beyond its ends
    d = (B.astype(np.float64) - A.astype(np.float64))[1000:20000]
    length = np.maximum(np.hypot(d[:, 0], d[:, 1]), 1e-9)
    normal = np.stack([-d[:, 1], d[:, 0]], axis=1) / length[:, None]
    along = rng.uniform(-0.3, 1.3, len(d))[:, None]
    H = (h.astype(np.float64) + inflate.astype(np.float64))[1000:20000, None]
    c[1000:20000] = A[1000:20000] + along * d + normal * H * rng.choice([-1.0, 1.0], len(d))[:, None]
    want = model.blocked_by(c[:, 0], c[:, 1], A, B, h, inflate)
    body = b"".join(c[k].tobytes() + np.asarray([A[k, 0], A[k, 1], B[k, 0], B[k, 1], h[k], inflate[k]], np.float32).tobytes()
                    for k in range(n))
    got = np.frombuffer(header(i32(1, n) + body), dtype=np.uint8).astype(bool)
    assert (got == want).all(), np.nonzero(got != want)[0][:5]
    assert want[1000:20000].sum() > 4000 and (~want[1000:20000]).sum() > 4000


def test_the_header_forms_units_as_the_model_does(header):
    rng = np.random.default_rng(5)
    m = rng.uniform(0, 30, 5000).astype(np.float32)
    res = rng.uniform(0.01, 1.0, 5000).astype(np.float32)
    m[:1000] = (res[:1000].astype(np.float64) * rng.integers(0, 50, 1000) / 12.0).astype(np.float32)  # next to whole units
    m[1000:1003] = [0.0, 1e30, 3e38]
    body = np.stack([m, res], axis=1).astype(np.float32).tobytes()
    got = np.frombuffer(header(i32(2, 5000) + body), dtype=np.float64)
    want = np.floor(m.astype(np.float64) / res.astype(np.float64) * 12.0)
    assert (got == want).all()
    assert [model.units(a, b) for a, b in zip(m[:50], res[:50])] == [int(v) for v in want[:50]]


def test_the_header_chooses_neighbours_and_rows_as_the_model_does(header):
    rng = np.random.default_rng(6)
    moves = np.frombuffer(header(i32(5, 0)), dtype=np.int32).reshape(8, 3)
    assert [tuple(r[:2]) for r in moves] == list(model.NEIGHBOURS) and list(moves[:, 2]) == list(model.COSTS)
    for trial in range(40):
        ny, nx = int(rng.integers(1, 12)), int(rng.integers(1, 12))
        if trial % 2:  # a real field ...
            blocked = rng.uniform(0, 1, (ny, nx)) < 0.3
            D = model.field_of(blocked, (int(rng.integers(0, ny)), int(rng.integers(0, nx))))
        else:  # ... and arbitrary values, ties included
            D = rng.integers(0, 40, (ny, nx)).astype(np.uint32)
            D[rng.uniform(0, 1, (ny, nx)) < 0.2] = model.BLOCKED
            D[rng.uniform(0, 1, (ny, nx)) < 0.2] = model.UNREACHED
        out = np.frombuffer(header(i32(3, ny, nx) + np.ascontiguousarray(D).tobytes()), dtype=np.uint32).reshape(ny, nx, 2)
        want = np.array([[model.next_move(D, iy, ix) for ix in range(nx)] for iy in range(ny)], np.int64).reshape(ny, nx, 2)
        assert (out == want).all(), trial
        assert (out[..., 0].astype(np.uint8) == model.moves_of(D)).all()
    for trial in range(40):
        n = int(rng.integers(1, 300))
        R = np.sort(rng.choice(5000, n, replace=False))[::-1].astype(np.uint32)
        if trial % 3 == 0:
            R[-1] = 0
        a = np.concatenate([rng.integers(0, 6000, 50), [0, int(R[0]), int(R[0]) + 1, 1 << 40]]).astype(np.int64)
        out = np.frombuffer(header(i32(4, n) + R.tobytes() + i32(len(a)) + a.tobytes()), dtype=np.int32)
        gains = int(R[0]) - R.astype(np.int64)
        want = [next((i for i in range(n) if gains[i] >= v), n) for v in a]
        assert list(out) == want
        cells = [(0, i) for i in range(n)]
        picked = model.pick_rows(cells, [int(r) for r in R], 1, int(a[0]), 0)[0]
        assert picked == (-1 if want[0] == n or R[want[0]] == 0 else want[0])


def test_the_header_declares_no_hip_type_and_the_abi_declares_the_guide():
    text = open(HEADER).read()
    assert "hip/" not in text and "float2" not in text
    from mppi_numba_amd import _lib
    abi = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mppi_hip.h")).read(), flags=re.S)
    for name, args in (("mppi_planner_set_guide", 10), ("mppi_planner_get_guide", 5), ("mppi_planner_guide_refresh", 1),
                       ("mppi_planner_get_guide_field", 2), ("mppi_planner_get_guide_rows", 3)):
        assert re.search(r"\b%s\s*\(" % name, abi), "include/mppi_hip.h does not declare %s" % name
        assert len(_lib.SIGNATURES[name]) == args
