"""CPU-only: tests/occupancy_model.py against csrc/occupancy_grid.h compiled with g++ on its own -- the arithmetic the kernels
call -- bit for bit, and the model's field against its second formulation."""
import os
import subprocess

import numpy as np
import pytest

import occupancy_model as om

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "mppi_numba_amd", "csrc", "occupancy_grid.h")

PROGRAM = r"""
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "%s"
using namespace mppi;
int main() {
  char kind[8], a[64], b[64], c[64], d[64];
  int k, M;
  for (;;) {
    if (std::scanf("%%7s", kind) != 1) break;
    if (kind[0] == 'P') {  // a test point: a b k M (float32 each)
      if (std::scanf("%%63s %%63s %%d %%d", a, b, &k, &M) != 4) return 1;
      const double X = occupancy_point((float)std::strtod(a, nullptr), (float)std::strtod(b, nullptr), k, M);
      unsigned long long bits;
      std::memcpy(&bits, &X, 8);
      std::printf("%%llu\n", bits);
    } else if (kind[0] == 'C') {  // the cell of a point: X (double) lo res (float32) n
      if (std::scanf("%%63s %%63s %%63s %%d", a, b, c, &k) != 4) return 1;
      int cell = -7;
      const bool in = occupancy_cell(std::strtod(a, nullptr), (float)std::strtod(b, nullptr), (float)std::strtod(c, nullptr), k, &cell);
      std::printf("%%d %%d\n", (int)in, in ? cell : 0);
    } else {  // a threshold: inflate (float32) rho margin (double) res (float32)
      if (std::scanf("%%63s %%63s %%63s %%63s", a, b, c, d) != 4) return 1;
      std::printf("%%u\n", occupancy_threshold((float)std::strtod(a, nullptr), std::strtod(b, nullptr), std::strtod(c, nullptr),
                                               (float)std::strtod(d, nullptr)));
    }
  }
  return 0;
}
"""


def hx(v):
    v = float(v)
    return "nan" if v != v else v.hex()


@pytest.fixture(scope="module")
def header(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("occupancy_grid")
    src, exe = tmp / "grid.cpp", tmp / "grid"
    src.write_text(PROGRAM % HEADER)
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-o", str(exe), str(src)])

    def ask(lines):
        out = subprocess.run([str(exe)], input=("\n".join(lines) + "\n").encode(), stdout=subprocess.PIPE, check=True).stdout
        return out.decode().splitlines()
    return ask


@pytest.mark.parametrize("M", [1, 3, 8])
def test_the_test_points_equal_the_header(header, M):
    rng = np.random.default_rng(100 + M)
    A = np.concatenate([rng.uniform(-5, 5, 300), [np.nan, 1.0, -0.0, 3.4e38]]).astype(np.float32)
    B = np.concatenate([rng.uniform(-5, 5, 300), [1.0, np.nan, 0.0, -3.4e38]]).astype(np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        want = om.test_points(A, B, M)  # (M, n)
    lines = ["P %s %s %d %d" % (hx(a), hx(b), k, M) for k in range(1, M + 1) for a, b in zip(A, B)]
    got = np.array([int(v) for v in header(lines)], np.uint64).reshape(M, len(A))
    same = (got == want.view(np.uint64)) | (np.isnan(want) & np.isnan(got.view(np.float64)))
    assert same.all(), np.argwhere(~same)[:5]
    assert (want[M - 1][:300] == B[:300].astype(np.float64)).all(), "the last point is the post-step centre itself"


def test_the_inside_rule_equals_the_header(header):
    rng = np.random.default_rng(7)
    lo, res, n = np.float32(-1.3), np.float32(0.1), 37
    hi = np.float64(lo) + n * np.float64(res)
    borders = np.float64(lo) + np.arange(n + 1) * np.float64(res)
    X = np.concatenate([rng.uniform(-3, 4, 400), rng.uniform(float(lo) - 2, float(lo), 20), rng.uniform(hi, hi + 2, 20), borders,
                        np.nextafter(borders, -np.inf), np.nextafter(borders, np.inf), [np.nan, np.inf, -np.inf, 1e300, -1e300]])
    inside, cell = om.cell_of(X, lo, res, n)
    got = np.array([[int(v) for v in line.split()] for line in header(["C %s %s %s %d" % (hx(x), hx(lo), hx(res), n) for x in X])])
    np.testing.assert_array_equal(got[:, 0], inside.astype(int))
    np.testing.assert_array_equal(got[:, 1], cell)
    assert inside.any() and (~inside[X < lo]).all() and (~inside[X > hi]).all() and not inside[-5:].any()
    assert (X < lo).sum() >= 20 and (X > hi).sum() >= 20, "points outside on both sides of the axis"
    # ... the same rule serves both axes: a point is inside iff both say so (n = 1: one cell)
    one, _ = om.cell_of(np.float64([-0.5, 0.0, 0.05, 0.11, 0.2]), 0.0, 0.1, 1)
    np.testing.assert_array_equal(one, [False, True, True, False, False])


def test_the_thresholds_equal_the_header_and_are_monotone(header):
    rng = np.random.default_rng(11)
    rows = []
    for _ in range(200):
        inflate, res = np.float32(rng.uniform(0, 0.5)), np.float32(rng.uniform(0.02, 0.5))
        rho = np.float64(np.float32(rng.uniform(0, 0.6)))
        margins = np.concatenate([[0.0], np.sort(rng.uniform(0.01, 1.0, 4)).astype(np.float32).astype(np.float64)])
        rows.append((inflate, rho, margins, res))
    rows.append((np.float32(0.0), 0.0, np.float64([0.0, 0.1]), np.float32(0.1)))
    rows.append((np.float32(3e38), 3e38, np.float64([0.0, 3e38]), np.float32(1e-30)))  # (the cap)
    lines = ["T %s %s %s %s" % (hx(i), hx(r), hx(m), hx(s)) for i, r, ms, s in rows for m in ms]
    got = iter(int(v) for v in header(lines))
    for inflate, rho, margins, res in rows:
        want = np.array([om.threshold(inflate, rho, m, res) for m in margins], np.uint32)
        have = np.array([next(got) for _ in margins], np.uint32)
        np.testing.assert_array_equal(have, want)
        assert (np.diff(want.astype(np.int64)) >= 0).all(), "the thresholds are non-decreasing in the level"
    assert om.threshold(np.float32(3e38), 3e38, 0.0, np.float32(1e-30)) == om.THR_MAX
    assert om.threshold(np.float32(0.0), 0.0, 0.0, np.float32(0.1)) == 0, "a point robot without inflation hits occupied cells only"


@pytest.mark.parametrize("shape,fill", [((1, 1), 1.0), ((1, 70), 0.1), ((65, 3), 0.2), ((64, 64), 0.01), ((70, 129), 0.3),
                                        ((33, 41), 0.0), ((9, 130), 1.0), ((130, 67), 0.001)])
def test_the_field_equals_its_separable_form(shape, fill):
    rng = np.random.default_rng(shape[0] * 1000 + shape[1])
    cells = rng.uniform(size=shape) < fill
    D = om.field_of(cells)
    np.testing.assert_array_equal(D, om.field_separable(cells))
    assert (D[cells] == 0).all() and (D[~cells] > 0).all()
    if not cells.any():
        assert (D == om.FAR).all()
    corner = np.zeros(shape, bool)
    corner[-1, 0] = True
    iy, ix = np.indices(shape)
    np.testing.assert_array_equal(om.field_of(corner), ((iy - (shape[0] - 1)) ** 2 + ix ** 2).astype(np.uint32))


def test_a_level_is_a_union_over_points_and_body_discs():
    """level_bits on two states written by hand: the chord's inner points see what its end does not."""
    cells = np.zeros((10, 10), np.uint8)
    cells[5, 5] = 1
    st = np.float32([[[0.05, 0.55, 0.0], [1.05, 0.55, 0.0]]])  # one step from cell (5, 0) to cell (5, 10): outside at its end
    for M, hit in ((1, False), (2, True), (4, True), (3, False)):
        grid = om.Grid((0.0, 0.0), 0.1, cells, 0.0, M)
        bits, inside = om.level_bits(grid, st, [0.0, 0.25])
        assert bits.shape == (2, 1, 1) and inside.shape == (1, 1, 1, M)
        assert bool(bits[0, 0, 0]) == hit, M
        assert not inside[0, 0, 0, M - 1], "the post-step point lies outside the grid"
    near = om.level_bits(om.Grid((0.0, 0.0), 0.1, cells, 0.0, 3), st, [0.0, 0.25])[0]
    assert not near[0, 0, 0] and near[1, 0, 0], "k = 1 of 3 lands two cells from the occupied one: inside the 0.25 m ring only"
