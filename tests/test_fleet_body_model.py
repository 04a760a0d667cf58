"""CPU checks of the fleet-of-bodies model (tests/fleet_body_model.py; mppi_planner_set_fleet_bodies): a one-disc body is
the disc fleet to the bit, a finer cover or a padding duplicate never counts a robot twice, the inputs of the GPU
comparisons mean something and stay the same when sine and cosine move by what a device may differ in, and the fold that
counts a robot once (csrc/crowd_fold.h) equals a loop over the groups."""
import os
import re
import subprocess

import numpy as np
import pytest

import fleet_body_cases as cases
import fleet_body_model as M
import fleet_model
import wall_model
from test_fleet_model import same_bits, three_robots
from track_model import oracle_params

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROOM = np.float32([[[-3, -3], [9, -3]], [[9, -3], [9, 9]], [[0.5, 2.5], [2.5, 0.5]]])
ROOM_HW = np.float32([0.0625, 0.0625, 0.125])  # (dyadic, like the one-disc body: h + rho is exact in float32)


@pytest.mark.parametrize("T,W", [(30, 0), (37, 3)])
def test_a_one_disc_body_is_the_disc_fleet(T, W):
    """Body (0, 0, rho) with dyadic rho and margin: the centres are the positions, rho + margin and (rho + margin) + rho are
    exact in float32, so walls, hits and costs are fleet_model's with radii = rho, bit for bit."""
    rho, margin = cases.DYADIC
    _, params, x0s, us, noise = three_robots(T)
    body = np.float32([[0.0, 0.0, rho]])
    walls = M.body_walls(params, x0s, us, body)
    want = fleet_model.fleet_walls(params, x0s, us)
    assert walls.shape == (3, 2, 1, T, 2, 2) and same_bits(walls[:, :, 0], want)
    hw = M.halfwidths(body, margin)
    pair = fleet_model.halfwidths(rho, margin, 3)
    assert hw.dtype == np.float32 and (np.float64(hw[0]) + np.float64(np.float32(rho)) == pair.astype(np.float64)).all()
    hit_any = False
    for a in range(3):
        p = oracle_params(dict(params, x0=x0s[a]))
        wt, h = fleet_model.reader_walls(want[a], pair[a], ROOM[:W], ROOM_HW[:W] + np.float32(rho))  # (its reader is a point to them)
        st = wall_model.states(p, noise, us[a])
        hit_any = hit_any or bool(fleet_model.fleet_hits(st, wt[:2], h[:2]).any())
        np.testing.assert_array_equal(M.wall_counts(st, body, walls[a], hw, ROOM[:W], ROOM_HW[:W]), fleet_model.fleet_hits(st, wt, h))
        assert same_bits(M.costs(p, body, walls[a], hw, noise, us[a], ROOM[:W], ROOM_HW[:W]), fleet_model.fleet_costs(p, wt, h, noise, us[a]))
    assert hit_any, "bad input: no step hits a fleet wall"
    parked = M.body_walls(params, x0s, us, cases.body(3), parked=np.array([False, True, False]))
    from mppi_numba_amd.barebone import body_discs
    stand = body_discs(x0s[1].astype(np.float32), cases.body(3))  # (3, 2): it stands at its start pose, heading included
    assert same_bits(parked[0, 0], np.broadcast_to(stand[:, None, None, :], (3, T, 2, 2)).copy())


def test_a_finer_cover_and_padding_never_count_a_robot_twice():
    """The same cart covered by 1, 3 and 8 discs: a step's fleet hits never exceed the number of other robots, while the
    hits counted per slot do; and the device's padding slots (the last disc repeated up to a power of two) change nothing."""
    T = 37
    _, params, x0s, us, noise = three_robots(T)
    p = oracle_params(dict(params, x0=x0s[0]))
    st = wall_model.states(p, noise, us[0])
    above = False
    for F in (1, 3, 5, 8):
        body = cases.body(F)
        walls, hw = M.body_walls(params, x0s, us, body)[0], M.halfwidths(body, 0.05)
        robots, per_slot = M.robot_hits(st, body, walls, hw)
        counts = robots.sum(axis=2)
        assert counts.max() <= 2 and counts.any()
        above = above or bool((per_slot > 2).any())
        wide, wide_hw = M.padded(walls, hw)
        assert wide.shape[1] == M.group_size(F) and wide_hw.shape == (M.group_size(F),)
        np.testing.assert_array_equal(M.robot_hits(st, body, wide, wide_hw)[0], robots)
        if F in (3, 5):
            assert wide.shape[1] > F and M.robot_hits(st, body, wide, wide_hw)[1].sum() > per_slot.sum()
    assert above, "bad input: counting per slot never gives more than one hit a robot"
    assert [M.group_size(F) for F in range(1, 9)] == [1, 2, 4, 4, 8, 8, 8, 8]


@pytest.mark.parametrize("case", cases.COST_CASES, ids=str)
def test_the_cost_cases_mean_something(case):
    share = cases.the_input_means_something(cases.cost_case(*case)["model"])
    print(case, "share of rollouts that hit some robot, per reader: %.2f .. %.2f" % (share.min(), share.max()))


@pytest.mark.parametrize("kind", cases.EXTRA_CASES)
def test_the_extra_cases_mean_something(kind):
    case = cases.extra_case(kind)
    cases.the_input_means_something(case["model"])
    plain = cases.cost_case(3, 3, 2, 37, 1.0)["model"]["costs"]
    assert (case["model"]["costs"] != plain).any(), "bad input: the %s change no cost" % kind


@pytest.mark.parametrize("case", [c for c in cases.COST_CASES if c[3] == 12 or c[0] == 3], ids=str)
def test_sine_and_cosine_may_move(case):
    """Sine and cosine moved by +-1e-15, the ds and dc of test_footprint_model (the device's sincos_f64 is within 2e-16 of
    libm's): no wall endpoint and no hit count of the GPU cases changes -- which entitles the GPU tests to demand bits."""
    held = cases.cost_case(*case)
    base_walls, base_counts = cases.moved_counts(held, 0.0, 0.0)
    assert same_bits(base_walls, held["model"]["walls"])
    for ds, dc in ((-1e-15, 1e-15), (1e-15, 1e-15), (1e-15, -1e-15), (-1e-15, -1e-15)):
        walls, counts = cases.moved_counts(held, ds, dc)
        assert same_bits(walls, base_walls), (ds, dc)
        np.testing.assert_array_equal(counts, base_counts)


@pytest.mark.parametrize("case", cases.WALL_CASES, ids=str)
def test_the_wall_cases_do_not_feel_sine_and_cosine(case):
    held = cases.wall_case(*case)
    assert (held["walls"][..., 0, :] != held["walls"][..., 1, :]).any()
    for ds, dc in ((-1e-15, 1e-15), (1e-15, -1e-15)):
        moved = M.body_walls(held["params"], held["x0s"], held["us"], held["footprint"], None, ds, dc)
        assert same_bits(moved, held["walls"]), (ds, dc)


def test_two_discs_cannot_pass_in_the_corridor():
    """On the CPU, with fleet_model: the corridor is wider than two cart bodies side by side with their margins
    (2 x 0.26 + 0.05 between the carts, 0.26 + 0.05 from either wall: 1.19 m) and narrower than two circumscribed discs
    (2.26 m).  At every pair of lateral offsets, 2.5 cm apart, two discs of radius 0.54 m that pass each other are hit -- one of
    them by a wall, or one by the other -- so a disc fleet has no way through; no failing closed loop is run."""
    disc_width = 2 * (cases.CIRCUMSCRIBED + cases.WALL_HW) + 2 * cases.CIRCUMSCRIBED + cases.CART_MARGIN
    body_width = 2 * (0.26 + cases.WALL_HW) + 2 * 0.26 + cases.CART_MARGIN
    assert body_width < cases.CORRIDOR_WIDTH < disc_width
    T = 30
    lateral = np.arange(-cases.CORRIDOR_WIDTH / 2, cases.CORRIDOR_WIDTH / 2 + 1e-9, 0.025)
    xs = np.linspace(0.0, 6.0, T + 1)
    pair_hw = fleet_model.halfwidths(cases.CIRCUMSCRIBED, cases.CART_MARGIN, 2)[0]
    free = 0
    for y_other in lateral:
        other = np.stack([xs[::-1], np.full(T + 1, y_other)], 1).astype(np.float32)  # it comes the other way
        wall = np.stack([other[:-1], other[1:]], 1)[None]  # (1, T, 2, 2)
        wt, hw = fleet_model.reader_walls(wall, pair_hw, cases.CORRIDOR, np.float32(cases.WALL_HW + cases.CIRCUMSCRIBED))
        st = np.zeros((len(lateral), T + 1, 3), np.float32)
        st[:, :, 0], st[:, :, 1] = xs[None], lateral[:, None]
        mine = fleet_model.fleet_hits(st, wt, hw).sum(axis=1) == 0  # this disc meets neither a wall nor the other disc ...
        back = np.zeros((1, T + 1, 3), np.float32)
        back[0, :, :2] = other
        free += int(mine.sum()) * int(fleet_model.fleet_hits(back, wt[1:], hw[1:]).sum() == 0)  # ... which clears the walls itself
    assert free == 0, "%d pairs of lateral offsets let two discs of radius 0.54 m pass" % free


FOLD_MAIN = r"""
#include <cstdio>
#include <cstdint>
#include "crowd_fold.h"
static int naive(unsigned long long mask, int group, int g) {
  int hits = 0;
  for (int l0 = 0; l0 < g; l0 += group) {
    bool any = false;
    for (int l = l0; l < l0 + group; ++l) any = any || ((mask >> l) & 1ull);
    hits += any ? 1 : 0;
  }
  for (int l = g; l < 64; ++l) hits += (int)((mask >> l) & 1ull);
  return hits;
}
int main() {
  uint64_t s = 0x9E3779B97F4A7C15ull;
  long checked = 0, bad = 0;
  for (int group = 1; group <= 8; group *= 2)
    for (int g = 0; g <= 64; g += group)
      for (int i = 0; i < 64; ++i) {
        s ^= s << 13; s ^= s >> 7; s ^= s << 17;  // xorshift64
        const unsigned long long sparse = s & (s >> 21) & (s << 9);
        const unsigned long long masks[] = {s, sparse, ~sparse, 0ull, ~0ull, 1ull << (i & 63)};
        for (unsigned long long mask : masks) {
          ++checked;
          if (crowd_fold_count(mask, group, g) != naive(mask, group, g)) ++bad;
        }
      }
  int spans = 0;
  for (int grouped = 0; grouped <= 200; grouped += 4)
    for (int wbase = 0; wbase <= 256; wbase += 64) {
      int want = grouped - wbase;
      want = want < 0 ? 0 : (want > 64 ? 64 : want);
      spans += crowd_fold_span(grouped, wbase) != want;
    }
  std::printf("checked %ld bad %ld spans %d\n", checked, bad, spans);
  return bad != 0 || spans != 0;
}
"""


def test_the_fold_equals_a_loop_over_the_groups(tmp_path):
    """csrc/crowd_fold.h compiled alone by the host compiler: for Fp in {1, 2, 4, 8}, every g a multiple of Fp in 0 .. 64 and
    some 47000 masks (random, sparse, dense, empty, full, single bits) crowd_fold_count equals the naive count."""
    src = tmp_path / "fold_main.cpp"
    src.write_text(FOLD_MAIN)
    exe = tmp_path / "fold_main"
    subprocess.check_call(["c++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "mppi_numba_amd", "csrc"), "-o", str(exe), str(src)])
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    print(out.stdout)
    found = re.match(r"checked (\d+) bad (\d+) spans (\d+)", out.stdout)
    assert out.returncode == 0 and found and int(found.group(1)) > 40000 and found.group(2) == "0" and found.group(3) == "0", out.stdout


def test_header_declares_and_binding_covers_the_entry_points():
    from mppi_numba_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mppi_hip.h")).read(), flags=re.S)
    for name, args in (("mppi_planner_set_fleet_bodies", 5), ("mppi_planner_get_fleet_bodies", 3), ("mppi_planner_get_fleet_body_walls", 2)):
        found = re.search(r"\bint\s+%s\s*\(([^)]*)\)" % name, text)
        assert found, "include/mppi_hip.h does not declare %s" % name
        assert len(found.group(1).split(",")) == args
        assert len(_lib.SIGNATURES[name]) == args
        assert hasattr(_lib.load(), name), "libmppi_hip.so does not export %s" % name
