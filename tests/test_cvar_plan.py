"""The CVaR mode's launches and the route from the TDMs to the cell words (csrc/cvar_plan.h: cvar_choose,
cvar_reduce_choose, cells_choose, sample_choose) against tables.

The header is plain C++: a small host program compiled with g++ reads states and prints choices.  The expected rows were
written by reading the code these functions replaced (launch_rollout_tdm with tdm_fast_kernel, launch_cvar_reduce with
cvar_numel, sample_into_cells, ensure_packed, tdm_launch_philox and the xoroshiro launch of tdm_sample_on), not by running
them; every LDS size and every chunk count of the tables is worked out a second time here.

The map quantities of the CVaR states are those of tests/test_map_plan.py (bench.py's maps as an MI355X reports them:
traction up to 1.0, dt = 0.1 s, w in [-pi, pi], cells of 0.25 m), in CVaR mode.  The cells states are a map of 70 x 90 cells
in a ring of 2 (74 x 94), as tests/test_gpu_cvar_plan.py cuts it.

Rows marked TRAP keep answers that look odd on purpose: they are today's, and a change to any of them is a change of
behaviour.
"""
import itertools
import math
import os
import struct
import subprocess

import pytest

from test_map_plan import FIELDS as MAP_FIELDS, held as map_held

HEADER = os.path.join(os.path.dirname(__file__), "..", "mppi_numba_amd", "csrc", "cvar_plan.h")

CELLS_FIELDS = ["mode", "M", "for_solve", "same_tdm", "lin_rng", "ang_rng", "lin_bins", "ang_bins", "alpha_positive",
                "lin_first_sample", "ang_first_sample", "rows", "cols", "lin_compact_ok", "ang_compact_ok", "lin_injected",
                "ang_injected", "lin_injected_nonneg", "ang_injected_nonneg", "has_risk", "packed_match"]

PROGRAM = r"""
#include <cstdio>
#include <cstring>
#include "%s"
static bool read_ints(int* f, int n) {
  for (int i = 0; i < n; ++i)
    if (std::scanf("%%d", f + i) != 1) return false;
  return true;
}
int main() {
  char what[16];
  while (std::scanf("%%15s", what) == 1) {
    if (!std::strcmp(what, "cvar")) {
      CvarHeld s;
      std::memset(&s, 0, sizeof(s));
      MapHeld& h = s.map;
      if (std::scanf("%%d %%d %%d %%d %%d %%d %%d %%d %%d %%d %%d %%d %%d %%d %%d %%d %%d %%d %%d %%d %%d %%lf %%lf %%lf %%lf %%f %%f %%f %%f %%f %%f %%f %%f %%f %%f %%d %%d %%d",
                     &h.mode, &h.math, &h.debug_flags, &h.speculation_off, &h.n_local, &h.T, &h.num_cus, &h.lds_per_cu, &h.inst_set,
                     &h.inst_tiles, &h.B, &h.cells16_valid, &h.cells16_with_risk, &h.pitch16, &h.rows, &h.cols, &h.lin_max_byte,
                     &h.ang_max_byte, &h.sink_ring, &h.grid_packed, &h.theta_bounded, &h.lin_lo, &h.lin_ratio, &h.ang_lo,
                     &h.ang_ratio, &h.dt, &h.res, &h.xlo, &h.ylo, &h.vrange[0], &h.vrange[1], &h.wrange[0], &h.wrange[1], &h.x0,
                     &h.y0, &s.num_grid_samples, &s.m_count, &s.want_sample_costs) != 38)
        return 1;
      const CvarChoice c = cvar_choose(s);
      std::printf("refused=%%d launch=%%d fast=%%d cost_f32=%%d exact=%%d pow2res=%%d threads=%%d mp2=%%d workgroups=%%d lds=%%zu "
                  "set_attribute=%%d costs_to=%%d\n", c.refused, c.launch, c.fast, c.cost_f32, c.exact, c.pow2res, c.threads, c.mp2,
                  c.workgroups, c.lds, c.set_attribute, c.costs_to);
    } else if (!std::strcmp(what, "reduce")) {
      int m, count;
      float alpha;
      if (std::scanf("%%d %%d %%f", &m, &count, &alpha) != 3) return 1;
      const CvarReduceChoice c = cvar_reduce_choose(m, count, alpha);
      std::printf("refused=%%d m_total=%%d mp2=%%d threads=%%d numel=%%d lds=%%zu\n", c.refused, c.m_total, c.mp2, c.threads, c.numel, c.lds);
    } else if (!std::strcmp(what, "cells")) {
      CellsHeld h;
      std::memset(&h, 0, sizeof(h));
      static_assert(sizeof(CellsHeld) == %d * sizeof(int), "CellsHeld has a field the test does not know");
      if (!read_ints(&h.mode, %d)) return 1;
      const CellsChoice c = cells_choose(h);
      std::printf("route=%%d grid_x=%%u grid_y=%%u bins=%%d cell_groups=%%ld mirror=%%d pitch16=%%d mirror_units=%%zu mirror_grid=%%u\n",
                  c.route, c.grid_x, c.grid_y, c.bins, c.cell_groups, c.mirror, c.pitch16, c.mirror_units, c.mirror_grid);
    } else if (!std::strcmp(what, "sample")) {
      int a[7];
      if (!read_ints(a, 7)) return 1;
      const SampleChoice c = sample_choose(a[0], a[1], a[2], a[3], a[4], a[5], a[6]);
      std::printf("kernel=%%d grid_x=%%u grid_y=%%u block=%%d cell_groups=%%ld bins=%%d chunks=%%d g_chunk=%%d threads=%%d form=%%d\n",
                  c.kernel, c.grid_x, c.grid_y, c.block, c.cell_groups, c.bins, c.chunks, c.g_chunk, c.threads, bins_form(a[1]));
    } else {
      return 1;
    }
  }
  return 0;
}
"""

DET, SPEED, TDM, BAREBONE = range(4)
EXACT, FAST = 0, 1
PHILOX, XOROSHIRO = 0, 1
CVAR_FAST, CVAR = 6, 7                      # NoiseLaunch (noise_plan.h)
TO_NOWHERE, TO_SAMPLE_COSTS, TO_SLAB = range(3)
NOTHING, SAMPLE, PACK_SINGLE, PACK_MULTI = range(4)
NO_MIRROR, MIRROR16, MIRROR32_RISK = range(3)
COLUMNS, GENERIC, XORO_KERNEL = range(3)
KIB = 1024


def f32(x):
    return struct.unpack("f", struct.pack("f", x))[0]


def pow2(v):
    p = 1
    while p < v:
        p *= 2
    return p


@pytest.fixture(scope="module")
def choose(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("cvar_plan")
    src = tmp / "choose.cpp"
    src.write_text(PROGRAM % (os.path.abspath(HEADER), len(CELLS_FIELDS), len(CELLS_FIELDS)))
    exe = tmp / "choose"
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-o", str(exe), str(src)])

    def run(what, lines):
        text = "".join("%s %s\n" % (what, " ".join(repr(v) for v in line)) for line in lines)
        out = subprocess.run([str(exe)], input=text.encode(), stdout=subprocess.PIPE, check=True).stdout.decode().splitlines()
        assert len(out) == len(lines)
        return [{k: int(v) for k, v in (item.split("=") for item in line.split())} for line in out]
    return run


def check(rows, got):
    for (state, want), have in zip(rows, got):
        for key, value in want.items():
            assert have[key] == value, "state %s: %s = %s, the table says %s" % (state, key, have[key], value)


# ---- cvar_choose ------------------------------------------------------------------------------------------------------
def cvar(T=100, M=128, m_count=1, want_sample_costs=0, **over):
    """c3's planner state: N = 1024 rollouts, exact math, |theta| bounded, rotation within its proof (0.1 * pi * 1.0 rad)"""
    s = map_held(mode=TDM, n_local=1024, T=T, **over)
    s.update(M=M, m_count=m_count, want_sample_costs=want_sample_costs)
    return s


def cvar_line(s):
    return [s[k] for k in MAP_FIELDS] + [s["M"], s["m_count"], s["want_sample_costs"]]


def lds_general(T, M):
    """k_rollout_tdm: [T] double2 control ratios | [next_pow2(M)] float"""
    return 16 * T + 4 * pow2(M)


def lds_fast(T, M):
    """k_rollout_tdm_fast: [T] double2 ratios + [T] double | [next_pow2(M)] float"""
    return (16 + 8) * T + 4 * pow2(M)


def fast(lds, threads, pow2res=1, cost_f32=0, **more):
    return dict(refused=0, launch=CVAR_FAST, fast=1, lds=lds, threads=threads, pow2res=pow2res, cost_f32=cost_f32,
                set_attribute=0, **more)


def general(lds, threads, exact=1, set_attribute=0, **more):
    # TRAP: the general kernel never takes pow2res (its text names exact= only), on a map of 0.25 m cells too
    return dict(refused=0, launch=CVAR, fast=0, lds=lds, threads=threads, exact=exact, pow2res=0, cost_f32=0,
                set_attribute=set_attribute, **more)


CVAR_ROWS = [
    (cvar(T=100, M=128), fast(2912, 128, mp2=128, workgroups=1024, costs_to=TO_NOWHERE)),
    # the fast kernel's 64 KiB: 48 000 + 4 * 4096 fits, 4097 samples round up to 8192
    (cvar(T=2000, M=4096), fast(64384, 1024, mp2=4096)),
    (cvar(T=2000, M=4097), general(64768, 1024, mp2=8192)),   # (within 64 KiB itself: no attribute)
    (cvar(T=2001, M=128), general(16 * 2001 + 512, 128)),     # the rotation's proof ends at 2000 steps
    (cvar(T=20, M=16384), general(65856, 1024, set_attribute=1, mp2=16384)),
    (cvar(T=20, M=65536), dict(refused=1, launch=CVAR, fast=0, lds=320 + 4 * 65536)),
    # the 160 KiB check is the general kernel's size, whichever kernel would run
    (cvar(T=4096, M=32768), dict(refused=1, launch=CVAR, lds=65536 + 131072)),
    (cvar(T=4096, M=16384), general(65536 + 65536, 1024, set_attribute=1)),
    (cvar(theta_bounded=0), general(2112, 128)),
    (cvar(w_lo=-4.0, w_hi=4.0), general(2112, 128)),          # 0.1 * 4 * 1.0 = 0.4 rad > 0.36
    (cvar(res=0.3), fast(2912, 128, pow2res=0)),
    # MPPI_MATH_FAST: the fast kernel's <cost f32> form; the general kernel's exact=0
    (cvar(math=FAST), fast(2912, 128, cost_f32=1, exact=0)),
    (cvar(math=FAST, w_lo=-4.0, w_hi=4.0), general(2112, 128, exact=0)),
    (cvar(math=FAST, res=0.3), fast(2912, 128, pow2res=0, cost_f32=1)),
]
# threads: one per traction sample, whole waves, at most 1024
CVAR_ROWS += [(cvar(M=m), dict(threads=t, fast=1, mp2=pow2(m))) for m, t in ((1, 64), (64, 64), (65, 128), (1024, 1024), (2048, 1024))]
# where the per-sample costs go: sharded samples go to this rank's slab, wanted or not
CVAR_ROWS += [(cvar(m_count=c, want_sample_costs=w), dict(costs_to=to, fast=1))
              for c, w, to in ((1, 0, TO_NOWHERE), (1, 1, TO_SAMPLE_COSTS), (2, 0, TO_SLAB), (2, 1, TO_SLAB))]
CVAR_ROWS += [(cvar(m_count=2, want_sample_costs=1, theta_bounded=0), dict(costs_to=TO_SLAB, fast=0))]


def test_cvar_choose_matches_the_table(choose):
    check(CVAR_ROWS, choose("cvar", [cvar_line(s) for s, _ in CVAR_ROWS]))


def test_the_cvar_tables_lds_sizes_follow_from_the_kernels_layouts():
    for state, want in CVAR_ROWS:
        if "lds" not in want:
            continue
        T, M = state["T"], state["M"]
        if want["refused"]:
            assert want["lds"] == lds_general(T, M) > 160 * KIB
        elif want["fast"]:
            assert want["lds"] == lds_fast(T, M) <= 64 * KIB
        else:
            assert want["lds"] == lds_general(T, M) <= 160 * KIB
            assert want["set_attribute"] == int(want["lds"] > 64 * KIB)
    assert lds_fast(2000, 4097) > 64 * KIB >= lds_fast(2000, 4096)


def test_cvar_choose_over_a_product_of_the_switches(choose):
    """The fast kernel never runs with more than 64 KiB; the launch id noise_plan.h is given is that of the kernel chosen."""
    states = [cvar(T=T, M=M, m_count=c, want_sample_costs=w, math=mth, theta_bounded=tb, w_lo=-wr, w_hi=wr)
              for T, M, c, w, mth, tb, wr in itertools.product((20, 100, 2000, 2001), (1, 64, 65, 1024, 4096, 4097, 16384, 65536),
                                                               (1, 2), (0, 1), (EXACT, FAST), (0, 1), (math.pi, 4.0))]
    for s, c in zip(states, choose("cvar", [cvar_line(s) for s in states])):
        T, M = s["T"], s["M"]
        if lds_general(T, M) > 160 * KIB:
            assert c["refused"] and not c["fast"] and c["launch"] == CVAR, s
            continue
        rotation = f32(0.1) * f32(s["w_hi"]) * 1.0 <= 0.36 and T <= 2000
        want_fast = bool(s["theta_bounded"]) and rotation and lds_fast(T, M) <= 64 * KIB
        assert not c["refused"] and c["fast"] == want_fast, s
        assert c["launch"] == (CVAR_FAST if c["fast"] else CVAR), s
        assert c["lds"] == (lds_fast(T, M) if c["fast"] else lds_general(T, M)), s
        assert not c["fast"] or c["lds"] <= 64 * KIB, s
        assert c["set_attribute"] == int(not c["fast"] and c["lds"] > 64 * KIB), s
        assert c["cost_f32"] == int(c["fast"] and s["math"] == FAST) and c["exact"] == int(s["math"] == EXACT), s
        assert c["pow2res"] == c["fast"], s  # (cells of 0.25 m)
        assert c["workgroups"] == s["n_local"] and c["mp2"] == pow2(M), s


# ---- cvar_reduce_choose -----------------------------------------------------------------------------------------------
def numel(m_total, alpha):
    return min(max(math.ceil(m_total * f32(alpha)), 1), m_total)


# (samples per rank, ranks, alpha) -> threads: 1024 above 1024, 64 below 64, else one per element; LDS 4 bytes per element
REDUCE_ROWS = [
    ((4, 2, 0.8), dict(refused=0, m_total=8, mp2=8, threads=64, lds=32, numel=7)),
    ((32, 2, 0.8), dict(refused=0, m_total=64, mp2=64, threads=64, lds=256, numel=52)),
    ((512, 2, 0.8), dict(refused=0, m_total=1024, mp2=1024, threads=1024, lds=4096, numel=820)),
    ((1024, 2, 0.8), dict(refused=0, m_total=2048, mp2=2048, threads=1024, lds=8192, numel=1639)),
    ((8192, 2, 0.8), dict(refused=0, m_total=16384, mp2=16384, threads=1024, lds=64 * KIB, numel=13108)),
    ((16385, 1, 0.8), dict(refused=1, m_total=16385, mp2=32768, lds=128 * KIB)),
    ((100, 3, 0.5), dict(refused=0, m_total=300, mp2=512, threads=512, lds=2048, numel=150)),
    ((512, 2, 1.0), dict(numel=1024)),
    ((512, 2, 1e-6), dict(numel=1)),   # ceil(0.001) = 1
    ((512, 2, 0.0), dict(numel=1)),    # clamped from below
    ((4, 2, 1.5), dict(numel=8)),      # ... and from above
]


def test_cvar_reduce_choose_matches_the_table(choose):
    check(REDUCE_ROWS, choose("reduce", [list(s) for s, _ in REDUCE_ROWS]))
    for (m, count, alpha), want in REDUCE_ROWS:
        assert want["numel"] == numel(m * count, alpha) if "numel" in want else want["refused"]
        if "lds" in want:
            assert want["lds"] == 4 * pow2(m * count) and want["refused"] == int(want["lds"] > 64 * KIB)


# ---- cells_choose -----------------------------------------------------------------------------------------------------
ROWS, COLS = 74, 94
CELL_GROUPS = ROWS * ((COLS + 3) // 4)  # groups of 4 cells along a row


def cells(**over):
    """solve() of a CVaR planner with 256 samples on two Philox TDMs of 8 bins, nothing packed yet"""
    s = dict(mode=TDM, M=256, for_solve=1, same_tdm=0, lin_rng=PHILOX, ang_rng=PHILOX, lin_bins=8, ang_bins=8, alpha_positive=1,
             lin_first_sample=0, ang_first_sample=0, rows=ROWS, cols=COLS, lin_compact_ok=1, ang_compact_ok=1, lin_injected=0,
             ang_injected=0, lin_injected_nonneg=0, ang_injected_nonneg=0, has_risk=0, packed_match=0)
    assert set(over) <= set(s), over
    s.update(over)
    return s


def staged(**over):
    """a stage-level call (rollout(), get_state_rollout(), ...): what is there is packed if it changed"""
    return cells(for_solve=0, **over)


def sampled(bins=0):
    # a workgroup of 256 threads takes 4 cell groups
    return dict(route=SAMPLE, bins=bins, cell_groups=CELL_GROUPS, grid_x=-(-CELL_GROUPS // 4), grid_y=1, mirror=NO_MIRROR)


def single(mirror):
    pitch = -(-COLS // 8) * 8
    want = dict(route=PACK_SINGLE, grid_x=-(-ROWS * COLS // 256), grid_y=1, mirror=mirror)
    if mirror != NO_MIRROR:  # speed-map mode: 32-bit cells in the same buffer, twice the 16-bit units; a thread per cell
        want.update(pitch16=pitch, mirror_units=ROWS * pitch * (2 if mirror == MIRROR32_RISK else 1), mirror_grid=-(-ROWS * pitch // 256))
    return want


def multi(m):
    # TRAP: no mirror on this route either -- cells16_valid is cleared on every repack
    return dict(route=PACK_MULTI, grid_x=ROWS * -(-COLS // 64), grid_y=-(-m // 64), mirror=NO_MIRROR, mirror_units=0)


IDLE = dict(route=NOTHING, mirror=NO_MIRROR)

CELLS_ROWS = [
    (cells(), sampled()),
    # the measured border, in solve() and outside it
    (cells(M=190), IDLE), (cells(M=191), IDLE), (cells(M=192), sampled()),
    (staged(M=192), multi(192)), (staged(M=190), multi(190)),
    # each condition failing alone: solve() samples and packs the ordinary way
    (cells(mode=DET), IDLE), (cells(mode=SPEED), IDLE),
    (cells(same_tdm=1), IDLE),  # TRAP: a lin TDM passed as ang too falls back to sample + pack
    (cells(lin_rng=XOROSHIRO), IDLE), (cells(ang_rng=XOROSHIRO), IDLE),
    (cells(lin_bins=65), IDLE), (cells(ang_bins=65), IDLE),
    (cells(alpha_positive=0), IDLE),
    (cells(ang_first_sample=2), IDLE), (cells(lin_first_sample=2, ang_first_sample=2), sampled()),
    # TRAP: a one-hot TDM whose unchanged maps the ordinary sampling step skips is sampled again by this route -- one_hot is
    # not among the inputs; nor is what is packed already
    (cells(packed_match=1), sampled()),
    # the bins form follows the larger PMF
    (cells(lin_bins=9, ang_bins=9), sampled(1)), (cells(lin_bins=16, ang_bins=16), sampled(1)),
    (cells(lin_bins=17, ang_bins=17), sampled(2)), (cells(lin_bins=32, ang_bins=32), sampled(2)),
    (cells(lin_bins=33, ang_bins=33), sampled(3)), (cells(lin_bins=64, ang_bins=64), sampled(3)),
    (cells(lin_bins=8, ang_bins=33), sampled(3)), (cells(lin_bins=17, ang_bins=2), sampled(2)),
    # the solves tests/test_gpu_philox_exact.py::test_cell_word_sampler relies on: 5 and 12 bins on a padded map of 34 x 45
    # cells, an odd M among them -- this route, the 16-bin form (the library has no text that names the route)
    (cells(lin_bins=5, ang_bins=12, rows=34, cols=45, M=192), dict(route=SAMPLE, bins=1, cell_groups=34 * 12, grid_x=102)),
    (cells(lin_bins=5, ang_bins=12, rows=34, cols=45, M=193), dict(route=SAMPLE, bins=1, cell_groups=34 * 12, grid_x=102)),
    (cells(lin_bins=5, ang_bins=12, rows=34, cols=45, M=256), dict(route=SAMPLE, bins=1, cell_groups=34 * 12, grid_x=102)),
    # one sample: the 16-bit mirror where both grids are 7-bit; speed-map mode: 32-bit cells with the risk byte
    (staged(mode=DET, M=1), single(MIRROR16)),
    (staged(mode=TDM, M=1), single(MIRROR16)),
    (staged(mode=DET, M=1, has_risk=1), single(MIRROR16)),
    (staged(mode=SPEED, M=1, has_risk=1), single(MIRROR32_RISK)),
    (staged(mode=SPEED, M=1), single(MIRROR16)),  # (check_tdms refuses this state before anything is packed)
    (staged(mode=DET, M=1, lin_compact_ok=0), single(NO_MIRROR)),
    (staged(mode=DET, M=1, ang_compact_ok=0), single(NO_MIRROR)),
    # injected grids: their own bytes decide, a negative one rules the mirror out
    (staged(mode=DET, M=1, lin_injected=1, lin_injected_nonneg=1), single(MIRROR16)),
    (staged(mode=DET, M=1, lin_injected=1, lin_injected_nonneg=0), single(NO_MIRROR)),
    (staged(mode=DET, M=1, ang_injected=1, ang_injected_nonneg=0), single(NO_MIRROR)),
    (staged(mode=DET, M=1, ang_injected=1, ang_injected_nonneg=1, ang_compact_ok=0), single(MIRROR16)),
    # TRAP: lin's own compact_ok is asked besides the 7-bit test on both grids
    (staged(mode=DET, M=1, lin_injected=1, lin_injected_nonneg=1, lin_compact_ok=0), single(NO_MIRROR)),
    # several samples
    (staged(M=2), multi(2)), (staged(M=64), multi(64)), (staged(M=65), multi(65)),
    # packed already; the barebone mode
    (staged(packed_match=1), IDLE), (staged(mode=DET, M=1, packed_match=1), IDLE),
    (cells(mode=BAREBONE), IDLE), (staged(mode=BAREBONE), IDLE),
]


def test_cells_choose_matches_the_table(choose):
    check(CELLS_ROWS, choose("cells", [[s[k] for k in CELLS_FIELDS] for s, _ in CELLS_ROWS]))


def test_cells_choose_gives_one_route_per_state(choose):
    """Over a product of the switches: one of the four routes, and only that route's numbers."""
    keys = ["mode", "M", "for_solve", "same_tdm", "lin_rng", "lin_bins", "alpha_positive", "ang_first_sample", "lin_compact_ok",
            "lin_injected", "has_risk", "packed_match"]
    values = [(DET, SPEED, TDM, BAREBONE), (1, 2, 191, 192), (0, 1), (0, 1), (PHILOX, XOROSHIRO), (8, 65), (0, 1), (0, 2), (0, 1),
              (0, 1), (0, 1), (0, 1)]
    states = [cells(**dict(zip(keys, v))) for v in itertools.product(*values)]
    for s, c in zip(states, choose("cells", [[s[k] for k in CELLS_FIELDS] for s in states])):
        into = (s["for_solve"] and s["mode"] == TDM and not s["same_tdm"] and s["lin_rng"] == PHILOX and s["lin_bins"] <= 64
                and s["alpha_positive"] and s["ang_first_sample"] == 0 and s["M"] >= 192)
        if s["mode"] == BAREBONE:
            want = NOTHING
        elif into:
            want = SAMPLE
        elif s["for_solve"] or s["packed_match"]:
            want = NOTHING
        else:
            want = PACK_SINGLE if s["M"] == 1 else PACK_MULTI
        assert c["route"] == want, s
        assert (c["cell_groups"] > 0) == (want == SAMPLE) and (c["grid_x"] > 0) == (want != NOTHING), s
        assert c["grid_y"] == (-(-s["M"] // 64) if want == PACK_MULTI else 1), s
        assert c["mirror"] == NO_MIRROR or want == PACK_SINGLE, s
        assert (c["mirror_units"] > 0) == (c["pitch16"] > 0) == (c["mirror_grid"] > 0) == (c["mirror"] != NO_MIRROR), s


# ---- sample_choose ----------------------------------------------------------------------------------------------------
def columns(rows, cols, G):
    """k_sample_grids_philox_cols: enough workgroups to fill the chip (256 Ki threads), an even count of samples per thread"""
    groups = rows * ((cols + 3) // 4)
    chunks = min(max(-(-256 * 1024 // groups), 1), G)
    g_chunk = (-(-G // chunks) + 1) // 2 * 2
    return dict(kernel=COLUMNS, cell_groups=groups, chunks=chunks, g_chunk=g_chunk, grid_x=-(-groups // 256), grid_y=-(-G // g_chunk),
                block=256)


# (rng, bins, rows, cols, G, thread_dim_x, thread_dim_y)
SAMPLE_ROWS = [
    ((PHILOX, 8, 70, 90, 256, 16, 16), dict(kernel=COLUMNS, cell_groups=1610, chunks=163, g_chunk=2, grid_x=7, grid_y=128, bins=0)),
    ((PHILOX, 8, 70, 90, 8, 16, 16), dict(kernel=COLUMNS, cell_groups=1610, chunks=8, g_chunk=2, grid_x=7, grid_y=4)),
    ((PHILOX, 8, 70, 90, 1, 16, 16), dict(kernel=COLUMNS, chunks=1, g_chunk=2, grid_y=1)),
    ((PHILOX, 8, 70, 90, 3, 16, 16), dict(kernel=COLUMNS, chunks=3, g_chunk=2, grid_y=2)),
    # bench.py's maps: 260 x 260 cells, 128 samples: 16 chunks of 8
    ((PHILOX, 8, 260, 260, 128, 16, 16), dict(kernel=COLUMNS, cell_groups=16900, chunks=16, g_chunk=8, grid_x=67, grid_y=16)),
    ((PHILOX, 8, 260, 260, 1024, 16, 16), dict(kernel=COLUMNS, chunks=16, g_chunk=64, grid_y=16)),
    # a map larger than 256 Ki cell groups: one chunk
    ((PHILOX, 8, 1024, 1028, 10, 16, 16), dict(kernel=COLUMNS, cell_groups=1024 * 257, chunks=1, g_chunk=10, grid_x=1028, grid_y=1)),
    # the chunked launches tests/test_gpu_philox_exact.py draws byte for byte: 16 chunks asked for, 6 samples each, so 11
    # workgroups cover 65 samples and the last holds half a pair; and 750 chunks of 2
    ((PHILOX, 8, 128, 512, 65, 16, 16), dict(kernel=COLUMNS, cell_groups=16384, chunks=16, g_chunk=6, grid_x=64, grid_y=11)),
    ((PHILOX, 8, 16, 48, 1500, 16, 16), dict(kernel=COLUMNS, cell_groups=192, chunks=1366, g_chunk=2, grid_x=1, grid_y=750)),
    ((PHILOX, 8, 5, 7, 65, 16, 16), dict(kernel=COLUMNS, cell_groups=10, chunks=65, g_chunk=2, grid_x=1, grid_y=33)),
    # beyond 64 bins: the generic kernel, a thread per (sample, cell group)
    ((PHILOX, 65, 70, 90, 256, 16, 16), dict(kernel=GENERIC, cell_groups=1610, grid_x=1610, grid_y=1, block=256, chunks=0)),
    ((PHILOX, 200, 70, 90, 3, 16, 16), dict(kernel=GENERIC, grid_x=19, grid_y=1)),
    # the xoroshiro-compatible generator: a state per thread of the reference's launch, waves of 64
    ((XOROSHIRO, 8, 70, 90, 8, 16, 16), dict(kernel=XORO_KERNEL, threads=2048, grid_x=32, grid_y=1, block=64)),
    ((XOROSHIRO, 65, 70, 90, 3, 5, 5), dict(kernel=XORO_KERNEL, threads=75, grid_x=2, block=64)),
]
# the bins forms 8 | 16 | 32 | 64, one ladder for both Philox samplers
SAMPLE_ROWS += [((PHILOX, b, 70, 90, 8, 16, 16), dict(kernel=COLUMNS if b <= 64 else GENERIC, form=f, bins=f if b <= 64 else 0))
                for b, f in ((1, 0), (8, 0), (9, 1), (16, 1), (17, 2), (32, 2), (33, 3), (64, 3), (65, 3))]


def test_sample_choose_matches_the_table(choose):
    check(SAMPLE_ROWS, choose("sample", [list(s) for s, _ in SAMPLE_ROWS]))


def test_the_sample_tables_chunks_follow_from_the_rule():
    for (rng, bins, rows, cols, G, _, _), want in SAMPLE_ROWS:
        if want["kernel"] != COLUMNS:
            continue
        again = columns(rows, cols, G)
        for key, value in want.items():
            assert again.get(key, value) == value, ((rows, cols, G), key)
        assert again["g_chunk"] % 2 == 0 and again["grid_y"] * again["g_chunk"] >= G
