"""The disc-sample rows of the barebone launch choice (csrc/barebone_plan.h), compiled on its own as
tests/test_barebone_plan.py compiles it: family crowd, the sample form, its chunk and its LDS -- against the layout of
k_rollout_barebone_crowd's sample forms worked out here -- and the refusal when crowd mode is off."""
import os
import subprocess

HEADER = os.path.join(os.path.dirname(__file__), "..", "mppi_numba_amd", "csrc", "barebone_plan.h")

PROGRAM = r"""
#include <cstdio>
#include "%s"
int main() {
  BareboneHeld h;
  int crowd, wtrk, fleet, gtrk;
  while (std::scanf("%%d %%d %%d %%d %%d %%d %%d %%d %%d %%d %%d", &h.T, &crowd, &h.samples, &h.smp_discs, &h.smp_rows, &h.n_walls,
                    &wtrk, &fleet, &gtrk, &h.crowd_waves, &h.n_obstacles) == 11) {
    h.crowd = crowd; h.wtrk_on = wtrk; h.fleet_on = fleet; h.gtrk_on = gtrk;
    const BareboneChoice c = barebone_choose(h);
    std::printf("%%d %%d %%d %%d %%d %%d %%d %%d %%zu %%d\n", (int)c.family, (int)c.discs, c.kmax, (int)c.track_form, (int)c.goal_form,
                c.walls, c.samples, c.chunk, c.lds, (int)c.limit);
  }
  std::printf("%%d %%d\n", kCrowdSamplesMax, kCrowdSampleHitsMax);
  return 0;
}
"""

CROWD, REFUSED = 1, 2
SAMPLES = 3            # kDiscsSamples
NEED_CROWD = 4         # kLimitSamplesNeedCrowd
LDS_AIM = 64 * 1024    # a sample form gives up whole shares of its chunk while it is above this


def layout_lds(T, C, walls, S):
    """[T] double2 | [2][C][64] double | [2][C + walls][64] float2 | [2][C][S][64] uint16 | two words | [S][64] float."""
    return 16 * T + 2 * C * 64 * 8 + 2 * (C + (1 if walls else 0)) * 64 * 8 + 2 * C * S * 64 * 2 + 8 + S * 64 * 4


def chunk_of(W, T, walls, S):
    counters = min(W - 2, 16)
    C = (16 // counters) * counters
    while C > counters and layout_lds(T, C, walls, S) > LDS_AIM:
        C -= counters
    return C


def table():
    rows = []
    for S in (1, 2, 16):
        for T in (37, 100, 200):
            for walls in (0, 1, 2):  # none | static walls (launched as wall tracks of one row) | wall tracks
                for W in (16, 4):
                    C = chunk_of(W, T, walls != 0, S)
                    state = (T, 1, S, 20, T + 1, 3 if walls == 1 else 0, int(walls == 2), 0, 0, W, 7)
                    rows.append((state, (CROWD, SAMPLES, 20, 1, 0, walls, S, C, layout_lds(T, C, walls != 0, S), 0)))
    # fleet and goal track beside the samples; the shared static set (7 discs) rests: kmax is the samples' count
    rows.append(((37, 1, 3, 5, 38, 2, 0, 1, 1, 16, 7), (CROWD, SAMPLES, 5, 1, 1, 2, 3, 14, layout_lds(37, 14, True, 3), 0)))
    # fewer discs than kCrowdMinDiscs, none at all: still the crowd family
    rows.append(((37, 1, 3, 0, 1, 0, 0, 0, 0, 16, 0), (CROWD, SAMPLES, 0, 1, 0, 0, 3, 14, layout_lds(37, 14, False, 3), 0)))
    # crowd mode off: refused
    rows.append(((37, 0, 3, 20, 38, 0, 0, 0, 0, 16, 0), (REFUSED, SAMPLES, 20, 1, 0, 0, 3, 0, 0, NEED_CROWD)))
    return rows


def test_sample_rows_of_the_choice(tmp_path):
    src = tmp_path / "choose.cpp"
    src.write_text(PROGRAM % os.path.abspath(HEADER))
    exe = tmp_path / "choose"
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-o", str(exe), str(src)])
    rows = table()
    text = "".join(" ".join(str(v) for v in state) + "\n" for state, _ in rows)
    out = subprocess.run([str(exe)], input=text.encode(), stdout=subprocess.PIPE, check=True).stdout.decode().splitlines()
    assert len(out) == len(rows) + 1
    assert out[-1].split() == ["16", "65535"]
    for (state, want), line in zip(rows, out):
        got = tuple(int(v) for v in line.split())
        assert got == want, "state %s: chose %s, the table says %s" % (state, got, want)
    # what the issue asks of the layout: S <= 16, T <= 200 and walls fit the 160 KiB of a CU, at either workgroup shape
    assert max(want[8] for _, want in rows) <= 160 * 1024
    # the chunk shrinks at S = 16 for the small workgroup, and not at S = 1
    assert chunk_of(4, 200, True, 16) < 16 and chunk_of(4, 200, True, 1) == 16 and chunk_of(16, 200, True, 16) == 14
