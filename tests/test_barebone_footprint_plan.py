"""The footprint rows of the barebone launch choice (csrc/barebone_plan.h), compiled on its own as
tests/test_barebone_samples_plan.py compiles it: a footprint with crowd mode gives the crowd family whatever else is held
(no discs and no walls included), without crowd mode the refusal; the LDS of the footprint forms against the layout of
k_rollout_barebone_crowd worked out here, with and without walls and samples; rows without a footprint as they were."""
import os
import subprocess

HEADER = os.path.join(os.path.dirname(__file__), "..", "mppi_numba_amd", "csrc", "barebone_plan.h")

PROGRAM = r"""
#include <cstdio>
#include "%s"
int main() {
  int crowd, wtrk, fleet, gtrk, trk;
  for (;;) {
    BareboneHeld h;
    if (std::scanf("%%d %%d %%d %%d %%d %%d %%d %%d %%d %%d %%d %%d %%d %%d", &h.T, &crowd, &h.samples, &h.smp_discs, &h.smp_rows, &h.n_walls,
                   &wtrk, &fleet, &gtrk, &h.crowd_waves, &h.n_obstacles, &trk, &h.trk_max, &h.footprint) != 14) break;
    h.crowd = crowd; h.wtrk_on = wtrk; h.fleet_on = fleet; h.gtrk_on = gtrk; h.trk_on = trk; h.trk_rows = trk ? h.T + 1 : 0;
    h.rot = true;
    const BareboneChoice c = barebone_choose(h);
    std::printf("%%d %%d %%d %%d %%d %%d %%d %%d %%zu %%d %%d\n", (int)c.family, (int)c.discs, c.kmax, (int)c.track_form, (int)c.goal_form,
                c.walls, c.samples, c.chunk, c.lds, (int)c.limit, c.footprint);
  }
  BareboneHeld by_name;  // (the last field, with a default)
  by_name.footprint = 3;
  std::printf("%%d %%d %%zu %%zu %%d\n", by_name.footprint, (int)kLimitFootprintNeedsCrowd, crowd_lds(50, 14, true), crowd_lds(50, 14, true, 2),
              crowd_chunk(16) * 100 + crowd_chunk(4));
  return 0;
}
"""

DEFAULT, CROWD, REFUSED = 0, 1, 2
SHARED, TRACKS, SAMPLES = 0, 2, 3
NEEDS_CROWD = 5        # kLimitFootprintNeedsCrowd
LDS_AIM = 64 * 1024


def layout_lds(T, C, walls, S, footprint):
    """[T] double2 | [2][C][64] double | [2][C + walls][64] float2 | hits: [2][C][64] int, or [2][C][S][64] uint16 and
    [S][64] float | two words | a footprint: [2][C + walls][64] float headings and [3][8] double, its rows."""
    slots = C + (1 if walls else 0)
    hits = 2 * C * S * 64 * 2 + S * 64 * 4 if S else 2 * C * 64 * 4
    return 16 * T + 2 * C * 64 * 8 + 2 * slots * 64 * 8 + hits + 8 + (2 * slots * 64 * 4 + 3 * 8 * 8 if footprint else 0)


def chunk_of(W, T, walls, S, footprint):
    counters = min(W - 2, 16)
    C = (16 // counters) * counters
    while S and C > counters and layout_lds(T, C, walls, S, footprint) > LDS_AIM:
        C -= counters
    return C


def table():
    """state: T crowd S smp_discs smp_rows n_walls wtrk fleet gtrk waves n_obstacles trk trk_max footprint
    choice: family discs kmax track_form goal_form walls samples chunk lds limit footprint"""
    rows = []
    for F in (1, 3, 8):
        for T in (37, 100):
            for walls in (0, 1, 2):
                for W in (16, 4):
                    C = chunk_of(W, T, walls != 0, 0, True)
                    for K in (0, 3, 70):  # static discs: the crowd family also below kCrowdMinDiscs and with none
                        state = (T, 1, 0, 0, 0, 3 if walls == 1 else 0, int(walls == 2), 0, 0, W, K, 0, 0, F)
                        rows.append((state, (CROWD, SHARED, K, 1, 0, walls, 0, C, layout_lds(T, C, walls != 0, 0, True), 0, F)))
                    state = (T, 1, 0, 0, 0, 3 if walls == 1 else 0, int(walls == 2), 0, 1, W, 9, 1, 4, F)  # tracks and a goal track
                    rows.append((state, (CROWD, TRACKS, 4, 1, 1, walls, 0, C, layout_lds(T, C, walls != 0, 0, True), 0, F)))
                    for S in (3, 16):
                        Cs = chunk_of(W, T, walls != 0, S, True)
                        state = (T, 1, S, 20, T + 1, 3 if walls == 1 else 0, int(walls == 2), 0, 0, W, 7, 0, 0, F)
                        rows.append((state, (CROWD, SAMPLES, 20, 1, 0, walls, S, Cs, layout_lds(T, Cs, walls != 0, S, True), 0, F)))
    # no crowd mode: refused, whatever else is held
    rows.append(((37, 0, 0, 0, 0, 0, 0, 0, 0, 16, 0, 0, 0, 3), (REFUSED, SHARED, 0, 0, 0, 0, 0, 0, 0, NEEDS_CROWD, 3)))
    rows.append(((37, 0, 3, 20, 38, 0, 0, 0, 0, 16, 0, 0, 0, 8), (REFUSED, SHARED, 0, 0, 0, 0, 0, 0, 0, NEEDS_CROWD, 8)))
    # without a footprint: the rows as they were (tests/test_barebone_plan.py and test_barebone_samples_plan.py hold the rest)
    rows.append(((37, 1, 0, 0, 0, 0, 0, 0, 0, 16, 3, 0, 0, 0), (DEFAULT, SHARED, 3, 0, 0, 0, 0, 0, 16 * 37 + 16 * 3 + 16 * 4, 0, 0)))
    rows.append(((37, 1, 0, 0, 0, 0, 0, 0, 0, 16, 70, 0, 0, 0), (CROWD, SHARED, 70, 0, 0, 0, 0, 0, 0, 0, 0)))
    rows.append(((37, 1, 0, 0, 0, 3, 0, 0, 0, 16, 0, 0, 0, 0), (CROWD, SHARED, 0, 0, 0, 1, 0, 0, 0, 0, 0)))
    rows.append(((37, 1, 3, 20, 38, 3, 0, 0, 0, 16, 7, 0, 0, 0), (CROWD, SAMPLES, 20, 1, 0, 1, 3, 14, layout_lds(37, 14, True, 3, False), 0, 0)))
    return rows


def test_footprint_rows_of_the_choice(tmp_path):
    src = tmp_path / "choose.cpp"
    src.write_text(PROGRAM % os.path.abspath(HEADER))
    exe = tmp_path / "choose"
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-o", str(exe), str(src)])
    rows = table()
    text = "".join(" ".join(str(v) for v in state) + "\n" for state, _ in rows)
    out = subprocess.run([str(exe)], input=text.encode(), stdout=subprocess.PIPE, check=True).stdout.decode().splitlines()
    assert len(out) == len(rows) + 1
    # the defaults of crowd_lds and crowd_chunk leave the values they gave before there was a footprint
    assert out[-1].split() == ["3", str(NEEDS_CROWD), str(layout_lds(50, 14, True, 0, False)), str(layout_lds(50, 14, True, 2, False)), "1416"]
    for (state, want), line in zip(rows, out):
        got = tuple(int(v) for v in line.split())
        assert got == want, "state %s: chose %s, the table says %s" % (state, got, want)
    # the heading plane and the rows are what a footprint adds: 2 * slots * 64 * 4 + 192 bytes, and everything fits a CU
    assert layout_lds(100, 14, True, 0, True) - layout_lds(100, 14, True, 0, False) == 2 * 15 * 256 + 192
    assert max(want[8] for _, want in rows) <= 160 * 1024
    # a sample form's chunk counts the heading plane: S = 16 at T = 100 with walls, four waves
    assert chunk_of(4, 100, True, 16, True) <= chunk_of(4, 100, True, 16, False) < 16
