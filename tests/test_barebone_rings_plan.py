"""The ring rows of the barebone launch choice (csrc/barebone_plan.h), compiled on its own as
tests/test_barebone_footprint_plan.py compiles it: clearance rings with crowd mode give the crowd family whatever else is
held (no obstacles at all, or two discs that would be the default family's, included) as a TRACKS form with the chunk and
the LDS of the choice; without crowd mode the refusal; the LDS of the ring forms against the layout of
k_rollout_barebone_crowd worked out here; rows without rings as they were."""
import os
import subprocess

HEADER = os.path.join(os.path.dirname(__file__), "..", "mppi_numba_amd", "csrc", "barebone_plan.h")

PROGRAM = r"""
#include <cstdio>
#include "%s"
int main() {
  int crowd, wtrk, gtrk, trk;
  for (;;) {
    BareboneHeld h;
    if (std::scanf("%%d %%d %%d %%d %%d %%d %%d %%d %%d %%d %%d", &h.T, &crowd, &h.n_walls, &wtrk, &gtrk, &h.crowd_waves, &h.n_obstacles,
                   &trk, &h.trk_max, &h.footprint, &h.rings) != 11) break;
    h.crowd = crowd; h.wtrk_on = wtrk; h.gtrk_on = gtrk; h.trk_on = trk; h.trk_rows = trk ? h.T + 1 : 0;
    h.rot = true;
    const BareboneChoice c = barebone_choose(h);
    std::printf("%%d %%d %%d %%d %%d %%d %%d %%zu %%d %%d %%d\n", (int)c.family, (int)c.discs, c.kmax, (int)c.track_form, (int)c.goal_form,
                c.walls, c.chunk, c.lds, (int)c.limit, c.footprint, c.rings);
  }
  BareboneHeld last{37, false, true, true, 3, false, 0, false, 0, 0, 0, false, false, false, 0, 0, 0, 16, 0, 2};  // (rings: the last field)
  std::printf("%%d %%d %%zu %%zu %%zu\n", last.rings, (int)kLimitRingsNeedCrowd, crowd_lds(50, 14, true), crowd_lds(50, 14, true, 0, true),
              crowd_lds(50, 14, true, 2, false, 0));
  return 0;
}
"""

DEFAULT, CROWD, REFUSED = 0, 1, 2
SHARED, TRACKS = 0, 2
NEEDS_CROWD = 6  # kLimitRingsNeedCrowd


def layout_lds(T, C, walls, footprint, rings, S=0):
    """[T] double2 | [2][C][64] double | [2][C + walls][64] float2 | counts: [2][C][64] int, with R rings
    [2][C][1 + R][64] uint16 | two words | a footprint: [2][C + walls][64] float headings and [3][8] double, its rows."""
    slots = C + (1 if walls else 0)
    counts = 2 * C * S * 64 * 2 + S * 64 * 4 if S else (2 * C * (1 + rings) * 64 * 2 if rings else 2 * C * 64 * 4)
    return 16 * T + 2 * C * 64 * 8 + 2 * slots * 64 * 8 + counts + 8 + (2 * slots * 64 * 4 + 3 * 8 * 8 if footprint else 0)


def chunk_of(W):
    counters = min(W - 2, 16)
    return (16 // counters) * counters


def table():
    """state: T crowd n_walls wtrk gtrk waves n_obstacles trk trk_max footprint rings
    choice: family discs kmax track_form goal_form walls chunk lds limit footprint rings"""
    rows = []
    for R in (1, 2, 4):
        for T, W in ((37, 16), (100, 4)):
            C = chunk_of(W)
            for walls in (0, 1, 2):  # none, static walls (kind 1), wall tracks (kind 2)
                held = (3 if walls == 1 else 0, int(walls == 2))
                for F in (0, 3):
                    lds = layout_lds(T, C, walls != 0, F > 0, R)
                    for K in (0, 2, 70):  # no obstacles at all; two discs: the default family without rings
                        rows.append(((T, 1) + held + (0, W, K, 0, 0, F, R), (CROWD, SHARED, K, 1, 0, walls, C, lds, 0, F, R)))
                    # disc tracks and a goal track
                    rows.append(((T, 1) + held + (1, W, 9, 1, 4, F, R), (CROWD, TRACKS, 4, 1, 1, walls, C, lds, 0, F, R)))
    # no crowd mode: refused, whatever else is held
    rows.append(((37, 0, 0, 0, 0, 16, 0, 0, 0, 0, 2), (REFUSED, SHARED, 0, 0, 0, 0, 0, 0, NEEDS_CROWD, 0, 2)))
    rows.append(((37, 0, 0, 0, 0, 16, 2, 0, 0, 0, 4), (REFUSED, SHARED, 0, 0, 0, 0, 0, 0, NEEDS_CROWD, 0, 4)))
    rows.append(((37, 0, 0, 0, 1, 16, 70, 1, 70, 0, 1), (REFUSED, SHARED, 0, 0, 0, 0, 0, 0, NEEDS_CROWD, 0, 1)))
    # without rings: the rows as they were
    rows.append(((37, 1, 0, 0, 0, 16, 2, 0, 0, 0, 0), (DEFAULT, SHARED, 2, 0, 0, 0, 0, 16 * 37 + 16 * 2 + 16 * 2, 0, 0, 0)))
    rows.append(((37, 1, 0, 0, 0, 16, 70, 0, 0, 0, 0), (CROWD, SHARED, 70, 0, 0, 0, 0, 0, 0, 0, 0)))
    rows.append(((37, 1, 3, 0, 0, 16, 0, 0, 0, 0, 0), (CROWD, SHARED, 0, 0, 0, 1, 0, 0, 0, 0, 0)))
    rows.append(((37, 1, 3, 0, 0, 16, 0, 0, 0, 3, 0), (CROWD, SHARED, 0, 1, 0, 1, 14, layout_lds(37, 14, True, True, 0), 0, 3, 0)))
    return rows


def test_ring_rows_of_the_choice(tmp_path):
    src = tmp_path / "choose.cpp"
    src.write_text(PROGRAM % os.path.abspath(HEADER))
    exe = tmp_path / "choose"
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-o", str(exe), str(src)])
    rows = table()
    text = "".join(" ".join(str(v) for v in state) + "\n" for state, _ in rows)
    out = subprocess.run([str(exe)], input=text.encode(), stdout=subprocess.PIPE, check=True).stdout.decode().splitlines()
    assert len(out) == len(rows) + 1
    # rings is BareboneHeld's last field; the defaults of crowd_lds leave the values they gave before there were rings
    assert out[-1].split() == ["2", str(NEEDS_CROWD), str(layout_lds(50, 14, True, False, 0)), str(layout_lds(50, 14, True, True, 0)),
                               str(layout_lds(50, 14, True, False, 0, S=2))]
    for (state, want), line in zip(rows, out):
        got = tuple(int(v) for v in line.split())
        assert got == want, "state %s: chose %s, the table says %s" % (state, got, want)
    # the LDS figures at (T, W) = (37, 16) and (100, 4), four rings, walls and a footprint: 1 + R counts of 16 bits where
    # the 32-bit hits were
    assert chunk_of(16) == 14 and chunk_of(4) == 16
    assert layout_lds(37, 14, True, True, 4) == 16 * 37 + 2 * 14 * 512 + 2 * 15 * 512 + 2 * 14 * 5 * 128 + 8 + 2 * 15 * 256 + 192 == 56088
    assert layout_lds(100, 16, True, True, 4) == 16 * 100 + 2 * 16 * 512 + 2 * 17 * 512 + 2 * 16 * 5 * 128 + 8 + 2 * 17 * 256 + 192 == 64776
    assert layout_lds(37, 14, False, False, 1) == layout_lds(37, 14, False, False, 0)  # (one ring: two 16-bit counts for one int)
    assert layout_lds(100, 16, True, True, 4) - layout_lds(100, 16, True, True, 0) == 2 * 16 * 64 * (5 * 2 - 4)
    assert max(want[7] for _, want in rows) <= 160 * 1024
