"""The form of a crowd launch (crowd_form and crowd_form_legal of csrc/barebone_plan.h), compiled on its own as
tests/test_barebone_plan.py compiles the choice: every choice the crowd family can return, through barebone_choose, maps
to the form the rules restated here give, and into the table of forms; the table has the members the library instantiates
-- its symbols name 192 k_rollout_barebone_crowd kernels: per BATCHED 64 with EXACT (ROT off and on) and 32 without, so 32
per (EXACT, ROT, BATCHED); rings beside samples, which the hand-over keeps apart, map outside the table."""
import itertools
import os
import subprocess

HEADER = os.path.join(os.path.dirname(__file__), "..", "mppi_numba_amd", "csrc", "barebone_plan.h")

PROGRAM = r"""
#include <cstdio>
#include "%s"
int main() {
  // the table itself: every (tracks, walls, goal, samples, rings, footprint) that is legal
  for (int m = 0; m < 96; ++m) {
    CrowdForm f;
    f.tracks = m & 1; f.goal = m & 2; f.samples = m & 4; f.rings = m & 8; f.footprint = m & 16;
    f.walls = (CrowdWallKind)(m / 32);
    if (crowd_form_legal(f))
      std::printf("legal %%d %%d %%d %%d %%d %%d\n", (int)f.tracks, (int)f.walls, (int)f.goal, (int)f.samples, (int)f.rings, (int)f.footprint);
  }
  std::printf("end\n");
  int batched, rot, crowd, own, trk, wtrk, fleet, gtrk;
  for (;;) {
    BareboneHeld h;
    if (std::scanf("%%d %%d %%d %%d %%d %%d %%d %%d %%d %%d %%d %%d %%d %%d %%d %%d %%d %%d %%d %%d", &h.T, &batched, &rot, &crowd, &h.n_obstacles,
                   &own, &h.inst_obs_max, &trk, &h.trk_max, &h.trk_rows, &h.n_walls, &wtrk, &fleet, &gtrk, &h.samples, &h.smp_discs,
                   &h.smp_rows, &h.crowd_waves, &h.footprint, &h.rings) != 20) break;
    h.batched = batched; h.rot = rot; h.crowd = crowd; h.inst_obs_on = own; h.trk_on = trk; h.wtrk_on = wtrk; h.fleet_on = fleet;
    h.gtrk_on = gtrk;
    const BareboneChoice c = barebone_choose(h);
    const CrowdForm f = crowd_form(c, h.rot);
    std::printf("%%d %%d %%d %%d %%d %%d %%d %%d %%d %%d %%d\n", (int)c.family, (int)f.rot, (int)f.tracks, (int)f.walls, (int)f.goal, (int)f.samples,
                (int)f.rings, (int)f.footprint, (int)f.disc_row, (int)f.wall_row, (int)crowd_form_legal(f));
  }
  return 0;
}
"""

CROWD = 1
NO_WALLS, STATIC_WALLS, WALL_TRACKS = 0, 1, 2
FORMS_PER_ROT = 32  # the library's symbols: 192 = (64 + 32) * 2; 64 = 2 * 32 (ROT), 32 without EXACT (no ROT)

T, WAVES, K = 37, 16, 70


def states():
    """(held, expectation): everything a handle in crowd mode can hold, the forms of the default family left out.
    held: the fields of BareboneHeld in their order."""
    rows = []
    for rot, walls, gtrk, discs, S, F, R in itertools.product((0, 1), ("none", "static", "tracks", "fleet"), (0, 1),
                                                               ("none", "shared", "own", "tracks"), (0, 3), (0, 3), (0, 2)):
        extra = bool(S or F or R)
        if discs == "none" and walls == "none" and not extra:
            continue  # (nothing for the crowd kernel to do: the default family)
        own, trk = discs == "own", discs == "tracks"
        batched = int(own or walls == "fleet")
        held = (T, batched, rot, 1, K if discs == "shared" else 0, int(own), K if own else 0, int(trk), K if trk else 0,
                T + 1 if trk else 0, 3 if walls == "static" else 0, int(walls == "tracks"), int(walls == "fleet"), gtrk, S,
                K if S else 0, T + 1 if S else 0, WAVES, F, R)
        # the rules: samples, a footprint and rings are TRACKS forms -- static discs and static walls as tracks of one row
        kind = NO_WALLS if walls == "none" else (WALL_TRACKS if walls in ("tracks", "fleet") or extra else STATIC_WALLS)
        form = (rot, int(trk or extra), kind, gtrk, int(S > 0), int(R > 0), int(F > 0),
                int(extra and not trk and not S), int(extra and walls == "static"))
        rows.append((held, form, not (S and R)))
    return rows


def test_every_crowd_choice_maps_into_the_table_of_forms(tmp_path):
    src = tmp_path / "form.cpp"
    src.write_text(PROGRAM % os.path.abspath(HEADER))
    exe = tmp_path / "form"
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-o", str(exe), str(src)])
    rows = states()
    text = "".join(" ".join(str(v) for v in held) + "\n" for held, _, _ in rows)
    out = subprocess.run([str(exe)], input=text.encode(), stdout=subprocess.PIPE, check=True).stdout.decode().splitlines()
    end = out.index("end")
    table = {tuple(int(v) for v in line.split()[1:]) for line in out[:end]}
    assert len(table) == end == FORMS_PER_ROT
    # the table, said once more: 12 plain forms, and 20 TRACKS forms without CrowdWalls under samples, rings or a footprint
    want = set()
    for tracks, walls, goal, (samples, rings), foot in itertools.product((0, 1), (0, 1, 2), (0, 1), ((0, 0), (1, 0), (0, 1)), (0, 1)):
        if not (samples or rings or foot) or (tracks and walls != STATIC_WALLS):
            want.add((tracks, walls, goal, samples, rings, foot))
    assert table == want
    lines = out[end + 1:]
    assert len(lines) == len(rows)
    reached = set()
    for (held, form, legal), line in zip(rows, lines):
        got = tuple(int(v) for v in line.split())
        assert got[0] == CROWD, "state %s: family %d" % (held, got[0])
        assert got[1:10] == form, "state %s: form %s, the rules say %s" % (held, got[1:10], form)
        assert got[10] == int(legal), "state %s: legal %d" % (held, got[10])
        if legal:
            assert got[2:8] in table
            reached.add(got[1:8])
    # every form of the table is some handle's, with ROT off and on: the 64 per BATCHED of exact math, 32 of them without it
    assert reached == {(rot,) + form for rot in (0, 1) for form in table}
    assert len(reached) == 2 * FORMS_PER_ROT and len({r for r in reached if r[0] == 0}) == FORMS_PER_ROT
