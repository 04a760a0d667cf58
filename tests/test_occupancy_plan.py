"""The grid forms of a crowd launch (crowd_form and crowd_form_legal of csrc/barebone_plan.h), compiled on its own as
tests/test_barebone_form_plan.py compiles the rest: the table of forms is the 32 per ROT of before plus exactly the grid
forms -- TRACKS forms that carry a footprint, 2 wall kinds x goal x rings = 8 per ROT, 48 in the library --, every state of
a handle that holds an occupancy grid maps into them, and a grid beside disc samples, which the hand-over keeps apart, maps
outside the table.  crowd_lds grows by the entry slot, the heading plane and the thresholds."""
import itertools
import os
import subprocess

HEADER = os.path.join(os.path.dirname(__file__), "..", "mppi_numba_amd", "csrc", "barebone_plan.h")

PROGRAM = r"""
#include <cstdio>
#include "%s"
int main() {
  for (int m = 0; m < 192; ++m) {
    CrowdForm f;
    f.tracks = m & 1; f.goal = m & 2; f.samples = m & 4; f.rings = m & 8; f.footprint = m & 16; f.grid = m & 32;
    f.walls = (CrowdWallKind)(m / 64);
    if (crowd_form_legal(f))
      std::printf("legal %%d %%d %%d %%d %%d %%d %%d\n", (int)f.tracks, (int)f.walls, (int)f.goal, (int)f.samples, (int)f.rings, (int)f.footprint,
                  (int)f.grid);
  }
  std::printf("end\n");
  int batched, rot, crowd, own, trk, wtrk, fleet, gtrk, grid;
  for (;;) {
    BareboneHeld h;
    if (std::scanf("%%d %%d %%d %%d %%d %%d %%d %%d %%d %%d %%d %%d %%d %%d %%d %%d %%d %%d %%d %%d %%d", &h.T, &batched, &rot, &crowd, &h.n_obstacles,
                   &own, &h.inst_obs_max, &trk, &h.trk_max, &h.trk_rows, &h.n_walls, &wtrk, &fleet, &gtrk, &h.samples, &h.smp_discs,
                   &h.smp_rows, &h.crowd_waves, &h.footprint, &h.rings, &grid) != 21) break;
    h.batched = batched; h.rot = rot; h.crowd = crowd; h.inst_obs_on = own; h.trk_on = trk; h.wtrk_on = wtrk; h.fleet_on = fleet;
    h.gtrk_on = gtrk; h.grid = grid;
    const BareboneChoice c = barebone_choose(h);
    const CrowdForm f = crowd_form(c, h.rot);
    const size_t want = crowd_lds(h.T, c.chunk, c.walls != 0, c.samples, f.footprint, c.rings, f.grid);
    std::printf("%%d %%d %%d %%d %%d %%d %%d %%d %%d %%d %%d %%d %%d %%d\n", (int)c.family, (int)f.rot, (int)f.tracks, (int)f.walls, (int)f.goal,
                (int)f.samples, (int)f.rings, (int)f.footprint, (int)f.grid, (int)f.disc_row, (int)f.wall_row, (int)crowd_form_legal(f),
                (int)(c.lds == want), (int)c.footprint);
  }
  std::printf("lds %%zu %%zu\n", crowd_lds(37, 14, false, 0, true, 0, true) - crowd_lds(37, 14, false, 0, true),
              crowd_lds(37, 14, true, 0, true, 2, true) - crowd_lds(37, 14, true, 0, true, 2));
  return 0;
}
"""

CROWD = 1
NO_WALLS, STATIC_WALLS, WALL_TRACKS = 0, 1, 2
T, WAVES, K = 37, 16, 70


def states():
    rows = []
    for rot, walls, gtrk, discs, S, F, R in itertools.product((0, 1), ("none", "static", "tracks", "fleet"), (0, 1),
                                                               ("none", "shared", "own", "tracks"), (0, 3), (0, 3), (0, 2)):
        own, trk = discs == "own", discs == "tracks"
        batched = int(own or walls == "fleet")
        held = (T, batched, rot, 1, K if discs == "shared" else 0, int(own), K if own else 0, int(trk), K if trk else 0,
                T + 1 if trk else 0, 3 if walls == "static" else 0, int(walls == "tracks"), int(walls == "fleet"), gtrk, S,
                K if S else 0, T + 1 if S else 0, WAVES, F, R, 1)
        # the rules: a grid form is a TRACKS form with a footprint -- static discs and static walls as tracks of one row
        kind = NO_WALLS if walls == "none" else WALL_TRACKS
        form = (rot, 1, kind, gtrk, int(S > 0), int(R > 0), 1, 1, int(not trk and not S), int(walls == "static"))
        rows.append((held, form, not S, F))
    return rows


def test_the_table_grows_by_the_grid_forms_only(tmp_path):
    src = tmp_path / "form.cpp"
    src.write_text(PROGRAM % os.path.abspath(HEADER))
    exe = tmp_path / "form"
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-o", str(exe), str(src)])
    rows = states()
    text = "".join(" ".join(str(v) for v in held) + "\n" for held, _, _, _ in rows)
    out = subprocess.run([str(exe)], input=text.encode(), stdout=subprocess.PIPE, check=True).stdout.decode().splitlines()
    end = out.index("end")
    table = {tuple(int(v) for v in line.split()[1:]) for line in out[:end]}
    assert len(table) == end
    # today's 32 per ROT, as tests/test_barebone_form_plan.py states them
    before = set()
    for tracks, walls, goal, (samples, rings), foot in itertools.product((0, 1), (0, 1, 2), (0, 1), ((0, 0), (1, 0), (0, 1)), (0, 1)):
        if not (samples or rings or foot) or (tracks and walls != STATIC_WALLS):
            before.add((tracks, walls, goal, samples, rings, foot, 0))
    assert len(before) == 32 and {f for f in table if not f[6]} == before
    grid_forms = {(1, walls, goal, 0, rings, 1, 1) for walls in (NO_WALLS, WALL_TRACKS) for goal in (0, 1) for rings in (0, 1)}
    assert {f for f in table if f[6]} == grid_forms and len(grid_forms) == 8
    assert 3 * 2 * len(grid_forms) == 48  # ((EXACT, ROT) in three combinations) x BATCHED: what the library instantiates on top
    lines = out[end + 1:-1]
    assert len(lines) == len(rows)
    reached = set()
    for (held, form, legal, F), line in zip(rows, lines):
        got = tuple(int(v) for v in line.split())
        assert got[0] == CROWD, "state %s: family %d -- a handle that holds a grid always launches the crowd kernel" % (held, got[0])
        assert got[1:11] == form, "state %s: form %s, the rules say %s" % (held, got[1:11], form)
        assert got[11] == int(legal), "state %s: legal %d" % (held, got[11])
        assert got[13] == F, "the choice keeps the footprint held (the point robot's one-disc body is the launcher's)"
        if legal:
            assert got[12] == 1, "state %s: the LDS of the choice is crowd_lds of the grid form" % (held,)
            assert got[2:9] in table
            reached.add(got[1:9])
    assert reached == {(rot,) + form for rot in (0, 1) for form in grid_forms}
    # the entry slot of positions (8 bytes) and headings (4) in both buffers where there are no walls, and 160 bytes of thresholds
    assert out[-1] == "lds %d %d" % (2 * 64 * (8 + 4) + 160, 160), out[-1]
