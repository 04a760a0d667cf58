"""The launch choice of the barebone mode (csrc/barebone_plan.h: barebone_choose, barebone_lds) against a table.

The header is plain C++: a small host program compiled with g++ reads states and prints choices.  The expected rows were
written by reading the launch ladders this function replaced (the classic single launch, the batch launch, the track and
the goal launches and crowd_launch), not by running it; every default-family row is checked once more against the LDS
layout of k_rollout_barebone worked out here.
"""
import os
import subprocess


HEADER = os.path.join(os.path.dirname(__file__), "..", "mppi_numba_amd", "csrc", "barebone_plan.h")

PROGRAM = r"""
#include <cstdio>
#include "%s"
int main() {
  BareboneHeld h;
  int batched, rot, crowd, inst, trk, wtrk, fleet, gtrk;
  while (std::scanf("%%d %%d %%d %%d %%d %%d %%d %%d %%d %%d %%d %%d %%d %%d", &h.T, &batched, &rot, &crowd, &h.n_obstacles, &inst,
                    &h.inst_obs_max, &trk, &h.trk_max, &h.trk_rows, &h.n_walls, &wtrk, &fleet, &gtrk) == 14) {
    h.batched = batched; h.rot = rot; h.crowd = crowd; h.inst_obs_on = inst; h.trk_on = trk;
    h.wtrk_on = wtrk; h.fleet_on = fleet; h.gtrk_on = gtrk;
    const BareboneChoice c = barebone_choose(h);
    std::printf("%%d %%d %%d %%d %%d %%d %%d %%zu %%d\n", (int)c.family, (int)c.discs, c.kmax, c.kd, (int)c.track_form,
                (int)c.goal_form, c.walls, c.lds, (int)c.limit);
  }
  return 0;
}
"""

DEFAULT, CROWD, REFUSED = 0, 1, 2
SHARED, OWN, TRACKS = 0, 1, 2


def held(T=8, batched=0, rot=0, crowd=0, discs=0, own=None, tracks=None, walls=0, wtrk=0, fleet=0, goal=0):
    """A state as the program reads it.  own: the largest per-problem static set; tracks: (largest count, rows)."""
    trk_max, trk_rows = tracks if tracks is not None else (0, 0)
    return (T, batched, rot, crowd, discs, int(own is not None), own or 0, int(tracks is not None), trk_max, trk_rows,
            walls, wtrk, fleet, goal)


def choice(family, discs=SHARED, kmax=0, kd=-1, track=0, goal=0, walls=0, lds=0, limit=0):
    return (family, discs, kmax, kd, track, goal, walls, lds, limit)


def layout_lds(T, slots, track, goal, spare=0):
    """[T] double2 | [slots] float4 (a row per step in the track forms; a row has one slot at the least) | goal: [T] float2."""
    row = 16 * max(1, slots)
    return 16 * T + (T * row if track else row) + (8 * T if goal else 0) + 16 * spare


# K = 0 .. 5 static discs at T = 8: the KD form under rotation, and the dynamic LDS of the four static launches
KD_ROT = [2, 2, 2, 4, 4, -1]
LDS_SINGLE_ROT = [176, 176, 192, 240, 256, 208]  # 16 T + 16 max(1, K) and the classic launch's KD slots on top
LDS_BATCH_ROT = [160, 160, 160, 192, 192, 208]   # 16 T + 16 max(1, KD or K)
LDS_LOOP = [144, 144, 160, 176, 192, 208]        # 16 T + 16 max(1, K)


def table():
    rows = []
    for K in range(6):
        for batched in (0, 1):
            rot_lds = (LDS_BATCH_ROT if batched else LDS_SINGLE_ROT)[K]
            rows.append((held(batched=batched, rot=1, discs=K), choice(DEFAULT, kmax=K, kd=KD_ROT[K], lds=rot_lds)))
            rows.append((held(batched=batched, rot=0, discs=K), choice(DEFAULT, kmax=K, kd=-1, lds=LDS_LOOP[K])))
            # crowd mode: the default family up to 4 discs, the crowd family from 5 on
            on = choice(DEFAULT, kmax=K, kd=KD_ROT[K], lds=rot_lds) if K <= 4 else choice(CROWD, kmax=K)
            rows.append((held(batched=batched, rot=1, crowd=1, discs=K), on))
    # a long horizon: the padded row of 2 slots needs 48 T (56 T with a goal) > 64 KiB, the problem's own row fits
    rows.append((held(T=1400, rot=1, tracks=(1, 3)), choice(DEFAULT, TRACKS, 1, -1, track=1, lds=44800)))
    rows.append((held(T=1400, rot=1, discs=1, goal=1), choice(DEFAULT, SHARED, 1, -1, track=1, goal=1, lds=56000)))
    rows.append((held(T=1400, rot=1, batched=1, tracks=(1, 3), goal=1), choice(DEFAULT, TRACKS, 1, -1, track=1, goal=1, lds=56000)))
    # ... and sets whose own row does not fit: refused, or the crowd family's
    rows.append((held(T=1400, rot=1, tracks=(3, 3)), choice(REFUSED, TRACKS, 3, -1, track=1, lds=89600, limit=2)))
    rows.append((held(T=1400, rot=1, discs=3, goal=1), choice(REFUSED, SHARED, 3, -1, track=1, goal=1, lds=100800, limit=3)))
    rows.append((held(T=1400, rot=1, crowd=1, tracks=(3, 3)), choice(CROWD, TRACKS, 3, track=1)))
    rows.append((held(discs=4096), choice(REFUSED, kmax=4096, lds=128 + 65536, limit=1)))
    rows.append((held(discs=4096, batched=1, rot=1), choice(REFUSED, kmax=4096, lds=128 + 65536, limit=1)))
    rows.append((held(discs=4096, crowd=1), choice(CROWD, kmax=4096)))
    # walls are the crowd kernel's alone
    rows.append((held(crowd=1, walls=3), choice(CROWD, walls=1)))
    rows.append((held(crowd=1, wtrk=1), choice(CROWD, walls=2)))
    rows.append((held(crowd=1, batched=1, fleet=1), choice(CROWD, walls=2)))
    rows.append((held(crowd=1, walls=3, wtrk=1), choice(CROWD, walls=2)))
    rows.append((held(crowd=1, batched=1, walls=3, fleet=1, goal=1, discs=2), choice(CROWD, kmax=2, track=1, goal=1, walls=2)))
    # disc tracks; a goal track over static discs (tracks of one row), over disc tracks, over a per-problem static set
    rows.append((held(rot=1, tracks=(2, 5)), choice(DEFAULT, TRACKS, 2, 2, track=1, lds=384)))
    rows.append((held(rot=0, batched=1, tracks=(2, 5)), choice(DEFAULT, TRACKS, 2, -1, track=1, lds=384)))
    rows.append((held(rot=1, discs=2, goal=1), choice(DEFAULT, SHARED, 2, 2, track=1, goal=1, lds=448)))
    rows.append((held(rot=1, batched=1, discs=2, goal=1), choice(DEFAULT, SHARED, 2, 2, track=1, goal=1, lds=448)))
    rows.append((held(rot=1, batched=1, discs=7, tracks=(3, 5), goal=1), choice(DEFAULT, TRACKS, 3, 4, track=1, goal=1, lds=704)))
    rows.append((held(rot=1, batched=1, discs=7, own=1, goal=1), choice(DEFAULT, OWN, 1, 2, track=1, goal=1, lds=448)))
    rows.append((held(rot=1, discs=7, own=1), choice(DEFAULT, OWN, 1, 2, lds=176)))  # (one problem given its own set)
    return rows


def test_barebone_choose_matches_the_table(tmp_path):
    src = tmp_path / "choose.cpp"
    src.write_text(PROGRAM % os.path.abspath(HEADER))
    exe = tmp_path / "choose"
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-o", str(exe), str(src)])
    rows = table()
    text = "".join(" ".join(str(v) for v in state) + "\n" for state, _ in rows)
    out = subprocess.run([str(exe)], input=text.encode(), stdout=subprocess.PIPE, check=True).stdout.decode().splitlines()
    assert len(out) == len(rows)
    for (state, want), line in zip(rows, out):
        got = tuple(int(v) for v in line.split())
        assert got == want, "state %s: chose %s, the table says %s" % (state, got, want)
        family, _, kmax, kd, track, goal, _, lds, _ = want
        if family == CROWD:
            continue
        T, batched = state[0], state[1]
        if track or batched:
            assert lds == layout_lds(T, kd if kd > 0 else kmax, track, goal), state
        else:  # the classic single launch of a static set asks for its KD slots on top
            assert lds == layout_lds(T, kmax, False, False, spare=max(kd, 0)), state
