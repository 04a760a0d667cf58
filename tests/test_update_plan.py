"""How the weights of a rollout launch become the next u (csrc/update_plan.h: update_choose, next_rollout_takes and what
they are made of) against a table.

The header is plain C++: a small host program compiled with g++ reads states and prints choices.  The expected rows were
written by reading the code these functions replaced (launch_update, launch_update_local, next_rollout_applies_updates,
p2p_usable, next_rollout_reduces_tiles, launch_rollout's settling of a pending update and launch_iteration's
beside_update), not by running them; the LDS bytes of the row kernel are worked out a second time here.

The base state is bench.py's c2 at N = 8192 in the middle of a loop: one GPU, deterministic dynamics, T = 100, the
time-parallel kernel on tiles of 32 before and after this update, another iteration to follow.  Five rows keep answers
that look inconsistent on purpose (TRAPS): they are today's, and a change to any of them is a change of behaviour.
"""
import os
import subprocess

import pytest

HEADER = os.path.join(os.path.dirname(__file__), "..", "mppi_numba_amd", "csrc", "update_plan.h")

FIELDS = ["mode", "world_size", "has_comm", "m_count", "B", "inst_set", "n_local", "n_inst", "inst_tiles", "T", "rng",
          "debug_flags", "fold_off", "p2p_on", "graph_on", "stream_flags_off", "flags_env_off", "flag_words",
          "prof", "defer_exchange", "may_leave_apply", "mirror_now", "want_next", "have_noise", "side_stream_pays",
          "scan_packets_fresh", "tile_packets_fresh", "scan_tile", "next_scan", "next_tile"]

PROGRAM = r"""
#include <cstdio>
#include <cstring>
#include "%s"
int main() {
  for (;;) {
    UpdateHeld h;
    std::memset(&h, 0, sizeof(h));
    int* f = &h.mode;  // (the struct is %d ints, in the order of FIELDS)
    static_assert(sizeof(UpdateHeld) == %d * sizeof(int), "UpdateHeld has a field the test does not know");
    int got = 0;
    while (got < %d && std::scanf("%%d", f + got) == 1) ++got;
    if (got != %d) break;
    const UpdateChoice c = update_choose(h);
    const RolloutTakes t = next_rollout_takes(h);
    const UpdateChoice s = update_local_launch(h, kUpdateLocalApply);  // (what settles tile packets nobody will reduce)
    std::printf("route=%%d kernel=%%d apply_here=%%d peers_ride=%%d tile_weights_first=%%d from_costs=%%d slim=%%d rows_per_wg=%%d "
                "per_problem_tiles=%%d grid_x=%%d grid_y=%%d block=%%d lds=%%zu lds_launch=%%zu beside_update=%%d ",
                (int)c.route, (int)c.kernel, (int)c.apply_here, (int)c.peers_ride, (int)c.tile_weights_first, (int)c.from_costs,
                (int)c.slim, c.rows_per_wg, c.per_problem_tiles, c.grid_x, c.grid_y, c.block, c.lds, c.lds_launch,
                (int)c.beside_update);
    std::printf("applies_packets=%%d reduces_tiles=%%d keeps_packets=%%d p2p_usable=%%d settle_kernel=%%d settle_peers_ride=%%d "
                "settle_apply_here=%%d\n", (int)t.applies_packets, (int)t.reduces_tiles, (int)rollout_keeps_pending_packets(h),
                (int)update_p2p_usable(h), (int)s.kernel, (int)s.peers_ride, (int)s.apply_here);
  }
  return 0;
}
"""

DET, SPEED, TDM, BAREBONE = range(4)
PHILOX, XOROSHIRO = 0, 1
NO_FOLDED_APPLY, NO_REDUCE_FOLD = 256, 512
LEAVE_TILES, LOCAL_APPLY, PACKET_ONLY, GATHER_APPLY, GATHER_LEAVE_APPLY = range(5)
NO_KERNEL, COMBINE, ROWS = range(3)
LDS_MAX = 60 * 1024  # the row kernel's tile arrays


def held(**over):
    """c2, N = 8192, in the middle of a loop on one GPU."""
    s = dict(mode=DET, world_size=1, has_comm=0, m_count=1, B=1, inst_set=0, n_local=8192, n_inst=None, inst_tiles=None, T=100,
             rng=PHILOX, debug_flags=0, fold_off=0, p2p_on=0, graph_on=0, stream_flags_off=0, flags_env_off=0, flag_words=1,
             prof=0, defer_exchange=0, may_leave_apply=1, mirror_now=0, want_next=1, have_noise=0, side_stream_pays=0,
             scan_packets_fresh=1, tile_packets_fresh=0, scan_tile=32, next_scan=1, next_tile=32)
    assert set(over) <= set(s), over
    s.update(over)
    if s["n_inst"] is None:
        s["n_inst"] = s["n_local"] // s["B"]
    if s["inst_tiles"] is None:
        s["inst_tiles"] = (s["n_inst"] + 63) // 64
    return s


def sharded(world=2, **over):
    """... control samples sharded over `world` ranks with a communicator"""
    return held(world_size=world, has_comm=1, **over)


def rows_state(**over):
    """a rollout kernel that leaves costs (and perhaps tile weights), no tile packets: the row kernel's states; c2 at
    N = 65536 (k_rollout_fused: four waves per CU, the second stream beside the rollout pays)"""
    base = dict(n_local=65536, scan_packets_fresh=0, next_scan=0, next_tile=0, side_stream_pays=1)
    base.update(over)
    return held(**base)


def c5(**over):
    """bench.py's c5: 64 problems of 4096 rollouts, k_rollout_fused (tile weights from its epilogue); 16 rollout waves
    per CU, so the second stream beside the rollout does not pay and the generator runs beside the update"""
    base = dict(B=64, inst_set=1, n_local=262144, tile_packets_fresh=1, scan_packets_fresh=0, next_scan=0, next_tile=0)
    base.update(over)
    return held(**base)


# ---- expected choices ---------------------------------------------------------------------------------------------------
def combine(route, tiles, T=100, B=1, peers_ride=0):
    return dict(route=route, kernel=COMBINE, apply_here=int(route == LOCAL_APPLY), peers_ride=peers_ride, per_problem_tiles=tiles,
                grid_x=T, grid_y=B, block=64, beside_update=0, slim=0)


def rows(route, inst_tiles, T=100, B=1, from_costs=1, tile_weights_first=0, slim=0):
    many = T * B >= 2048
    lds = 4 * inst_tiles * (2 if from_costs else 1)
    return dict(route=route, kernel=ROWS, apply_here=int(route == LOCAL_APPLY), from_costs=from_costs,
                tile_weights_first=tile_weights_first, rows_per_wg=4 if many else 1, grid_x=(T + 3) // 4 if many else T, grid_y=B,
                block=256 if slim else 1024, lds=lds, lds_launch=max(lds, LDS_MAX) if slim else lds, slim=slim, beside_update=slim,
                peers_ride=0)


LEAVE = dict(route=LEAVE_TILES, kernel=NO_KERNEL, beside_update=0)
C5_ROWS = rows(LOCAL_APPLY, 64, B=64, from_costs=0, slim=1)
C5_PLAIN = rows(LOCAL_APPLY, 64, B=64, from_costs=0)

ROUTES = [
    (held(), dict(LEAVE, applies_packets=1, reduces_tiles=1, keeps_packets=1, p2p_usable=0)),
    (held(may_leave_apply=0), combine(LOCAL_APPLY, 256)),
    (held(defer_exchange=1), combine(PACKET_ONLY, 256)),
    (sharded(), dict(combine(GATHER_LEAVE_APPLY, 256), applies_packets=1, reduces_tiles=0)),
    (sharded(may_leave_apply=0), combine(GATHER_APPLY, 256)),
    (sharded(defer_exchange=1), combine(PACKET_ONLY, 256)),
    # world_size > 1 without a communicator is the collective route too (the launcher refuses it there)
    (held(world_size=2, may_leave_apply=0), combine(GATHER_APPLY, 256)),
    # the stage-level calls: nothing of launch_iteration's set
    (held(may_leave_apply=0, want_next=0), combine(LOCAL_APPLY, 256)),
    (rows_state(may_leave_apply=0, want_next=0), rows(LOCAL_APPLY, 1024)),
    (rows_state(defer_exchange=1), rows(PACKET_ONLY, 1024)),
    (sharded(n_local=65536, scan_packets_fresh=0, next_scan=0, next_tile=0), dict(rows(GATHER_APPLY, 1024), applies_packets=0)),
]

TRAPS = [
    # 1. the combine launch carries the peer exchange when apply_here && p2p_on && world_size > 1 -- weaker than
    #    p2p_usable: here the next launch is another kernel family (p2p not usable), and the launch that settles the
    #    tile packets still exchanges; so does the local route of sharded samples
    (held(world_size=2, p2p_on=1, next_scan=0, next_tile=0),
     dict(combine(GATHER_APPLY, 256), p2p_usable=0, settle_kernel=COMBINE, settle_peers_ride=1, settle_apply_here=1)),
    (held(world_size=2, p2p_on=1, m_count=2), dict(combine(LOCAL_APPLY, 256, peers_ride=1), p2p_usable=0)),
    (held(world_size=2, p2p_on=1, defer_exchange=1), dict(combine(PACKET_ONLY, 256, peers_ride=0), p2p_usable=1)),
    # 2. launch_rollout keeps pending rank packets on (mode == DET && scan kernel) alone: a debug flag or a mirror that
    #    takes applies_packets away does not take packets already left away from the launch
    (sharded(debug_flags=NO_FOLDED_APPLY), dict(combine(GATHER_APPLY, 256), applies_packets=0, keeps_packets=1)),
    (sharded(mirror_now=1), dict(combine(GATHER_APPLY, 256), applies_packets=0, keeps_packets=1)),
    (sharded(world=17), dict(combine(GATHER_APPLY, 256), applies_packets=0, keeps_packets=1)),
    (sharded(next_scan=0, next_tile=0), dict(combine(GATHER_APPLY, 256), applies_packets=0, keeps_packets=0)),
    # 3. reduces_tiles admits the speed-map mode; the packet fold and the peer exchange admit DET only
    (held(mode=SPEED), dict(LEAVE, applies_packets=0, reduces_tiles=1, keeps_packets=0)),
    (sharded(mode=SPEED), dict(combine(GATHER_APPLY, 256), applies_packets=0, reduces_tiles=0)),
    (held(mode=SPEED, world_size=2, p2p_on=1), dict(combine(GATHER_APPLY, 256), p2p_usable=0, reduces_tiles=0)),
    # 4. a communicator on a single rank takes the collective route
    (held(has_comm=1), dict(combine(GATHER_LEAVE_APPLY, 256), applies_packets=1, reduces_tiles=0)),
    (held(has_comm=1, may_leave_apply=0), combine(GATHER_APPLY, 256)),
    # 5. with m_count > 1 the update is local whatever the world size (CVaR mode: the row kernel from the costs)
    (sharded(mode=TDM, m_count=2, n_local=1024, scan_packets_fresh=0, next_scan=0, next_tile=0),
     dict(rows(LOCAL_APPLY, 16), applies_packets=0, reduces_tiles=0)),
    (held(mode=TDM, world_size=2, m_count=2, n_local=1024, scan_packets_fresh=0, next_scan=0, next_tile=0), rows(LOCAL_APPLY, 16)),
]

FOLDS = [
    # a profiled iteration and the last one of a call leave nothing to the next launch
    (held(prof=1), dict(combine(LOCAL_APPLY, 256), reduces_tiles=1)),
    (sharded(prof=1), dict(combine(GATHER_APPLY, 256), applies_packets=1)),
    # the debug flags and the fold's own fail-soft switch
    (held(debug_flags=NO_FOLDED_APPLY), dict(combine(LOCAL_APPLY, 256), applies_packets=0, reduces_tiles=0)),
    (held(debug_flags=NO_REDUCE_FOLD), dict(combine(LOCAL_APPLY, 256), applies_packets=1, reduces_tiles=0)),
    (sharded(debug_flags=NO_REDUCE_FOLD), dict(combine(GATHER_LEAVE_APPLY, 256), applies_packets=1)),
    (held(fold_off=1), dict(combine(LOCAL_APPLY, 256), applies_packets=1, reduces_tiles=0)),
    (sharded(fold_off=1), dict(combine(GATHER_LEAVE_APPLY, 256), applies_packets=1)),
    # the last update of solve() writes the host mirror: an update launch of its own
    (held(mirror_now=1), dict(combine(LOCAL_APPLY, 256), applies_packets=0, reduces_tiles=0)),
    # the next launch on other tiles than the last one (MPPI_DEBUG_SCAN_FULL_TILES set in between)
    (held(scan_tile=32, next_tile=64), dict(combine(LOCAL_APPLY, 256), reduces_tiles=0)),
    (held(scan_tile=64, next_tile=32), dict(combine(LOCAL_APPLY, 128), reduces_tiles=0)),
    # another kernel family next; a batched handle
    (held(next_scan=0, next_tile=0), dict(combine(LOCAL_APPLY, 256), applies_packets=0, reduces_tiles=0)),
    (held(B=64, inst_set=1, n_local=4096), dict(combine(LOCAL_APPLY, 2, B=64), applies_packets=0, reduces_tiles=0)),
    # 4 * tiles >= T: T = 100 with 25 and with 24 tiles of 32
    (held(n_local=800), dict(LEAVE, reduces_tiles=1)),
    (held(n_local=768), dict(combine(LOCAL_APPLY, 24), reduces_tiles=0)),
    # the peer exchange: 2 and 16 ranks fold like one GPU, 17 do not; not after another kernel family's launch
    (held(world_size=2, p2p_on=1), dict(LEAVE, p2p_usable=1, reduces_tiles=1, applies_packets=1)),
    (held(world_size=2, p2p_on=1, may_leave_apply=0), dict(combine(LOCAL_APPLY, 256, peers_ride=1), p2p_usable=1)),
    (held(world_size=16, p2p_on=1), dict(LEAVE, p2p_usable=1)),
    (held(world_size=17, p2p_on=1), dict(combine(GATHER_APPLY, 256), p2p_usable=0, reduces_tiles=0, applies_packets=0)),
    (held(world_size=2, p2p_on=1, n_local=65536, scan_packets_fresh=0), dict(rows(GATHER_LEAVE_APPLY, 1024), p2p_usable=1)),
    (held(world_size=1, p2p_on=1), dict(LEAVE, p2p_usable=0)),
]

FORMS = [
    # rows per workgroup: T * B at 2047 and 2048
    (rows_state(T=2047), rows(LOCAL_APPLY, 1024, T=2047)),
    (rows_state(T=2048), rows(LOCAL_APPLY, 1024, T=2048)),
    (rows_state(B=32, inst_set=1, n_local=2048, T=64), rows(LOCAL_APPLY, 1, T=64, B=32)),
    (rows_state(B=31, inst_set=1, n_local=1984, T=66), rows(LOCAL_APPLY, 1, T=66, B=31)),
    # the tile arrays in LDS: two floats per tile fit up to 7680 tiles; beyond, k_tile_weights in front and one float
    (rows_state(n_local=7680 * 64), rows(LOCAL_APPLY, 7680)),
    (rows_state(n_local=7681 * 64), rows(LOCAL_APPLY, 7681, from_costs=0, tile_weights_first=1)),
    # the rollout kernel's epilogue has left the tile weights
    (rows_state(tile_packets_fresh=1), rows(LOCAL_APPLY, 1024, from_costs=0)),
    # one float per tile beyond 60 KiB: the launcher refuses what the choice reports
    (rows_state(n_local=15361 * 64), dict(rows(LOCAL_APPLY, 15361, from_costs=0, tile_weights_first=1), lds=61444)),
]

# every conjunct of beside_update switched off once
BESIDE = [
    (c5(), C5_ROWS),
    (c5(want_next=0), C5_PLAIN),
    (c5(have_noise=1), C5_PLAIN),
    (c5(side_stream_pays=1), C5_PLAIN),
    (c5(flags_env_off=1), C5_PLAIN),
    (c5(graph_on=1), C5_PLAIN),
    (c5(prof=1), C5_PLAIN),
    (c5(defer_exchange=1), rows(PACKET_ONLY, 64, B=64, from_costs=0)),
    (c5(flag_words=0), C5_PLAIN),
    (c5(stream_flags_off=1), C5_PLAIN),
    (c5(rng=XOROSHIRO), C5_PLAIN),
    (c5(n_local=39936, T=100), rows(LOCAL_APPLY, 10, B=64, from_costs=0)),  # 3.99M rollout-steps
    (c5(n_local=40000, n_inst=625, inst_tiles=10, T=100), rows(LOCAL_APPLY, 10, B=64, from_costs=0, slim=1)),  # 4M
    (c5(scan_packets_fresh=1), combine(LOCAL_APPLY, 128, B=64)),
    (c5(world_size=2), rows(GATHER_APPLY, 64, B=64, from_costs=0)),
    (c5(has_comm=1), rows(GATHER_APPLY, 64, B=64, from_costs=0)),
    (c5(m_count=2), C5_PLAIN),
    (c5(B=1, inst_set=0, n_local=7681 * 64), rows(LOCAL_APPLY, 7681, from_costs=0)),
    # ... and slim from the costs: 60 KiB asked for either way
    (c5(tile_packets_fresh=0), rows(LOCAL_APPLY, 64, B=64, from_costs=1, slim=1)),
    (c5(B=1, inst_set=0, n_local=7680 * 64, tile_packets_fresh=0), rows(LOCAL_APPLY, 7680, slim=1)),
]

TABLE = ROUTES + TRAPS + FOLDS + FORMS + BESIDE


@pytest.fixture(scope="module")
def choose(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("update_plan")
    src = tmp / "choose.cpp"
    n = len(FIELDS)
    src.write_text(PROGRAM % (os.path.abspath(HEADER), n, n, n, n))
    exe = tmp / "choose"
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-o", str(exe), str(src)])

    def run(states):
        text = "".join(" ".join(str(int(s[k])) for k in FIELDS) + "\n" for s in states)
        out = subprocess.run([str(exe)], input=text.encode(), stdout=subprocess.PIPE, check=True).stdout.decode().splitlines()
        assert len(out) == len(states)
        return [{k: int(v) for k, v in (item.split("=") for item in line.split())} for line in out]
    return run


def test_update_choose_matches_the_table(choose):
    assert len(TABLE) >= 45
    for (state, want), got in zip(TABLE, choose([s for s, _ in TABLE])):
        for key, value in want.items():
            assert got[key] == value, "state %s: %s = %s, the table says %s" % (state, key, got[key], value)


def test_the_table_has_a_row_for_every_route_and_kernel():
    assert {want["route"] for _, want in TABLE} == {LEAVE_TILES, LOCAL_APPLY, PACKET_ONLY, GATHER_APPLY, GATHER_LEAVE_APPLY}
    assert {want["kernel"] for _, want in TABLE} == {NO_KERNEL, COMBINE, ROWS}
    assert {s["world_size"] for s, _ in TABLE} >= {1, 2, 16, 17}


def test_the_row_kernels_lds_follows_from_its_layout():
    """scale_sh[n_tiles] floats (update_kernels.h), beta_sh[n_tiles] more when the weights are formed from the costs;
    60 KiB are the limit, and what a slim launch asks for whatever it needs."""
    for state, want in TABLE:
        if want.get("kernel") != ROWS:
            continue
        tiles = state["inst_tiles"]
        fits = 2 * 4 * tiles <= LDS_MAX
        assert want["from_costs"] == int(fits and not state["tile_packets_fresh"]), state
        assert want["tile_weights_first"] == int(not fits and not state["tile_packets_fresh"]), state
        assert want["lds"] == 4 * tiles * (2 if want["from_costs"] else 1), state
        assert want["lds_launch"] == (LDS_MAX if want["slim"] and want["lds"] <= LDS_MAX else want["lds"]), state
    assert 2 * 4 * 7680 == LDS_MAX


def test_beside_update_implies_the_local_rows_route(choose):
    """launch_iteration starts the generator beside the update only where k_update_rows<.., 256> applies locally: over
    every combination of the switches the table uses, beside_update comes with that route, that kernel and its LDS."""
    import itertools
    keys = ["world_size", "has_comm", "m_count", "defer_exchange", "prof", "scan_packets_fresh", "tile_packets_fresh", "may_leave_apply"]
    states = [c5(**dict(zip(keys, bits))) for bits in itertools.product(*[(2, 1) if k in ("world_size", "m_count") else (0, 1) for k in keys])]
    states += [c5(B=1, inst_set=0, n_local=t * 64) for t in (7680, 7681, 15360, 15361)]
    hits = 0
    for state, got in zip(states, choose(states)):
        assert got["slim"] == got["beside_update"], state
        if got["beside_update"]:
            hits += 1
            assert (got["route"], got["kernel"], got["apply_here"], got["block"], got["lds_launch"]) == (LOCAL_APPLY, ROWS, 1, 256, LDS_MAX), state
            assert got["lds"] <= LDS_MAX, state
    assert hits >= 4
