"""Where an iteration's noise comes from, who produces the next iteration's and how the two streams are ordered around it
(csrc/noise_plan.h: noise_choose) against a table.

The header is plain C++: a small host program compiled with g++ reads states and prints choices.  The expected rows were
written by reading the code the function replaced (launch_iteration with scan_generates_noise and side_stream_pays, the
`extra` blocks of launch_scan, launch_pipe and launch_rollout_tdm, noise_flag_params, and the two generator sequences on the
second stream), not by running it; the CVaR kernel's block count is worked out a second time here.

NoiseHeld::update_can_host is update_noise_beside (csrc/update_plan.h) asked by noise_held as if no noise were there yet:
tests/test_update_plan.py (BESIDE) switches every conjunct of it off once.  Here the conjuncts that noise_choose adds are
switched off once each: want_next, noise left by the rollout launch, side_stream_pays, and update_can_host itself.

Four rows keep answers that look inconsistent on purpose (TRAPS): they are today's, and a change to any of them is a
change of behaviour.
"""
import os
import subprocess

import pytest

HEADER = os.path.join(os.path.dirname(__file__), "..", "mppi_numba_amd", "csrc", "noise_plan.h")

FIELDS = ["rng", "n_local", "T", "num_cus", "num_grid_samples",
          "debug_flags", "graph_on", "stream_flags_off", "flags_env_off", "flag_words",
          "want_next", "have_noise", "noise_on_side_stream", "prev_signalled",
          "launch", "workgroups", "scan_exact", "update_can_host"]

OUT = ["launch", "source", "discard_ahead", "consumer", "extra_blocks", "side_stream_pays", "record_front", "signals",
       "beside_rollout", "beside_update", "hold", "announce", "join", "have_after_rollout", "have_noise"]

PROGRAM = r"""
#include <cstdio>
#include <cstring>
#include "%s"
int main() {
  for (;;) {
    NoiseHeld h;
    std::memset(&h, 0, sizeof(h));
    int* f = &h.rng;  // (the struct is %d ints, in the order of FIELDS)
    static_assert(sizeof(NoiseHeld) == %d * sizeof(int), "NoiseHeld has a field the test does not know");
    static_assert(sizeof(NoiseChoice) == %d * sizeof(int), "NoiseChoice has a field the test does not print");
    int got = 0;
    while (got < %d && std::scanf("%%d", f + got) == 1) ++got;
    if (got != %d) break;
    const NoiseChoice c = noise_choose(h);
    const int* o = &c.launch;
    for (int i = 0; i < %d; ++i) std::printf("%%d ", o[i]);
    std::printf("\n");
  }
  return 0;
}
"""

PHILOX, XOROSHIRO = 0, 1
SCAN_READ_NOISE, DROP_NOISE_FLAG = 1 << 6, 1 << 11
SCAN, SCAN_EXACT, PIPE, FUSED, GENERAL, CVAR_FAST, CVAR, BAREBONE = range(1, 9)
IN_LINE, AHEAD, IN_KERNEL = range(3)
NO_ORDER, BY_FLAG, BY_EVENT = range(3)
NO_HOLD, EVENT_FRONT, GATE, EVENT_BEHIND = range(4)
SILENT, FLAG, DROPPED = range(3)


def held(**over):
    """c2, N = 8192, T = 100 in the middle of a loop on 256 CUs: k_rollout_scan_exact on 256 tiles of 32"""
    s = dict(rng=PHILOX, n_local=8192, T=100, num_cus=256, num_grid_samples=1, debug_flags=0, graph_on=0, stream_flags_off=0,
             flags_env_off=0, flag_words=1, want_next=1, have_noise=0, noise_on_side_stream=0, prev_signalled=0,
             launch=SCAN_EXACT, workgroups=None, scan_exact=None, update_can_host=0)
    assert set(over) <= set(s), over
    s.update(over)
    if s["workgroups"] is None:
        s["workgroups"] = (s["n_local"] + 31) // 32
    if s["scan_exact"] is None:
        s["scan_exact"] = int(s["launch"] == SCAN_EXACT)
    return s


def small(**over):
    """... at N = 800, T = 32: 25 tiles, 231 CUs to spare"""
    return held(**dict(dict(n_local=800, T=32), **over))


def pipe(n=800, t=32, **over):
    """k_rollout_pipe, one wave triple per workgroup"""
    return held(**dict(dict(n_local=n, T=t, launch=PIPE, workgroups=(n + 63) // 64), **over))


def cvar(n=256, t=32, m=64, **over):
    """c3: the CVaR fast kernel, a workgroup per rollout"""
    return held(**dict(dict(n_local=n, T=t, num_grid_samples=m, launch=CVAR_FAST, workgroups=n), **over))


def ns(**over):
    """bench.py's ns: N = 65536, T = 100, k_rollout_fused on 256 workgroups of four waves, in the steady state of a loop:
    this iteration's noise is in flight on the second stream and the previous launch signalled its start"""
    return held(**dict(dict(n_local=65536, launch=FUSED, workgroups=256, have_noise=1, noise_on_side_stream=1, prev_signalled=1), **over))


def c5(**over):
    """bench.py's c5: 64 problems of 4096 rollouts, k_rollout_fused, 16 rollout waves per CU; steady state"""
    return held(**dict(dict(n_local=262144, launch=FUSED, workgroups=1024, have_noise=1, noise_on_side_stream=1, prev_signalled=1,
                            update_can_host=1), **over))


# ---- expected choices ---------------------------------------------------------------------------------------------------
def cvar_blocks(n, t, m, cus=256):
    """launch_rollout_tdm: rows of 64 Philox items (two steps each), four rows per wave of the block, at most two blocks per CU"""
    rows = (n + 63) // 64 * ((t + 1) // 2)
    waves = min((m + 63) // 64 * 64, 1024) // 64
    return min(2 * cus, -(-rows // (4 * waves)))


NOTHING_AHEAD = dict(extra_blocks=0, record_front=0, beside_rollout=0, beside_update=0, hold=NO_HOLD, announce=SILENT, join=0,
                     have_after_rollout=0, have_noise=0)
IN_KERNEL_ROW = dict(NOTHING_AHEAD, source=IN_KERNEL, discard_ahead=0, consumer=NO_ORDER, signals=0)


def blocks(count, source=IN_LINE, **more):
    return dict(dict(source=source, consumer=NO_ORDER, extra_blocks=count, beside_rollout=0, beside_update=0, hold=NO_HOLD,
                     announce=SILENT, join=0, have_after_rollout=1, have_noise=1), **more)


def beside_rollout(hold, announce=FLAG, **more):
    return dict(dict(extra_blocks=0, side_stream_pays=1, record_front=int(hold == EVENT_FRONT), beside_rollout=1, beside_update=0,
                     hold=hold, announce=announce, join=0, have_after_rollout=1, have_noise=1), **more)


NS_STEADY = beside_rollout(GATE, source=AHEAD, consumer=BY_FLAG, signals=1)
BESIDE_UPDATE = dict(source=AHEAD, consumer=BY_FLAG, extra_blocks=0, side_stream_pays=0, record_front=0, signals=1, beside_rollout=0,
                     beside_update=1, hold=GATE, announce=FLAG, join=0, have_after_rollout=0, have_noise=1)
C5_IN_LINE = dict(NOTHING_AHEAD, source=AHEAD, consumer=BY_FLAG, side_stream_pays=0, signals=1)

ROUTES = [
    # c2 in a loop: in-kernel, nothing ahead -- also in the first iteration behind a different kind of launch
    (held(), dict(IN_KERNEL_ROW, launch=SCAN_EXACT)),
    (small(), IN_KERNEL_ROW),
    (small(launch=SCAN), IN_KERNEL_ROW),
    (small(have_noise=1), dict(IN_KERNEL_ROW, discard_ahead=1)),
    (small(have_noise=1, noise_on_side_stream=1), dict(IN_KERNEL_ROW, discard_ahead=1, consumer=NO_ORDER)),
    # ... reading its noise: the tolerance kernel's spare CUs generate, the exact kernel's do not (in line)
    (small(launch=SCAN, debug_flags=SCAN_READ_NOISE), blocks(256 - 25)),
    (small(launch=SCAN, debug_flags=SCAN_READ_NOISE, have_noise=1), blocks(256 - 25, source=AHEAD)),
    (held(launch=SCAN, debug_flags=SCAN_READ_NOISE), dict(NOTHING_AHEAD, source=IN_LINE)),  # 256 tiles: no CU to spare
    (small(launch=SCAN, debug_flags=SCAN_READ_NOISE, workgroups=13), blocks(256 - 13)),  # (tiles of 64)
    # xoroshiro on a scan map: the kernel reads, nothing is appended
    (small(rng=XOROSHIRO), dict(NOTHING_AHEAD, source=IN_LINE)),
    (small(rng=XOROSHIRO, launch=SCAN), dict(NOTHING_AHEAD, source=IN_LINE)),
    # the pipelined kernel: spare CUs, or none (in line below 4M rollout-steps, the second stream above)
    (pipe(), blocks(256 - 13)),
    (pipe(rng=XOROSHIRO), blocks(256 - 13)),
    (pipe(16384, 100), dict(NOTHING_AHEAD, source=IN_LINE, side_stream_pays=0)),
    (pipe(16384, 200, workgroups=255), blocks(1, side_stream_pays=0)),
    (pipe(49152, 100, workgroups=256), beside_rollout(EVENT_FRONT, source=IN_LINE, signals=0)),
    (pipe(49152, 100, workgroups=256, prev_signalled=1), beside_rollout(EVENT_BEHIND, source=IN_LINE, signals=0)),
    # the CVaR kernels
    (cvar(), blocks(cvar_blocks(256, 32, 64))),
    (cvar(4096, 100, 128), blocks(cvar_blocks(4096, 100, 128))),
    (cvar(4096, 100, 1024), blocks(cvar_blocks(4096, 100, 1024))),
    (cvar(65536, 100, 128), blocks(512)),
    (cvar(rng=XOROSHIRO), dict(NOTHING_AHEAD, source=IN_LINE)),
    (cvar(launch=CVAR), dict(NOTHING_AHEAD, source=IN_LINE)),
    (cvar(launch=CVAR, have_noise=1), dict(NOTHING_AHEAD, source=AHEAD, consumer=NO_ORDER)),
    # barebone, and the general map kernel: nothing appended; the second stream where it pays
    (held(launch=BAREBONE, workgroups=128), dict(NOTHING_AHEAD, source=IN_LINE, signals=0)),
    (held(launch=BAREBONE, n_local=65536, workgroups=1024), beside_rollout(EVENT_FRONT, source=IN_LINE, signals=0)),
    (held(launch=GENERAL, n_local=65536, workgroups=1024, have_noise=1, noise_on_side_stream=1),
     beside_rollout(EVENT_FRONT, source=AHEAD, consumer=BY_EVENT, signals=0)),
    # the last iteration of a caller that wants nothing ahead
    (pipe(want_next=0), dict(NOTHING_AHEAD, source=IN_LINE)),
    (cvar(want_next=0), dict(NOTHING_AHEAD, source=IN_LINE)),
    (small(launch=SCAN, debug_flags=SCAN_READ_NOISE, want_next=0), dict(NOTHING_AHEAD, source=IN_LINE)),
    (ns(want_next=0), dict(NOTHING_AHEAD, source=AHEAD, consumer=BY_FLAG, signals=1, side_stream_pays=1)),
    (c5(want_next=0), C5_IN_LINE),
]

THROUGHPUT = [
    # the first iteration of a loop: in line, the event in front; the second: the generator's flag, still the event (the
    # first launch could not be known to signal); from the third on the gate
    (ns(have_noise=0, noise_on_side_stream=0, prev_signalled=0), beside_rollout(EVENT_FRONT, source=IN_LINE, consumer=NO_ORDER, signals=1)),
    (ns(prev_signalled=0), beside_rollout(EVENT_FRONT, source=AHEAD, consumer=BY_FLAG, signals=1)),
    (ns(), NS_STEADY),
    # noise ahead that is not in flight (handed over behind a join): no order needed
    (ns(noise_on_side_stream=0), dict(NS_STEADY, consumer=NO_ORDER)),
    # graph replay: the event in front, the join before the update, no flag, no progress word
    (ns(graph_on=1, noise_on_side_stream=0), beside_rollout(EVENT_FRONT, SILENT, source=AHEAD, consumer=NO_ORDER, signals=0, join=1)),
    (ns(graph_on=1, noise_on_side_stream=0, prev_signalled=0), beside_rollout(EVENT_FRONT, SILENT, source=AHEAD, consumer=NO_ORDER, signals=0, join=1)),
    # the handle has fallen back to events; the developer's switch; a handle without the words
    (ns(stream_flags_off=1, prev_signalled=0), beside_rollout(EVENT_FRONT, source=AHEAD, consumer=BY_EVENT, signals=0)),
    (ns(flags_env_off=1, prev_signalled=0), beside_rollout(EVENT_FRONT, source=AHEAD, consumer=BY_EVENT, signals=0)),
    (ns(flag_words=0, prev_signalled=0), beside_rollout(EVENT_FRONT, SILENT, source=AHEAD, consumer=BY_EVENT, signals=0)),
    # the test hook: the sequence number moves, nothing is stored; the consumer looks all the same
    (ns(debug_flags=DROP_NOISE_FLAG), dict(NS_STEADY, announce=DROPPED)),
    (ns(debug_flags=DROP_NOISE_FLAG, graph_on=1, noise_on_side_stream=0),
     beside_rollout(EVENT_FRONT, SILENT, source=AHEAD, consumer=NO_ORDER, signals=0, join=1)),
    # 8 rollout waves per CU pay, 9 do not; 4M rollout-steps pay, fewer do not
    (ns(n_local=131072, workgroups=512), NS_STEADY),
    (ns(n_local=131072 + 64, workgroups=513), dict(NOTHING_AHEAD, source=AHEAD, consumer=BY_FLAG, signals=1, side_stream_pays=0)),
    (ns(n_local=40000, workgroups=157), NS_STEADY),
    (ns(n_local=39999, workgroups=157), dict(NOTHING_AHEAD, source=AHEAD, consumer=BY_FLAG, signals=1, side_stream_pays=0)),
    # a kernel that does not look at the flag itself is ordered by the event, with and without the words
    (ns(launch=GENERAL, prev_signalled=0), beside_rollout(EVENT_FRONT, source=AHEAD, consumer=BY_EVENT, signals=0)),
    (ns(launch=PIPE, n_local=49152, prev_signalled=0), beside_rollout(EVENT_FRONT, source=AHEAD, consumer=BY_EVENT, signals=0)),
    (ns(launch=PIPE, n_local=49152, noise_on_side_stream=0, prev_signalled=0), beside_rollout(EVENT_FRONT, source=AHEAD, consumer=NO_ORDER, signals=0)),
    (ns(launch=GENERAL, flag_words=0, prev_signalled=0), beside_rollout(EVENT_FRONT, SILENT, source=AHEAD, consumer=BY_EVENT, signals=0)),
]

# c5: more than 8 rollout waves per CU, the generator beside the update; each conjunct that noise_choose adds off once
BESIDE_THE_UPDATE = [
    (c5(), BESIDE_UPDATE),
    (c5(have_noise=0, noise_on_side_stream=0, prev_signalled=0), dict(BESIDE_UPDATE, source=IN_LINE, consumer=NO_ORDER)),
    (c5(want_next=0), C5_IN_LINE),
    (c5(update_can_host=0), C5_IN_LINE),
    (c5(n_local=131072, workgroups=512), NS_STEADY),  # side_stream_pays: beside the rollout instead
    (pipe(n=135168, workgroups=200, update_can_host=1), blocks(56, side_stream_pays=0, beside_update=0)),  # noise left by the launch
    (c5(debug_flags=DROP_NOISE_FLAG), BESIDE_UPDATE),  # (trap 4)
    (c5(launch=GENERAL), dict(BESIDE_UPDATE, consumer=BY_EVENT, signals=0)),
    # a time-parallel kernel in the kernel: it wants nothing ahead, whatever the update could host
    (small(update_can_host=1), IN_KERNEL_ROW),
]

TRAPS = [
    # 1. the event in front of the rollout is decided from whether the PREVIOUS launch signalled, not the coming one:
    #    behind a launch that did not, a launch that will still gets the event; behind one that did, a launch that will not
    #    gets no event in front and the generator is ordered behind it (one iteration without overlap)
    (ns(prev_signalled=0), beside_rollout(EVENT_FRONT, source=AHEAD, consumer=BY_FLAG, signals=1)),
    (ns(launch=GENERAL, prev_signalled=1), beside_rollout(EVENT_BEHIND, source=AHEAD, consumer=BY_EVENT, signals=0)),
    (ns(stream_flags_off=1, prev_signalled=1), beside_rollout(EVENT_BEHIND, source=AHEAD, consumer=BY_EVENT, signals=0)),
    # 2. ... and it is recorded wherever the second stream would pay, also in front of a launch whose own blocks generate
    (pipe(44000, 100, workgroups=230), blocks(26, side_stream_pays=1, record_front=1)),
    (cvar(65536, 100, 128), blocks(512, side_stream_pays=1, record_front=1)),
    # 3. the time-parallel kernel appends noise blocks for the tolerance kernel only
    (small(debug_flags=SCAN_READ_NOISE), dict(NOTHING_AHEAD, source=IN_LINE)),
    (small(debug_flags=SCAN_READ_NOISE, have_noise=1), dict(NOTHING_AHEAD, source=AHEAD)),
    # 4. the generator announces itself whatever the switches say of the consumer, and the test hook that drops the flag
    #    does not reach the generator beside the update
    (ns(flags_env_off=1, prev_signalled=0), dict(announce=FLAG, consumer=BY_EVENT)),
    (ns(stream_flags_off=1, prev_signalled=0), dict(announce=FLAG, consumer=BY_EVENT)),
    (c5(debug_flags=DROP_NOISE_FLAG), dict(announce=FLAG, beside_update=1)),
]

TABLE = ROUTES + THROUGHPUT + BESIDE_THE_UPDATE + TRAPS


@pytest.fixture(scope="module")
def choose(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("noise_plan")
    src = tmp / "choose.cpp"
    n = len(FIELDS)
    src.write_text(PROGRAM % (os.path.abspath(HEADER), n, n, len(OUT), n, n, len(OUT)))
    exe = tmp / "choose"
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-o", str(exe), str(src)])

    def run(states):
        text = "".join(" ".join(str(int(s[k])) for k in FIELDS) + "\n" for s in states)
        out = subprocess.run([str(exe)], input=text.encode(), stdout=subprocess.PIPE, check=True).stdout.decode().splitlines()
        assert len(out) == len(states)
        return [dict(zip(OUT, map(int, line.split()))) for line in out]
    return run


def test_noise_choose_matches_the_table(choose):
    assert len(TABLE) >= 60
    for (state, want), got in zip(TABLE, choose([s for s, _ in TABLE])):
        assert got["launch"] == state["launch"]
        for key, value in want.items():
            assert got[key] == value, "state %s: %s = %s, the table says %s" % (state, key, got[key], value)


def test_the_table_has_a_row_for_every_route_and_ordering():
    assert {s["launch"] for s, _ in TABLE} == set(range(1, 9))
    assert {want["source"] for _, want in TABLE if "source" in want} == {IN_LINE, AHEAD, IN_KERNEL}
    assert {want["consumer"] for _, want in TABLE if "consumer" in want} == {NO_ORDER, BY_FLAG, BY_EVENT}
    assert {want["hold"] for _, want in TABLE if "hold" in want} == {NO_HOLD, EVENT_FRONT, GATE, EVENT_BEHIND}
    assert {want["announce"] for _, want in TABLE if "announce" in want} == {SILENT, FLAG, DROPPED}
    assert any(want.get("beside_update") for _, want in TABLE) and any(want.get("join") for _, want in TABLE)


def test_the_cvar_blocks_follow_from_the_generator_layout():
    """noise_items (rng_kernels.h): ceil(N / 64) * 64 * ceil(T / 2) Philox items in rows of 64; a block of W waves takes
    four rows per wave; never more than two blocks per CU."""
    assert cvar_blocks(256, 32, 64) == 16       # tests/test_gpu_update_plan.py: "k_rollout_tdm_fast pow2res=1 noise_blocks=16"
    assert cvar_blocks(4096, 100, 128) == 400   # 3200 rows, 8 per block
    assert cvar_blocks(4096, 100, 1024) == 50   # 64 per block
    assert cvar_blocks(65536, 100, 128) == 512  # 6400 blocks asked for, two per CU given


def test_every_choice_has_one_source_and_every_generator_one_hold(choose):
    """Over the table and over every combination of the switches: one source per row; a generator on the second stream is
    held back in exactly one way, is never beside both launches, and never comes with blocks of the rollout launch; the
    noise is there on return exactly when somebody produced it."""
    import itertools
    keys = ["debug_flags", "graph_on", "stream_flags_off", "flags_env_off", "flag_words", "want_next", "have_noise",
            "noise_on_side_stream", "prev_signalled", "update_can_host", "rng"]
    values = {"debug_flags": (0, SCAN_READ_NOISE, DROP_NOISE_FLAG)}
    states = [s for s, _ in TABLE]
    for base in (small(), small(launch=SCAN), pipe(), pipe(49152, 100, workgroups=256), cvar(), cvar(launch=CVAR), ns(), c5(),
                 held(launch=BAREBONE, n_local=65536, workgroups=1024), ns(launch=GENERAL)):
        for bits in itertools.product(*[values.get(k, (0, 1)) for k in keys]):
            s = dict(base, **dict(zip(keys, bits)))
            if s["noise_on_side_stream"] <= s["have_noise"]:
                states.append(s)
    generators = 0
    for s, c in zip(states, choose(states)):
        assert c["source"] in (IN_LINE, AHEAD, IN_KERNEL), s
        assert (c["source"] == AHEAD) == bool(s["have_noise"] and c["source"] != IN_KERNEL), s
        assert c["discard_ahead"] == int(c["source"] == IN_KERNEL and s["have_noise"]), s
        assert (c["consumer"] != NO_ORDER) == (c["source"] == AHEAD and bool(s["noise_on_side_stream"])), s
        on_side = c["beside_rollout"] + c["beside_update"]
        assert on_side <= 1 and not (on_side and c["extra_blocks"]), s
        assert (c["hold"] != NO_HOLD) == bool(on_side), s
        assert c["record_front"] or c["hold"] != EVENT_FRONT, s
        assert c["hold"] != GATE or c["signals"] or c["beside_update"], s  # (somebody writes the word the gate waits for)
        assert c["announce"] == SILENT or on_side, s
        assert not c["join"] or (c["beside_rollout"] and s["graph_on"]), s
        assert c["have_noise"] == int(bool(on_side or c["extra_blocks"])), s
        assert c["have_after_rollout"] == int(bool(c["beside_rollout"] or c["extra_blocks"])), s
        assert s["want_next"] or not c["have_noise"], s
        if c["consumer"] == BY_FLAG:
            assert s["launch"] == FUSED and s["flag_words"] and not s["flags_env_off"] and not s["stream_flags_off"], s
        generators += on_side
    assert generators >= 100
