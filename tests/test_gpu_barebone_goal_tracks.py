"""A goal that moves in the barebone planner: params['goal_track'] (L, 2), MPPI_Batch.set_goal_tracks,
mppi_planner_set_goal_tracks.  Row j is the goal's position at time j*dt from "now" = row `track_offset`; the state after
step t of a rollout is measured against row min(track_offset + t + 1, L - 1).  Both kernel families take it -- the default
forms stage the rows in LDS, the crowd kernel's count waves load the step's row -- and every comparison of costs here is bit
for bit with tests/goal_track_model.py (whose row selection and equal-rows case tests/test_goal_track_model.py pins on the
CPU) unless it says otherwise."""
import ctypes as C
import functools
import gc

import numpy as np
import pytest

from test_gpu_barebone_batch import ERR_INVALID, make_params, oracle_params, problem_params, problems, random_discs
from test_gpu_barebone_crowd import cfg_of, inputs, shape_of
from test_gpu_barebone_tracks import form_of, rollout_with
from test_gpu_barebone_wall_tracks import disc_case, moving_building
from test_gpu_barebone_walls import DIAG, N, SIDE, assert_bits, building, task, without_walls
from crowd_model import hit_counts
from goal_track_model import NO_DISCS, freeze_step, goal_rows, goal_track_costs

pytestmark = pytest.mark.gpu

DT = 0.1


@pytest.fixture(autouse=True)
def release_the_handles():
    """A planner and its device-array views refer to each other, so a handle lives until the cycle collector runs.  Collect
    when a test ends: the streams of this module's planners do not outlive it."""
    yield
    gc.collect()


@functools.lru_cache(maxsize=None)
def crossing_goal(t, rows):
    """A goal that comes in from the left of the fan of rollouts of task(t, .) -- start (0, 0), heading along DIAG, about
    0.12 m per step -- at constant velocity and, in its last row, stands on the diagonal 0.12 * t + 0.45 m from the start:
    about the goal tolerance (0.5 m) ahead of where a rollout of average speed ends, so that the faster rollouts get within
    the tolerance of the goal's late rows and the slower ones do not -- whichever offset the rows are read from, past the
    end included.  Row 0 is 1.2 m to the side of that and 0.3 m nearer, where hardly a rollout turns to."""
    end = (0.12 * t + 0.45) * DIAG
    first = end + 1.2 * SIDE - 0.3 * DIAG
    s = (np.arange(rows, dtype=np.float64) / max(rows - 1, 1))[:, None]
    track = (first[None] * (1.0 - s) + end[None] * s).astype(np.float32) if rows > 1 else first[None].astype(np.float32)
    track.setflags(write=False)
    return track


def goal_params(params, track):
    p = {k: v for k, v in params.items() if k != "xgoal"}
    p["goal_track"] = track
    return p


def the_goal_input_means_something(p, track, st, t, offset):
    """Asserted with the model, on the CPU, before anything is compared, for every track of more than one row at every
    offset: some rollouts freeze at the moving goal mid-horizon and some never reach it, and at least one reaches the moving
    goal that would not reach the goal of row 0 -- existence, not shares."""
    if len(track) == 1:
        return
    froze = freeze_step(p, goal_rows(track, t, offset), st)
    froze_at_row0 = freeze_step(p, goal_rows(track[:1], t), st)
    assert ((froze > 0) & (froze < t - 1)).any(), "bad input: no rollout freezes at the moving goal mid-horizon"
    assert (froze == t).any(), "bad input: every rollout reaches the moving goal"
    assert ((froze < t) & (froze_at_row0 == t)).any(), "bad input: no rollout reaches the moving goal but not the goal of row 0"


def model_costs(params, track, t, offset, noise, u_in, disc_tracks, rad, wall_tracks=None, hw=None):
    """The model's costs, after the checks that the input means something; the costs of the row-0 static goal differ."""
    p = oracle_params(dict(without_walls(params), xgoal=track[0]))
    st = hit_counts(p, *NO_DISCS, noise, u_in)[1]
    the_goal_input_means_something(p, track, st, t, offset)
    model = goal_track_costs(p, track, noise, u_in, offset, disc_tracks, rad, wall_tracks, hw)
    if len(track) > 1:
        at_row0 = goal_track_costs(p, track[:1], noise, u_in, 0, disc_tracks, rad, wall_tracks, hw)
        assert (model != at_row0).any(), "bad input: the costs are those of the row-0 static goal"
    return model


@pytest.mark.parametrize("K,kind,wscale", [(K, kind, wscale) for K in (0, 2, 4, 7) for kind in ("static", "tracks")
                                           for wscale in (1.0, 1.5)])
def test_default_family_costs_equal_the_model(K, kind, wscale):
    """T = 13: one batch of eight steps plus a tail.  Rotation on (wscale 1.0: the KD forms up to four discs) and off;
    goal tracks of 1, 12 and T + 6 rows -- the disc tracks have T + 1 --; offsets 0, 5 and past the end."""
    from mppi_numba_amd.barebone import MPPI_Numba
    t = 13
    params, u_in, noise = task(t, wscale)
    tracks, rad, full = disc_case(K, kind, t, params)
    planner = MPPI_Numba(cfg_of(N, t, False))
    for L in (1, 12, t + 6):
        track = crossing_goal(t, L)
        assert kind != "tracks" or tracks.shape[1] != L
        planner.set_params(goal_params(full, track))
        for offset in (0, 5, L + 3):
            model = model_costs(params, track, t, offset, noise, u_in, tracks, rad)
            planner.move_mppi_task_vars_to_device()  # (hands the tracks over the first time: offset 0)
            planner.set_track_offset(offset)
            got, _, _, kernel = rollout_with(planner, u_in, noise)
            assert kernel.startswith("k_rollout_barebone exact=1 rotation=%d " % (wscale == 1.0)) and form_of(K, wscale == 1.0) in kernel, kernel
            assert kernel.endswith(" goal_rows=%d" % L) and ("tracks=%d" % (t + 1) in kernel) == (kind == "tracks"), kernel
            assert_bits(got, model, "%d discs (%s), %d goal rows, offset %d vs the model" % (K, kind, L, offset))


@pytest.mark.parametrize("walls,kind,t,wscale", [(walls, kind, t, wscale) for walls in ("none", "static", "tracks")
                                                 for kind in ("static", "tracks") for t, wscale in ((30, 1.0), (37, 1.5))])
def test_crowd_family_costs_equal_the_model(walls, kind, t, wscale):
    """70 discs; no walls, 65 static walls, 65 walls x 12 rows.  T = 30 and 37: more than one chunk, no multiple of the
    counters.  Goal tracks of 1, 12 and T + 6 rows (9 in place of 12 beside the 12-row wall tracks: never the walls' count;
    the disc tracks have T + 1)."""
    from mppi_numba_amd.barebone import MPPI_Numba
    params, u_in, noise = task(t, wscale)
    tracks, rad, full = disc_case(70, kind, t, params)
    wtracks = hw = None
    if walls == "static":
        seg, hw = building(65)
        wtracks = seg[:, None]
        full["wall_segments"], full["wall_halfwidth"] = seg, hw
    elif walls == "tracks":
        wtracks, hw = moving_building(65, 12)
        full["wall_tracks"], full["wall_halfwidth"] = wtracks, hw
    planner = MPPI_Numba(cfg_of(N, t, True))
    for L in (1, 9 if walls == "tracks" else 12, t + 6):
        track = crossing_goal(t, L)
        assert L not in ([tracks.shape[1]] if kind == "tracks" else []) + ([12] if walls == "tracks" else [])
        planner.set_params(goal_params(full, track))
        for offset in (0, 5, L + 3):
            model = model_costs(params, track, t, offset, noise, u_in, tracks, rad, wtracks, hw)
            planner.move_mppi_task_vars_to_device()
            planner.set_track_offset(offset)
            got, _, _, kernel = rollout_with(planner, u_in, noise)
            assert t > shape_of(kernel)[1], kernel
            assert kernel.endswith(" goal_rows=%d" % L) and ("rotation=1" in kernel) == (wscale == 1.0) and "exact=1" in kernel, kernel
            assert (" walls=65" in kernel) == (walls != "none") and (" wall_rows=12" in kernel) == (walls == "tracks"), kernel
            assert ("tracks=%d" % (t + 1) in kernel) == (kind == "tracks"), kernel
            assert_bits(got, model, "%s walls, %s discs, %d goal rows, offset %d vs the model" % (walls, kind, L, offset))


@pytest.mark.parametrize("math", ["exact", "fast"])
@pytest.mark.parametrize("crowd,K,kind,t", [(False, 2, "static", 13), (False, 4, "tracks", 13), (False, 7, "static", 13),
                                            (True, 70, "static", 30), (True, 70, "tracks", 37)])
def test_equal_rows_equal_the_static_goal(crowd, K, kind, t, math):
    """Costs and u after update(), both families.  The only statement made about fast math: the goal forms are the same
    code on the same operands.  The crowd cases carry 65 static walls."""
    from mppi_numba_amd.barebone import MPPI_Numba
    params, u_in, noise = task(t, 1.0)
    _, _, full = disc_case(K, kind, t, params)
    if crowd:
        full["wall_segments"], full["wall_halfwidth"] = building(65)
    static = MPPI_Numba(cfg_of(N, t, crowd, math=math))
    static.set_params(full)
    moving = MPPI_Numba(cfg_of(N, t, crowd, math=math))
    for L in (1, 7):
        moving.set_params(goal_params(full, np.repeat(np.float32(params["xgoal"])[None], L, axis=0)))
        for offset in (0, 3, L + 2):
            for planner in (static, moving):
                planner.move_mppi_task_vars_to_device()
                planner.set_track_offset(offset)
            want, want_u, _, static_kernel = rollout_with(static, u_in, noise)
            got, got_u, _, kernel = rollout_with(moving, u_in, noise)
            assert "goal_rows" not in static_kernel and kernel.endswith(" goal_rows=%d" % L), (static_kernel, kernel)
            assert kernel.startswith("k_rollout_barebone_crowd" if crowd else "k_rollout_barebone exact"), kernel
            assert ("exact=1" in kernel) == (math == "exact"), kernel
            assert_bits(got, want, "%d equal rows, offset %d vs the static goal" % (L, offset))
            assert_bits(got_u, want_u, "... u")


def problem_goal(rng, x0, goal, rows):
    """A goal that starts 0.6 m to the left of `goal` and crosses the line start -> goal at up to 1 m/s."""
    from mppi_numba_amd.barebone import constant_velocity_tracks
    along = (np.asarray(goal, np.float64) - np.asarray(x0, np.float64)[:2])
    left = np.array([-along[1], along[0]]) / np.linalg.norm(along)
    return constant_velocity_tracks([goal + 0.6 * left], [-rng.uniform(0.5, 1.0) * left], DT, rows)[0]


@pytest.mark.parametrize("crowd,K", [(False, 2), (True, 70)])
def test_batch_with_goal_tracks(crowd, K):
    """n = 64 per problem.  Per-problem goal tracks with per-problem offsets, every problem against a single-problem planner
    given its track and offset and against the model; unchanged tracks leave the offsets alone; a shared track; None gives
    the bits of `goals` again."""
    from mppi_numba_amd.barebone import MPPI_Batch, MPPI_Numba
    B, n, t, L = 3, 64, 13 if not crowd else 30, 9
    offsets = np.array([0, 3, 12], dtype=np.int32)
    rng = np.random.default_rng(17 + K)
    x0s, goals = problems(rng, B)
    pos, rad = random_discs(rng, K, x0s[0], goals[0])
    params = make_params(DT, 1.0, (pos, rad))
    gtracks = [problem_goal(rng, x0s[b], goals[b], L) for b in range(B)]
    u_in = np.stack([inputs(rng, n, t)[0] for _ in range(B)])
    noise = rng.normal(0, 0.5, (B, n, t, 2)).astype(np.float32)
    flat = noise.reshape(B * n, t, 2)
    batch = MPPI_Batch(cfg_of(n, t, crowd), B)
    batch.setup(params, x0s, goals)
    plain, plain_u, _, kernel = rollout_with(batch, u_in, flat)
    assert "goal_rows" not in kernel, kernel
    batch.set_track_offset(offsets)
    batch.set_goal_tracks(gtracks)
    np.testing.assert_array_equal(batch.track_offset, np.zeros(B))  # (new tracks: row 0 is "now")
    batch.set_track_offset(offsets)
    costs, u_out, _, kernel = rollout_with(batch, u_in, flat)
    assert "problems=%d" % B in kernel and kernel.endswith(" goal_rows=%d" % L), kernel
    assert kernel.startswith("k_rollout_barebone_crowd" if crowd else "k_rollout_barebone exact"), kernel
    np.testing.assert_array_equal(batch.goal_now, np.stack([gtracks[b][min(offsets[b], L - 1)] for b in range(B)]))
    single = MPPI_Numba(cfg_of(n, t, crowd))
    for b in range(B):
        pb = problem_params(params, x0s[b], goals[b])
        single.set_params(goal_params(pb, gtracks[b]))
        single.move_mppi_task_vars_to_device()
        single.set_track_offset(int(offsets[b]))
        want, want_u, _, single_kernel = rollout_with(single, u_in[b], noise[b])
        assert "problems" not in single_kernel and single_kernel.endswith(" goal_rows=%d" % L), single_kernel
        assert_bits(costs[b], want, "problem %d (offset %d) vs a single handle" % (b, offsets[b]))
        assert_bits(u_out[b], want_u, "problem %d u vs a single handle" % b)
        model = goal_track_costs(oracle_params(pb), gtracks[b], noise[b], u_in[b], int(offsets[b]), pos[:, None], rad)
        assert_bits(costs[b], model, "problem %d vs the model" % b)
        assert (costs[b] != plain[b]).any(), "bad input: problem %d's goal track changes nothing" % b
    # the same tracks again, as (B, L, 2): no change, the offsets stay
    batch.set_goal_tracks(np.stack(gtracks))
    np.testing.assert_array_equal(batch.track_offset, offsets)
    again, _, _, _ = rollout_with(batch, u_in, flat)
    assert_bits(again, costs, "same tracks again")
    # a refused call leaves the handle with what it had
    with pytest.raises(ValueError):
        batch.set_goal_tracks([gtracks[0], gtracks[1][:4], gtracks[2]])
    with pytest.raises(ValueError):
        batch.set_goal_tracks(gtracks[:2])
    again, _, _, _ = rollout_with(batch, u_in, flat)
    assert_bits(again, costs, "after refused calls")
    # None: the goals of set_instances again
    batch.set_goal_tracks(None)
    back, back_u, _, kernel = rollout_with(batch, u_in, flat)
    assert "goal_rows" not in kernel, kernel
    assert_bits(back, plain, "set_goal_tracks(None) vs the static goals")
    assert_bits(back_u, plain_u, "... u")
    np.testing.assert_array_equal(batch.goal_now, goals)
    # one shared track of the params, per-problem offsets
    shared = MPPI_Batch(cfg_of(n, t, crowd), B)
    shared.setup(goal_params(params, gtracks[1]), x0s)
    shared.move_mppi_task_vars_to_device()
    shared.set_track_offset(offsets)
    got, _, _, kernel = rollout_with(shared, u_in, flat)
    assert "problems=%d" % B in kernel and kernel.endswith(" goal_rows=%d" % L), kernel
    for b in range(B):
        model = goal_track_costs(oracle_params(problem_params(params, x0s[b], goals[b])), gtracks[1], noise[b], u_in[b],
                                 int(offsets[b]), pos[:, None], rad)
        assert_bits(got[b], model, "problem %d, shared track vs the model" % b)
    # per-problem tracks win over the shared one, and None hands the shared one back
    shared.set_goal_tracks(gtracks)
    shared.set_track_offset(offsets)
    own, _, _, _ = rollout_with(shared, u_in, flat)
    assert_bits(own, costs, "per-problem tracks over a shared one")
    shared.set_goal_tracks(None)
    shared.move_mppi_task_vars_to_device()
    shared.set_track_offset(offsets)
    back, _, _, _ = rollout_with(shared, u_in, flat)
    assert_bits(back, got, "the shared track again")


def _euler(x, u0, dt):
    """barebone_mppi_numba.ipynb cell 7 in float64 (see test_gpu_barebone_batch._notebook_loop)."""
    u = u0.astype(np.float64)
    return np.array([x[0] + dt * np.cos(x[2]) * u[0], x[1] + dt * np.sin(x[2]) * u[0], x[2] + dt * u[1]])


def intercept_track(rows):
    """A goal that comes down the line x = 3 at 0.8 m/s and crosses the x axis, which a robot at the origin drives along."""
    from mppi_numba_amd.barebone import constant_velocity_tracks
    return constant_velocity_tracks([[3.0, 2.4]], [[0.0, -0.8]], DT, rows)[0]


def test_closed_loop_equals_the_host_loop():
    """Two planners with the same seed: the loop on the device, and solve, Euler step, shift_and_update and the goal_now
    test from the host.  xhist, uhist and the steps taken, bit for bit; the goal is reached on the way."""
    from mppi_numba_amd.barebone import MPPI_Numba
    n, t, max_steps = 256, 30, 60
    params = goal_params(make_params(DT, 1.0, (np.array([[1.5, 0.9], [2.0, -1.0]]), np.array([0.4, 0.5]))), intercept_track(50))
    params["x0"] = np.array([0.0, 0.0, 0.0])
    tol = params["goal_tolerance"]
    host, dev = (MPPI_Numba(cfg_of(n, t, False, seed=5)) for _ in range(2))
    for planner in (host, dev):
        planner.setup(params)
    x = np.asarray(params["x0"], np.float64)
    want_x, want_u = np.full((max_steps + 1, 3), np.nan), np.full((max_steps, 2), np.nan, np.float32)
    want_x[0], want_steps = x, max_steps
    for step in range(max_steps):
        useq = host.solve()
        want_u[step] = useq[0]
        x = _euler(x, useq[0], DT)
        want_x[step + 1] = x
        host.shift_and_update(x, useq, num_shifts=1)
        assert host.track_offset == step + 1
        if np.linalg.norm(x[:2] - host.goal_now.astype(np.float64)) <= tol:
            want_steps = step + 1
            break
    assert host.last_rollout_kernel().endswith(" goal_rows=50")
    assert 5 < want_steps < max_steps, "bad input: the goal is not intercepted on the way (%d steps)" % want_steps
    assert np.linalg.norm(x[:2] - np.float64(params["goal_track"][0])) > tol  # (... and not where it started)
    got_x, got_u, got_steps = dev.closed_loop(max_steps)
    print("closed loop with a goal track: %d steps, end %s, goal there %s" % (got_steps, got_x[got_steps, :2], dev.goal_now))
    assert got_steps == want_steps
    assert dev.track_offset == want_steps  # (it stopped, and keeps the offset it had when it reached the goal)
    np.testing.assert_array_equal(dev.goal_now, params["goal_track"][want_steps])
    np.testing.assert_array_equal(got_u.view(np.int32), want_u.view(np.int32))
    np.testing.assert_array_equal(got_x.view(np.int64), want_x.view(np.int64))


def test_closed_loop_of_a_batch_equals_the_host_loop():
    """Three problems, each with its own goal track; the last one's goal comes within reach early.  The host loop holds a
    problem that has reached its goal where it is -- state and offset -- as the device does."""
    from mppi_numba_amd.barebone import MPPI_Batch
    B, n, t, L, max_steps = 3, 64, 30, 45, 40
    rng = np.random.default_rng(21)
    x0s, goals = problems(rng, B)
    gtracks = [problem_goal(rng, x0s[b], goals[b], L) for b in range(B)]
    params = make_params(DT, 1.0, random_discs(rng, 2, x0s[0], goals[0]))
    tol = params["goal_tolerance"]
    before = np.array([2, 0, 5], dtype=np.int32)
    host, dev = (MPPI_Batch(cfg_of(n, t, False, seed=7), B) for _ in range(2))
    for planner in (host, dev):
        planner.setup(params, x0s, goals, goal_tracks=gtracks)
        planner.set_track_offset(before)
    x = x0s.astype(np.float64)
    want_x, want_u = np.full((B, max_steps + 1, 3), np.nan), np.full((B, max_steps, 2), np.nan, np.float32)
    want_x[:, 0], want_steps, done = x, np.full(B, max_steps, np.int32), np.zeros(B, bool)
    for step in range(max_steps):
        useqs = host.solve()
        offsets = host.track_offset
        for b in np.nonzero(~done)[0]:
            want_u[b, step] = useqs[b, 0]
            x[b] = _euler(x[b], useqs[b, 0], DT)
            want_x[b, step + 1] = x[b]
        host.shift_and_update(x, useqs, num_shifts=1)
        host.set_track_offset(np.where(done, offsets, offsets + 1))  # (a problem at its goal keeps its offset)
        now = host.goal_now.astype(np.float64)
        for b in np.nonzero(~done)[0]:
            if np.linalg.norm(x[b, :2] - now[b]) <= tol:
                done[b], want_steps[b] = True, step + 1
        if done.all():
            break
    assert host.last_rollout_kernel().endswith(" problems=%d goal_rows=%d" % (B, L))
    assert done.any() and want_steps.max() > want_steps.min(), "bad input: no problem stops before another (%s)" % want_steps
    got_x, got_u, got_steps = dev.closed_loop(max_steps)
    print("closed loop of a batch with goal tracks: steps", got_steps)
    np.testing.assert_array_equal(got_steps, want_steps)
    np.testing.assert_array_equal(dev.track_offset, before + want_steps)  # stopped ones keep theirs, the others advanced
    np.testing.assert_array_equal(got_u.view(np.int32), want_u.view(np.int32))
    np.testing.assert_array_equal(got_x.view(np.int64), want_x.view(np.int64))


def test_solve_under_graph_replay_with_a_goal_track():
    """A direct loop and a replayed one in step, equal at every solve -- through a change of one row of the track, which
    forces a new capture, and through offsets that advance, which do not."""
    from mppi_numba_amd.barebone import MPPI_Batch
    B, n, t, L = 4, 128, 13, 20
    rng = np.random.default_rng(9)
    x0s, goals = problems(rng, B)
    gtracks = np.stack([problem_goal(rng, x0s[b], goals[b], L) for b in range(B)])
    params = make_params(DT, 1.0, random_discs(rng, 2, x0s[0], goals[0]), num_opt=5)
    direct, graphed, kept = (MPPI_Batch(cfg_of(n, t, False), B) for _ in range(3))
    for planner in (direct, graphed, kept):
        planner.setup(params, x0s, goals, goal_tracks=gtracks)
    graphed.set_graph_replay(True, 2)
    x = x0s.copy()

    def step_all():
        nonlocal x
        out = [planner.solve() for planner in (direct, graphed, kept)]
        x = x + np.float32([0.05, 0.04, 0.01])
        for planner in (direct, graphed, kept):
            planner.shift_and_update_on_device(x, num_shifts=1)
        return out

    for _ in range(8):  # (a graph per parity of the noise and control buffers: eight solves have captured every one in use)
        a_, b_, c_ = step_all()
        np.testing.assert_array_equal(a_, b_)
        np.testing.assert_array_equal(a_, c_)
    kernel = graphed.last_rollout_kernel()
    assert kernel.startswith("k_rollout_barebone exact") and kernel.endswith(" problems=%d goal_rows=%d" % (B, L)), kernel
    np.testing.assert_array_equal(graphed.track_offset, np.full(B, 8))
    assert graphed.graph_stats()["replays"] >= 2, graphed.graph_stats()
    captures = graphed.graph_stats()["captures"]
    for _ in range(3):  # the offsets advance: nothing a captured graph holds
        a_, b_, _ = step_all()
        np.testing.assert_array_equal(a_, b_)
    np.testing.assert_array_equal(graphed.track_offset, np.full(B, 11))
    assert graphed.graph_stats()["captures"] == captures, "an advanced offset forced a new capture"
    # one row of the tracks changes: new tracks (row 0 is "now"), another result, the same under replay and directly
    changed = gtracks.copy()
    changed[:, 2] += np.float32([0.3, -0.2])
    for planner in (direct, graphed):
        planner.set_goal_tracks(changed)
    kept.set_track_offset(0)  # (what new tracks do to the other two)
    a_, b_, c_ = step_all()
    np.testing.assert_array_equal(a_, b_)
    assert not np.array_equal(a_, c_), "another row 2, the same controls"
    assert graphed.graph_stats()["captures"] > captures
    np.testing.assert_array_equal(graphed.track_offset, np.full(B, 1))
    a_, b_, _ = step_all()
    np.testing.assert_array_equal(a_, b_)


def test_mode_and_error_handling():
    from mppi_numba_amd import _lib
    from mppi_numba_amd.barebone import MPPI_Batch, MPPI_Numba
    from mppi_numba_amd.mppi import MPPI_Numba as MapPlanner
    n, t = 128, 13
    params = make_params(DT, 1.0)
    track = crossing_goal(t, 9)
    planner = MPPI_Numba(cfg_of(n, t, False))
    planner.setup(goal_params(params, track))
    assert np.isfinite(planner.solve()).all()
    kernel = planner.last_rollout_kernel()
    assert kernel.endswith(" goal_rows=9"), kernel
    np.testing.assert_array_equal(planner.goal_now, track[0])
    both = goal_params(params, track)
    both["xgoal"] = params["xgoal"]
    planner.set_params(both)
    with pytest.raises(ValueError):  # a static goal or a track: one of the two
        planner.solve()
    for wrong in (track[:, 0], track.reshape(3, 3, 2), np.zeros((9, 3), np.float32), np.zeros((0, 2), np.float32)):
        planner.set_params(goal_params(params, wrong))
        with pytest.raises(ValueError):
            planner.solve()
    broken = track.copy()
    broken[4, 1] = np.nan
    planner.set_params(goal_params(params, broken))
    with pytest.raises(_lib.MppiError) as err:
        planner.solve()
    assert err.value.code == ERR_INVALID and "finite" in str(err.value), str(err.value)
    planner.set_params(goal_params(params, track))
    assert np.isfinite(planner.solve()).all() and planner.last_rollout_kernel() == kernel  # (refused: the handle kept its track)
    # the key goes: the static goal applies again
    planner.set_params(params)
    assert np.isfinite(planner.solve()).all()
    assert "goal_rows" not in planner.last_rollout_kernel()
    np.testing.assert_array_equal(planner.goal_now, np.float32(params["xgoal"]))
    # the C entry point: the wrong count, no rows, a map mode
    lib = _lib.load()
    flat = np.ascontiguousarray(np.stack([track, track]))
    assert lib.mppi_planner_set_goal_tracks(planner._handle, 2, 9, _lib.ptr(flat, C.c_float)) == ERR_INVALID
    assert "count" in lib.mppi_last_error().decode()
    assert lib.mppi_planner_set_goal_tracks(planner._handle, 1, 0, _lib.ptr(flat, C.c_float)) == ERR_INVALID
    assert "row" in lib.mppi_last_error().decode()
    batch = MPPI_Batch(cfg_of(64, t, False), 3)
    batch.setup(params)
    with pytest.raises(ValueError):  # a list with differing L
        batch.set_goal_tracks([track, track[:5], track])
    with pytest.raises(ValueError):  # the wrong count
        batch.set_goal_tracks([track, track])
    assert lib.mppi_planner_set_goal_tracks(batch._handle, 2, 9, _lib.ptr(flat, C.c_float)) == ERR_INVALID
    from test_gpu_batch import make_world
    mcfg, lin, ang, mparams = make_world("c2", 128, 20)
    mapped = MapPlanner(mcfg)
    mapped.setup(mparams, lin, ang)
    assert lib.mppi_planner_set_goal_tracks(mapped._handle, 1, 9, _lib.ptr(flat, C.c_float)) == ERR_INVALID
    assert "barebone" in lib.mppi_last_error().decode()
    # the default family's LDS: 40 static discs at 100 steps fit (16 * 100 + 16 * 40), their rows beside a goal track do not
    # (16 * 100 + 16 * 100 * 40 + 8 * 100 = 66 400 bytes) -- refused without crowd mode, the crowd kernel's with it
    big_t = 100
    rng = np.random.default_rng(3)
    pos, rad = random_discs(rng, 40, params["x0"], params["xgoal"])
    crowded = make_params(DT, 1.0, (pos, rad))
    big = MPPI_Numba(cfg_of(n, big_t, False))
    big.setup(crowded)
    assert np.isfinite(big.solve()).all()
    big.set_params(goal_params(crowded, crossing_goal(big_t, 30)))
    with pytest.raises(_lib.MppiError) as err:
        big.solve()
    assert err.value.code == ERR_INVALID and "66400 bytes" in str(err.value), str(err.value)
    big.set_crowd(True)
    assert np.isfinite(big.solve()).all()
    crowd_kernel = big.last_rollout_kernel()
    shape_of(crowd_kernel)
    assert crowd_kernel.endswith(" goal_rows=30"), crowd_kernel
    with pytest.raises(_lib.MppiError) as err:  # the set holds the handle in crowd mode
        big.set_crowd(False)
    assert err.value.code == ERR_INVALID and "goal track" in str(err.value), str(err.value)
    assert big.crowd


# The scenario, written down once (DESIGN.md section 8 has the figures): a robot at the origin, heading along x, follows a
# goal that starts 1.5 m ahead and 1 m to the left and keeps 1 m/s along x for 8 s, past two discs of radius 0.4 m whose
# edges are 0.2 m from its line.  goal_tolerance = 0: nothing freezes.  Horizon 3 s, 1024 rollouts, two iterations a step.
SCENARIO = dict(t=30, n=1024, steps=80, start=np.array([1.5, 1.0]), velocity=np.array([1.0, 0.0]),
                discs=(np.array([[3.0, 1.6], [5.5, 0.4]]), np.array([0.4, 0.4])))


def _follow(seed, tracked):
    """Mean distance to the goal's true position over the control steps after the first 2 s."""
    from mppi_numba_amd.barebone import MPPI_Numba, constant_velocity_tracks
    s = SCENARIO
    truth = constant_velocity_tracks([s["start"]], [s["velocity"]], DT, s["steps"] + s["t"] + 2)[0]
    params = make_params(DT, 1.0, s["discs"], num_opt=2)
    params["x0"], params["goal_tolerance"] = np.array([0.0, 0.0, 0.0]), 0.0
    if tracked:
        params = goal_params(params, truth)
    else:
        params["xgoal"] = truth[0]
    planner = MPPI_Numba(cfg_of(s["n"], s["t"], False, seed=seed))
    planner.setup(params)
    x = np.asarray(params["x0"], np.float64)
    gaps = []
    for step in range(s["steps"]):
        if not tracked:
            planner.params["xgoal"] = truth[step]  # the goal's present place, shown before every solve
        useq = planner.solve()
        x = _euler(x, useq[0], DT)
        planner.shift_and_update(x, useq, num_shifts=1)
        gaps.append(np.linalg.norm(x[:2] - truth[step + 1].astype(np.float64)))
    assert ("goal_rows" in planner.last_rollout_kernel()) == tracked
    assert planner.track_offset == (s["steps"] if tracked else 0)
    return float(np.mean(gaps[20:]))


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_following_a_moving_goal(seed):
    """The planner given the track against a planner that is shown the goal's present place as a static goal before every
    solve: over the steps after the first 2 s the tracked planner's mean distance to the goal's true position is smaller."""
    tracked, reaimed = _follow(seed, True), _follow(seed, False)
    print("seed %d: mean distance to the moving goal after 2 s: with the track %.4f m, re-aimed static goal %.4f m" % (seed, tracked, reaimed))
    assert tracked < reaimed


def test_intercept_ends_before_max_steps():
    """A positive tolerance: closed_loop ends early, at a goal that crosses the robot's reach -- within the tolerance of where
    the goal is then, not of where it started."""
    from mppi_numba_amd.barebone import MPPI_Numba
    max_steps = 70
    track = intercept_track(60)
    params = goal_params(make_params(DT, 1.0), track)
    params["x0"] = np.array([0.0, 0.0, 0.0])
    planner = MPPI_Numba(cfg_of(1024, 30, False, seed=2))
    planner.setup(params)
    xhist, _, steps = planner.closed_loop(max_steps)
    assert 0 < steps < max_steps, steps
    end = xhist[steps, :2]
    assert planner.track_offset == steps
    assert np.linalg.norm(end - track[steps].astype(np.float64)) <= params["goal_tolerance"]
    assert np.linalg.norm(end - track[0].astype(np.float64)) > params["goal_tolerance"]
    assert np.isnan(xhist[steps + 1:]).all()
