"""Walls that move, and a wall set per problem, in the barebone planner's crowd mode: params['wall_tracks'] (W, L, 2, 2),
MPPI_Batch.set_wall_sets, mppi_planner_set_wall_tracks.  Row j of a wall is the segment it occupies during control interval
j after "now"; step t of a rollout is tested against row min(track_offset + t, L - 1).  k_rollout_barebone_crowd's
CrowdWallTracks form counts these hits beside a step's disc hits; every comparison of costs here is bit for bit with
tests/wall_track_model.py (whose row selection tests/test_wall_track_model.py pins on the CPU) unless it says otherwise."""
import functools

import numpy as np
import pytest

from test_gpu_barebone_batch import ERR_INVALID, make_params, oracle_params, problem_params, problems
from test_gpu_barebone_crowd import cfg_of, inputs, shape_of
from test_gpu_barebone_tracks import track_params
from test_gpu_barebone_walls import (DIAG, N, OBS_PENALTY, assert_bits, building, discs_of, rollout_with, task, wall_params,
                                     without_walls)
from crowd_model import hit_counts
from wall_model import active_steps, chain, hit, pure_crossing, wall_hits_of_states
from wall_track_model import wall_track_costs, wall_track_hits_of_states

pytestmark = pytest.mark.gpu

DT = 0.1


@functools.lru_cache(maxsize=None)
def moving_building(count, rows):
    """building(count) with `rows` rows: wall 0, the thin wall that is jumped, drifts along the diagonal at 0.4 m/s (away
    from the start); walls 1 .. 3 stand; the scattered walls keep random velocities of up to 0.3 m/s a component."""
    from mppi_numba_amd.barebone import constant_velocity_walls
    seg, hw = building(count)
    vel = np.random.default_rng(count + 3).uniform(-0.3, 0.3, (count, 2))
    vel[:4] = 0.0
    vel[0] = 0.4 * DIAG
    tracks = constant_velocity_walls(seg, vel, DT, rows, at=0.0)
    assert (tracks[:, 0] == seg).all()
    tracks.setflags(write=False)
    return tracks, hw


def track_wall_params(params, tracks, hw):
    p = without_walls(params)
    p["wall_tracks"], p["wall_halfwidth"] = tracks, hw
    return p


def the_moving_input_means_something(p, disc_tracks, rad, wtracks, hw, noise, u_in, offset):
    """Asserted with the model, on the CPU, before anything is compared: a step jumps wall 0 where that wall IS at the step;
    from four walls on a (rollout, step) pair has two wall hits; and with more than one row the hit counts differ from those
    of the row-0 static set -- else the case could not tell the rows apart."""
    W, Lw = wtracks.shape[:2]
    disc_counts, st = hit_counts(p, disc_tracks, rad, noise, u_in, offset)
    T = st.shape[1] - 1
    rows = np.minimum(offset + np.arange(T), Lw - 1)
    P, Q = st[:, :-1, :2], st[:, 1:, :2]
    assert pure_crossing(P, Q, wtracks[0, rows, 0][None], wtracks[0, rows, 1][None], hw[0]).any(), "bad input: no step jumps the thin wall"
    walls = wall_track_hits_of_states(st, wtracks, hw, offset)
    if W >= 4:
        assert (walls >= 2).any(), "bad input: no (rollout, step) pair has two wall hits"
    if Lw > 1:
        assert (walls != wall_hits_of_states(st, wtracks[:, 0], hw)).any(), "bad input: the rows cannot be told apart"
    return chain(p, disc_counts + walls, st, noise, u_in)


def disc_case(K, kind, t, params):
    """(disc tracks for the model, radii, params with these discs and no walls)."""
    where, rad = discs_of(K, kind, t, params)
    if kind == "tracks":
        tracks, full = where, track_params(params, where, rad)
    else:
        tracks, full = where[:, None, :], problem_params(params, params["x0"], params["xgoal"], (where, rad))
    full["x0"], full["xgoal"] = params["x0"], params["xgoal"]
    return tracks, rad, full


CASES = [(W, K, kind, t, wscale, rows) for W in (1, 64, 65, 130) for K, kind in ((0, "static"), (70, "static"), (70, "tracks"))
         for t, wscale in ((30, 1.0), (37, 1.5)) for rows in (1, 12, -6)]  # (-6: T + 6 rows)


@pytest.mark.parametrize("W,K,kind,t,wscale,rows", CASES)
def test_costs_equal_the_model(W, K, kind, t, wscale, rows):
    """Exact math, rotation on (wscale 1.0) and off (1.5); T = 30 and 37: more than one chunk, no multiple of the counters.
    12 rows are fewer than the horizon (the clamp takes part mid-rollout); with T + 6 rows offset 5 reads rows that offset 0
    never does; offset Lw + 3 lies past the end.  The disc tracks have T + 1 rows: never the walls' count."""
    from mppi_numba_amd.barebone import MPPI_Numba
    params, u_in, noise = task(t, wscale)
    Lw = t + 6 if rows < 0 else rows
    wtracks, hw = moving_building(W, Lw)
    tracks, rad, full = disc_case(K, kind, t, params)
    assert kind != "tracks" or tracks.shape[1] != Lw
    p = oracle_params(without_walls(params))
    planner = MPPI_Numba(cfg_of(N, t, True))
    planner.set_params(track_wall_params(full, wtracks, hw))
    for offset in (0, 5, Lw + 3):
        model = the_moving_input_means_something(p, tracks, rad, wtracks, hw, noise, u_in, offset)
        planner.move_mppi_task_vars_to_device()  # (hands the tracks over the first time: offset 0)
        planner.set_track_offset(offset)
        got, _, _, kernel = rollout_with(planner, u_in, noise)
        assert t > shape_of(kernel)[1], kernel
        assert kernel.endswith(" walls=%d wall_rows=%d" % (W, Lw)), kernel
        assert ("rotation=1" in kernel) == (wscale == 1.0) and "exact=1" in kernel, kernel
        assert ("tracks=%d" % (t + 1) in kernel) == (kind == "tracks"), kernel
        assert_bits(got, model, "%d walls x %d rows, %d discs (%s), offset %d vs the model" % (W, Lw, K, kind, offset))


@pytest.mark.parametrize("W,K,kind,t", [(1, 0, "static", 30), (65, 70, "tracks", 37), (130, 70, "static", 30)])
def test_equal_rows_equal_static_walls(W, K, kind, t):
    from mppi_numba_amd.barebone import MPPI_Numba
    params, u_in, noise = task(t, 1.0)
    seg, hw = building(W)
    _, _, full = disc_case(K, kind, t, params)
    static = MPPI_Numba(cfg_of(N, t, True))
    static.set_params(wall_params(full, seg, hw))
    moving = MPPI_Numba(cfg_of(N, t, True))
    for Lw in (1, 7):
        moving.set_params(track_wall_params(full, np.repeat(seg[:, None], Lw, axis=1), hw))
        for offset in (0, 3, Lw + 2):
            for planner in (static, moving):
                planner.move_mppi_task_vars_to_device()
                planner.set_track_offset(offset)
            want, want_u, _, static_kernel = rollout_with(static, u_in, noise)
            got, got_u, _, kernel = rollout_with(moving, u_in, noise)
            assert static_kernel.endswith(" walls=%d" % W) and kernel.endswith(" walls=%d wall_rows=%d" % (W, Lw)), (static_kernel, kernel)
            assert (want > OBS_PENALTY).any()
            assert_bits(got, want, "%d rows, offset %d: equal rows vs static walls" % (Lw, offset))
            assert_bits(got_u, want_u, "... u")


def test_fast_math_adds_the_wall_hits():
    """test_gpu_barebone_walls.test_fast_math_adds_the_wall_hits with walls that move -- its argument and its bounds, the
    model's hits taken row by row: a launch with the wall tracks and a launch without differ by the model's wall hits (of
    the steps before the freeze) times obs_cost, exactly for the rollouts whose verdicts all stay the same for half-widths
    1e-4 m smaller and larger and whose goal tests are 1e-4 m clear of the tolerance (at least 80 % of them), within the
    range of hits those margins allow for the others; the difference of the two chains within (2T + 2 + hits) ulps."""
    from mppi_numba_amd.barebone import MPPI_Numba
    W, Lw, K, kind, t, offset = 65, 12, 3, "static", 37, 2
    params, u_in, noise = task(t, 1.0)
    wtracks, hw = moving_building(W, Lw)
    tracks, rad, base = disc_case(K, kind, t, params)
    p = oracle_params(without_walls(params))
    the_moving_input_means_something(p, tracks, rad, wtracks, hw, noise, u_in, offset)
    planner = MPPI_Numba(cfg_of(N, t, True, math="fast"))
    planner.set_params(base)
    absent, _, _, kernel_absent = rollout_with(planner, u_in, noise)
    planner.set_params(track_wall_params(base, wtracks, hw))
    planner.move_mppi_task_vars_to_device()
    planner.set_track_offset(offset)
    present, _, _, kernel = rollout_with(planner, u_in, noise)
    assert "walls" not in kernel_absent and kernel.endswith(" walls=%d wall_rows=%d" % (W, Lw)) and "exact=0" in kernel, (kernel_absent, kernel)
    shape_of(kernel)
    disc_counts, st = hit_counts(p, tracks, rad, noise, u_in, offset)
    walls = wall_track_hits_of_states(st, wtracks, hw, offset)
    margin = np.float32(1e-4)
    thick = hw > 0
    fewest, most = np.zeros_like(walls), wall_track_hits_of_states(st, wtracks, hw + margin, offset)
    fewest += wall_track_hits_of_states(st, wtracks[thick], np.maximum(hw[thick] - margin, 0), offset)
    assert (~thick).any()
    for step in range(t):  # half-width 0: segments that meet stop meeting only by way of an endpoint of one ON the other
        row = min(offset + step, Lw - 1)
        P, Q = st[:, step, None, :2], st[:, step + 1, None, :2]
        A, B = wtracks[None, ~thick, row, 0], wtracks[None, ~thick, row, 1]
        touching = hit(P, P, A, B, margin) | hit(Q, Q, A, B, margin) | hit(P, Q, A, A, margin) | hit(P, Q, B, B, margin)
        fewest[:, step] += (hit(P, Q, A, B, hw[~thick]) & ~touching).sum(axis=1)
    assert (fewest <= walls).all() and (walls <= most).all()
    tol = float(np.float32(params["goal_tolerance"]))
    goal_d = np.linalg.norm(st[:, 1:, :2].astype(np.float64) - np.float32(params["xgoal"]).astype(np.float64), axis=2)
    surely, maybe = goal_d <= tol - 1e-4, goal_d <= tol + 1e-4
    active_least = (np.cumsum(maybe, axis=1) - maybe) == 0    # frozen as early as can be
    active_most = (np.cumsum(surely, axis=1) - surely) == 0   # ... as late as can be
    active = active_steps(p, st)
    want_hits = (walls * active).sum(axis=1)
    lowest, highest = (fewest * active_least).sum(axis=1), (most * active_most).sum(axis=1)
    steady = lowest == highest
    assert (lowest <= want_hits).all() and (want_hits <= highest).all()
    assert steady.mean() >= 0.8, "bad input: only %.0f %% of the rollouts are clear of every boundary" % (100 * steady.mean())
    assert (want_hits[steady] > 0).any()
    diff = present.astype(np.float64) - absent.astype(np.float64)
    got_hits = np.rint(diff / OBS_PENALTY).astype(np.int64)
    print("fast math: %d of %d rollouts steady, wall hits up to %d, widest range %d" % (steady.sum(), N, want_hits.max(), (highest - lowest).max()))
    assert (got_hits[steady] == want_hits[steady]).all(), "%d rollouts differ in their hits" % (got_hits[steady] != want_hits[steady]).sum()
    assert ((lowest <= got_hits) & (got_hits <= highest)).all(), "rollouts %s are outside their range of hits" % np.nonzero((got_hits < lowest) | (got_hits > highest))[0]
    ops = 2 * t + 2 + got_hits + disc_counts.sum(axis=1) + (highest - lowest)
    bound = ops * np.spacing(present).astype(np.float64)
    assert (np.abs(diff - got_hits * OBS_PENALTY) <= bound).all()


def problem_walls(rng, count, x0, goal, rows=None):
    """`count` walls around the segment start -> goal; rows: tracks, each wall keeping a velocity of up to 0.5 m/s a component."""
    from mppi_numba_amd.barebone import constant_velocity_walls
    s = rng.uniform(0.1, 0.9, (count, 1))
    a = np.asarray(x0, np.float64)[:2] * (1 - s) + np.asarray(goal, np.float64) * s + rng.normal(0, 0.4, (count, 2))
    seg = np.stack([a, a + rng.uniform(-1.0, 1.0, (count, 2))], axis=1).astype(np.float32)
    hw = rng.uniform(0.0, 0.2, count).astype(np.float32)
    if rows is None:
        return seg, hw
    return constant_velocity_walls(seg, rng.uniform(-0.5, 0.5, (count, 2)), DT, rows), hw


def test_batch_with_per_problem_wall_sets():
    """n = 64 per problem (a batched handle takes whole tiles).  Every problem against a single-problem planner given its
    set and offset, and against the model; then back to the shared walls of params; then empty sets against no walls."""
    from mppi_numba_amd.barebone import MPPI_Batch, MPPI_Numba
    counts, offsets = [0, 1, 70], np.array([0, 3, 40], dtype=np.int32)
    B, n, t, Lw = len(counts), 64, 30, 45
    rng = np.random.default_rng(23)
    x0s, goals = problems(rng, B)
    params = make_params(DT, 1.0)
    shared = problem_walls(rng, 5, x0s[0], goals[0])
    static_sets = [problem_walls(rng, k, x0s[b], goals[b]) for b, k in enumerate(counts)]
    track_sets = [problem_walls(rng, k, x0s[b], goals[b], Lw) for b, k in enumerate(counts)]
    u_in = np.stack([inputs(rng, n, t)[0] for _ in range(B)])
    noise = rng.normal(0, 0.5, (B, n, t, 2)).astype(np.float32)
    none = np.zeros((0, 1, 2), np.float32), np.zeros(0, np.float32)
    batch = MPPI_Batch(cfg_of(n, t, True), B)
    batch.setup(wall_params(params, *shared), x0s, goals, wall_sets=static_sets)  # (the per-problem sets win)
    single = MPPI_Numba(cfg_of(n, t, True))
    for kind, sets in (("static", static_sets), ("tracks", track_sets)):
        batch.set_wall_sets(sets)
        if kind == "tracks":
            np.testing.assert_array_equal(batch.track_offset, np.zeros(B))
            batch.set_track_offset(offsets)
        costs, u_out, _, kernel = rollout_with(batch, u_in, noise.reshape(B * n, t, 2))
        shape_of(kernel)
        assert "problems=%d" % B in kernel and kernel.endswith(" walls=70 wall_rows=%d" % (Lw if kind == "tracks" else 1)), kernel
        for b in range(B):
            pb = problem_params(params, x0s[b], goals[b])
            seg, hw = sets[b]
            wtracks = seg if kind == "tracks" else seg[:, None]
            offset = int(offsets[b]) if kind == "tracks" else 0
            if counts[b]:
                single.set_params(track_wall_params(pb, seg, hw) if kind == "tracks" else wall_params(pb, seg, hw))
            else:
                single.set_params(pb)
            single.move_mppi_task_vars_to_device()
            single.set_track_offset(offset)
            want, want_u, _, single_kernel = rollout_with(single, u_in[b], noise[b])
            assert ("walls=%d" % counts[b] in single_kernel) == (counts[b] > 0), single_kernel
            what = "problem %d (%d walls, %s, offset %d)" % (b, counts[b], kind, offset)
            assert_bits(costs[b], want, what + " vs a single handle")
            assert_bits(u_out[b], want_u, what + " u vs a single handle")
            p = oracle_params(pb)
            model = wall_track_costs(p, none[0], none[1], wtracks, hw, noise[b], u_in[b], offset)
            if counts[b] == 70:
                st = hit_counts(p, none[0], none[1], noise[b], u_in[b])[1]
                hits = wall_track_hits_of_states(st, wtracks, hw, offset)
                assert hits.any(), "bad input: problem %d hits no wall" % b
                if kind == "tracks":
                    assert (hits != wall_track_hits_of_states(st, wtracks, hw, 0)).any(), "bad input: the offset shows nowhere"
            assert_bits(costs[b], model, what + " vs the model")
    # the same sets again: no change, the offsets stay
    batch.set_wall_sets(track_sets)
    np.testing.assert_array_equal(batch.track_offset, offsets)
    again, _, _, _ = rollout_with(batch, u_in, noise.reshape(B * n, t, 2))
    assert_bits(again, costs, "same sets again")
    # mixed kinds are refused, and the handle keeps what it had
    with pytest.raises(ValueError):
        batch.set_wall_sets([static_sets[0], track_sets[1], track_sets[2]])
    again, _, _, _ = rollout_with(batch, u_in, noise.reshape(B * n, t, 2))
    assert_bits(again, costs, "after a refused call")
    # back to the shared walls of params
    batch.set_wall_sets(None)
    back, _, _, kernel = rollout_with(batch, u_in, noise.reshape(B * n, t, 2))
    assert kernel.endswith(" walls=5"), kernel
    for b in range(B):
        p = oracle_params(problem_params(params, x0s[b], goals[b]))
        assert_bits(back[b], wall_track_costs(p, none[0], none[1], shared[0][:, None], shared[1], noise[b], u_in[b]),
                    "problem %d, shared walls again" % b)
    # sets that are all empty: a batch without walls
    batch.set_wall_sets([(np.zeros((0, 2, 2), np.float32), 0.0)] * B)
    empty, _, _, kernel = rollout_with(batch, u_in, noise.reshape(B * n, t, 2))
    assert kernel.endswith(" walls=0 wall_rows=1"), kernel
    plain = MPPI_Batch(cfg_of(n, t, True), B)
    plain.setup(params, x0s, goals)
    want, _, _, kernel = rollout_with(plain, u_in, noise.reshape(B * n, t, 2))
    assert "walls" not in kernel, kernel
    assert_bits(empty, want, "empty sets vs a batch without walls")


def test_offsets_advance_with_wall_tracks_alone():
    """No disc tracks: the wall tracks alone make shift_and_update* and closed_loop advance "now"."""
    from mppi_numba_amd.barebone import MPPI_Batch, MPPI_Numba
    t, Lw = 30, 45
    params, u_in, noise = task(t, 1.0)
    wtracks, hw = moving_building(65, Lw)
    p = oracle_params(without_walls(params))
    none = np.zeros((0, 1, 2), np.float32), np.zeros(0, np.float32)
    planner = MPPI_Numba(cfg_of(N, t, True))
    planner.setup(track_wall_params(params, wtracks, hw))
    useq = planner.solve()
    assert planner.track_offset == 0
    planner.shift_and_update(np.asarray(params["x0"]), useq, num_shifts=3)
    assert planner.track_offset == 3
    planner.shift_and_update(np.asarray(params["x0"]), useq, num_shifts=1)
    assert planner.track_offset == 4
    got, _, _, kernel = rollout_with(planner, u_in, noise)
    assert kernel.endswith(" walls=65 wall_rows=%d" % Lw) and "tracks=" not in kernel, kernel
    at0 = wall_track_costs(p, none[0], none[1], wtracks, hw, noise, u_in, 0)
    at4 = wall_track_costs(p, none[0], none[1], wtracks, hw, noise, u_in, 4)
    assert (at0 != at4).any()
    assert_bits(got, at4, "after four shifts vs the model at offset 4")
    planner.params["wall_tracks"] = wtracks.copy()  # the same tracks as a new object: "now" stays
    again, _, _, _ = rollout_with(planner, u_in, noise)
    assert planner.track_offset == 4
    assert_bits(again, at4, "unchanged tracks leave the offset alone")
    moved = wtracks.copy()
    moved[:, 1:] += np.float32(0.01)
    planner.params["wall_tracks"] = moved  # new tracks: row 0 is "now"
    fresh, _, _, _ = rollout_with(planner, u_in, noise)
    assert planner.track_offset == 0
    assert_bits(fresh, wall_track_costs(p, none[0], none[1], moved, hw, noise, u_in, 0), "new tracks vs the model at offset 0")
    # closed loop on the device, per problem
    B, n, max_steps = 3, 64, 40
    rng = np.random.default_rng(21)
    x0s, goals = problems(rng, B)
    sets = [problem_walls(rng, k, x0s[b], goals[b], Lw) for b, k in enumerate((40, 3, 0))]  # (the goal within reach: no walls in the way)
    bparams = make_params(DT, 1.0)
    batch = MPPI_Batch(cfg_of(n, t, True), B)
    batch.setup(bparams, x0s, goals, wall_sets=sets)
    before = np.array([2, 0, 5], dtype=np.int32)
    batch.set_track_offset(before)
    _, _, steps = batch.closed_loop(max_steps)
    print("closed loop with wall tracks alone: steps", steps)
    assert batch.last_rollout_kernel().endswith(" walls=40 wall_rows=%d" % Lw)
    np.testing.assert_array_equal(batch.track_offset, before + steps)
    assert steps[-1] < max_steps and steps.max() > steps[-1]  # the goal within reach is reached early: it stopped advancing
    bu = np.stack([inputs(rng, n, t)[0] for _ in range(B)])
    bnoise = rng.normal(0, 0.5, (B, n, t, 2)).astype(np.float32)
    costs, _, _, _ = rollout_with(batch, bu, bnoise.reshape(B * n, t, 2))
    np.testing.assert_array_equal(batch.track_offset, before + steps)
    for b in range(B):
        pb = oracle_params(problem_params(bparams, batch.x0s[b], goals[b]))
        assert_bits(costs[b], wall_track_costs(pb, none[0], none[1], sets[b][0], sets[b][1], bnoise[b], bu[b], int(before[b] + steps[b])),
                    "problem %d after %d control steps vs the model" % (b, steps[b]))


def test_solve_under_graph_replay_and_wall_track_changes():
    """As test_gpu_barebone_walls.test_solve_under_graph_replay_and_wall_changes compares: a direct loop and a replayed one
    in step, equal at every solve -- through a change of one row of the tracks and through set_track_offset."""
    from mppi_numba_amd.barebone import MPPI_Batch
    B, n, t, Lw = 4, 128, 30, 20
    rng = np.random.default_rng(9)
    x0s, goals = problems(rng, B)
    a = rng.uniform(-1.0, 4.0, (70, 2))
    seg = np.stack([a, a + rng.uniform(-1.0, 1.0, (70, 2))], axis=1)
    hw = rng.uniform(0.0, 0.15, 70).astype(np.float32)
    from mppi_numba_amd.barebone import constant_velocity_walls
    wtracks = constant_velocity_walls(seg, rng.uniform(-0.4, 0.4, (70, 2)), DT, Lw)
    params = track_wall_params(make_params(DT, 1.0, num_opt=5), wtracks, hw)
    direct, graphed, kept = (MPPI_Batch(cfg_of(n, t, True), B) for _ in range(3))
    for planner in (direct, graphed, kept):
        planner.setup(params, x0s, goals)
    graphed.set_graph_replay(True, 2)
    x = x0s.copy()

    def step_all():
        nonlocal x
        out = [planner.solve() for planner in (direct, graphed, kept)]
        x = x + np.float32([0.05, 0.04, 0.01])
        for planner in (direct, graphed, kept):
            planner.shift_and_update_on_device(x, num_shifts=1)
        return out

    for _ in range(3):
        a_, b_, c_ = step_all()
        np.testing.assert_array_equal(a_, b_)
        np.testing.assert_array_equal(a_, c_)
    kernel = graphed.last_rollout_kernel()
    assert kernel.startswith("k_rollout_barebone_crowd") and kernel.endswith(" walls=70 wall_rows=%d" % Lw), kernel
    np.testing.assert_array_equal(graphed.track_offset, np.full(B, 3))
    assert graphed.graph_stats()["replays"] >= 2, graphed.graph_stats()
    captures = graphed.graph_stats()["captures"]
    # one row of the tracks changes: new tracks (row 0 is "now"), another result, the same under replay and directly
    changed = wtracks.copy()
    changed[:, 2] += np.float32([0.3, -0.2])
    for planner in (direct, graphed):
        planner.params["wall_tracks"] = changed
    kept.set_track_offset(0)  # (what new tracks do to the other two)
    a_, b_, c_ = step_all()
    np.testing.assert_array_equal(a_, b_)
    assert not np.array_equal(a_, c_), "another row 2, the same controls"
    assert graphed.graph_stats()["captures"] > captures
    np.testing.assert_array_equal(graphed.track_offset, np.full(B, 1))
    a_, b_, _ = step_all()
    np.testing.assert_array_equal(a_, b_)
    # "now" set by hand
    for planner in (direct, graphed):
        planner.set_track_offset(4)
    for _ in range(2):
        a_, b_, _ = step_all()
        np.testing.assert_array_equal(a_, b_)
    np.testing.assert_array_equal(graphed.track_offset, np.full(B, 6))
    np.testing.assert_array_equal(direct.track_offset, np.full(B, 6))


def _plan_positions(x, useq, dt):
    """(T + 1, 2) float64: where the nominal unicycle goes from state x under useq (the notebook's Euler step)."""
    out = np.empty((len(useq) + 1, 2))
    x = np.array(x, dtype=np.float64)
    out[0] = x[:2]
    for j, u in enumerate(useq.astype(np.float64)):
        x = x + dt * np.array([np.cos(x[2]) * u[0], np.sin(x[2]) * u[0], u[1]])
        out[j + 1] = x[:2]
    return out


def _corridor_run(seed, swept):
    """Two robots of radius 0.25 m meet head-on in a corridor 2.4 m wide and would swap places.  One planner each; in every
    control step A plans first, then B, each against the other's last plan from "now" on -- as swept_walls tracks of
    half-width 0.5 m (the sum of the radii), or as disc tracks of that radius.  Returns the smallest true clearance of the
    executed motion (both move linearly within a control step: 16 samples per step) and the steps taken."""
    from mppi_numba_amd.barebone import Config, MPPI_Numba, swept_walls
    T, dt, max_steps, reach = 30, 0.1, 90, 0.5
    corridor = np.float32([[[-2.0, 1.2], [8.0, 1.2]], [[-2.0, -1.2], [8.0, -1.2]]])
    starts, goals = np.array([[0.0, 0.0, 0.0], [6.0, 0.0, np.pi]]), np.array([[6.0, 0.0], [0.0, 0.0]])
    planners, x, plans = [], starts.copy(), []
    for r in range(2):
        cfg = Config(T=(T + 0.5) * dt, dt=dt, num_control_rollouts=1024, num_vis_state_rollouts=4, seed=seed + 10 * r,
                     enforce_recommended_limits=False, crowd=True)
        planner = MPPI_Numba(cfg)
        planner.setup(dict(dt=dt, x0=starts[r].copy(), xgoal=goals[r], goal_tolerance=0.3, dist_weight=10, lambda_weight=1.0,
                           num_opt=2, u_std=np.array([1.0, 1.0]), vrange=np.array([0.0, 2.0]),
                           wrange=np.array([-np.pi, np.pi]), obs_penalty=1e6))
        planners.append(planner)
        plans.append(np.repeat(starts[r][None, :2], T + 1, axis=0))  # (nothing planned yet: it stands)
    clearance, done, steps = np.inf, [False, False], 0
    for step in range(max_steps):
        before = x.copy()
        for r in range(2):
            if done[r]:
                continue
            other = plans[1 - r][None]  # (1, rows, 2): the other's positions from now on
            prm = planners[r].params
            for key in ("wall_tracks", "wall_segments", "wall_halfwidth", "obstacle_tracks", "obstacle_radius"):
                prm.pop(key, None)
            if swept:
                sweeps = swept_walls(other)
                prm["wall_tracks"] = np.concatenate([sweeps, np.repeat(corridor[:, None], sweeps.shape[1], axis=1)])
                prm["wall_halfwidth"] = np.float32([reach, 0.05, 0.05])
            else:
                prm["obstacle_tracks"], prm["obstacle_radius"] = other.astype(np.float32), np.float32([reach])
                prm["wall_segments"], prm["wall_halfwidth"] = corridor, np.float32(0.05)
            useq = planners[r].solve()
            plans[r] = _plan_positions(x[r], useq, dt)
            u = useq[0].astype(np.float64)
            x[r] = x[r] + dt * np.array([np.cos(x[r, 2]) * u[0], np.sin(x[r, 2]) * u[0], u[1]])
            planners[r].shift_and_update(x[r], useq, num_shifts=1)
        for r in range(2):  # what is left of a plan once its first step is taken (a robot at its goal stands)
            plans[r] = np.repeat(x[r][None, :2], T + 1, axis=0) if done[r] else np.concatenate([plans[r][1:], plans[r][-1:]])
        s = np.linspace(0.0, 1.0, 16)[:, None]
        gap = (before[0, :2] + s * (x[0, :2] - before[0, :2])) - (before[1, :2] + s * (x[1, :2] - before[1, :2]))
        clearance = min(clearance, np.linalg.norm(gap, axis=1).min() - reach)
        steps = step + 1
        for r in range(2):
            if not done[r] and np.linalg.norm(x[r, :2] - goals[r]) <= 0.3:
                done[r] = True
                plans[r] = np.repeat(x[r][None, :2], T + 1, axis=0)
        if all(done):
            break
    kernel = planners[0].last_rollout_kernel()
    assert ("wall_rows=" in kernel) == swept, kernel
    return clearance, steps, all(done)


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_two_robots_meet_in_a_corridor(seed):
    """The swept capsules keep the executed motion clear; the same run with the other's plan as disc tracks -- instants,
    which a head-on swap within one control step slips between -- is reported beside it, not asserted.  (On the MI355X, with
    the parameters as they were first written down, seeds 1 / 2 / 3: smallest clearance with swept walls 0.032 / 0.019 /
    0.026 m, with disc tracks 0.013 / 0.067 / -0.011 m; 31 - 32 control steps either way.)"""
    clear_swept, steps_swept, done_swept = _corridor_run(seed, True)
    clear_discs, steps_discs, done_discs = _corridor_run(seed, False)
    print("seed %d: swept walls: smallest clearance %.4f m in %d steps (both at their goals: %s); disc tracks: %.4f m in %d steps (%s)"
          % (seed, clear_swept, steps_swept, done_swept, clear_discs, steps_discs, done_discs))
    assert clear_swept >= 0.0, "the robots that take each other's swept plans touched"


def test_mode_and_error_handling():
    from mppi_numba_amd import _lib
    from mppi_numba_amd.barebone import MPPI_Batch, MPPI_Numba
    n, t, Lw = 128, 30, 9
    wtracks, hw = moving_building(6, Lw)
    seg = np.ascontiguousarray(wtracks[:, 0])
    params = make_params(DT, 1.0)
    planner = MPPI_Numba(cfg_of(n, t, False))
    planner.setup(params)
    assert np.isfinite(planner.solve()).all()
    plain = planner.last_rollout_kernel()
    assert plain.startswith("k_rollout_barebone exact"), plain
    planner.set_params(track_wall_params(params, wtracks, hw))
    with pytest.raises(_lib.MppiError) as err:  # no crowd mode: no wall tracks
        planner.solve()
    assert err.value.code == ERR_INVALID and "crowd" in str(err.value), str(err.value)
    planner.set_crowd(True)
    assert np.isfinite(planner.solve()).all()
    kernel = planner.last_rollout_kernel()
    shape_of(kernel)
    assert kernel.endswith(" walls=6 wall_rows=%d" % Lw), kernel
    with pytest.raises(_lib.MppiError) as err:  # the wall tracks hold the handle in crowd mode
        planner.set_crowd(False)
    assert err.value.code == ERR_INVALID and "wall tracks" in str(err.value), str(err.value)
    assert planner.crowd
    both = track_wall_params(params, wtracks, hw)
    both["wall_segments"] = seg
    planner.set_params(both)
    with pytest.raises(ValueError):  # static or tracks: one of the two
        planner.solve()
    for wrong in (seg, wtracks[:, :, 0], wtracks.reshape(6, Lw, 4), np.zeros((6, 0, 2, 2), np.float32)):
        planner.set_params(track_wall_params(params, wrong, hw))
        with pytest.raises(ValueError):
            planner.solve()
    planner.set_params(track_wall_params(params, wtracks, hw[:4]))
    with pytest.raises(ValueError):
        planner.solve()
    bad = hw.copy()
    bad[2] = -0.1
    planner.set_params(track_wall_params(params, wtracks, bad))
    with pytest.raises(_lib.MppiError) as err:
        planner.solve()
    assert err.value.code == ERR_INVALID and "half-width" in str(err.value), str(err.value)
    broken = wtracks.copy()
    broken[1, 3, 0, 1] = np.nan
    planner.set_params(track_wall_params(params, broken, hw))
    with pytest.raises(_lib.MppiError) as err:
        planner.solve()
    assert err.value.code == ERR_INVALID and "finite" in str(err.value), str(err.value)
    planner.set_params(track_wall_params(params, wtracks, hw))
    assert np.isfinite(planner.solve()).all() and planner.last_rollout_kernel() == kernel  # (refused: the handle kept its tracks)
    # the key goes: the tracks are cleared, the costs are those of a planner without walls, and crowd mode can go
    rng = np.random.default_rng(4)
    u_in, noise = inputs(rng, n, t)
    with_walls, _, _, _ = rollout_with(planner, u_in, noise)
    planner.set_params(params)
    got, _, _, cleared = rollout_with(planner, u_in, noise)
    assert cleared == plain, cleared
    bare = MPPI_Numba(cfg_of(n, t, True))
    bare.setup(params)
    want, _, _, _ = rollout_with(bare, u_in, noise)
    assert_bits(got, want, "tracks cleared vs a planner without walls")
    assert (with_walls != want).any()
    planner.set_crowd(False)
    assert not planner.crowd
    # a batch: mixed static and track sets
    batch = MPPI_Batch(cfg_of(64, t, True), 2)
    batch.setup(params)
    with pytest.raises(ValueError):
        batch.set_wall_sets([(seg, hw), (wtracks, hw)])
    with pytest.raises(ValueError):  # one row count per call
        batch.set_wall_sets([(wtracks, hw), (wtracks[:, :4], hw)])
