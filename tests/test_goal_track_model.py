"""CPU checks of the goal tracks' model (tests/goal_track_model.py; the row selection of k_rollout_barebone's goal forms
and of k_rollout_barebone_crowd's GoalRows argument): equal rows are the static goal to the bit -- the oracle's own costs --,
the row a step sees and the clamp, and a track of one row.  Plus the C ABI's new entry point: declared, bound, exported."""
import os
import re

import numpy as np
import pytest

from crowd_model import hit_counts
from goal_track_model import NO_DISCS, chain, freeze_step, goal_d2, goal_rows, goal_track_costs
from oracle import oracle as O
from test_crowd_model import _problem
from test_wall_track_model import some_walls
from track_model import oracle_params
from wall_track_model import wall_track_costs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _same_bits(a, b):
    return a.dtype == b.dtype == np.float32 and (a.view(np.int32) == b.view(np.int32)).all()


@pytest.mark.parametrize("T,K,wscale", [(30, 0, 1.0), (30, 5, 2.0), (37, 3, 1.0), (37, 70, 1.0)])
def test_equal_rows_are_the_static_goal(T, K, wscale):
    """Tracks of 1, T and T + 6 equal rows at offsets 0, 5 and L + 3: the bits of oracle.rollout_barebone; with walls (and
    the discs as tracks) the bits of wall_track_costs.  T = 37: rollouts reach the goal and freeze."""
    rng, params, pos, rad, u, noise = _problem(T, K, wscale)
    p = oracle_params(params)
    want = O.rollout_barebone(p, pos, rad, noise, u)
    goal = np.float32(params["xgoal"])
    seg, hw = some_walls(rng, 9, params["x0"], params["xgoal"])
    wtracks = np.repeat(seg[:, None], 4, axis=1)
    discs = np.repeat(pos[:, None], 3, axis=1)
    want_walls = wall_track_costs(p, discs, rad, wtracks, hw, noise, u)
    assert (want_walls != want).any(), "bad input: no wall is hit"
    for L in (1, T, T + 6):
        track = np.repeat(goal[None], L, axis=0)
        for offset in (0, 5, L + 3):
            got = goal_track_costs(p, track, noise, u, offset, pos[:, None], rad)
            assert _same_bits(got, want), (L, offset)
            got = goal_track_costs(p, track, noise, u, offset, discs, rad, wtracks, hw)
            assert _same_bits(got, want_walls), (L, offset, "walls")
    if T == 37:
        st = hit_counts(p, *NO_DISCS, noise, u)[1]
        froze = freeze_step(p, goal_rows(goal[None], T), st)
        assert (froze < T).any() and (froze == T).any(), "bad input: the freeze takes no part"


@pytest.mark.parametrize("L", [8, 13, 20])  # fewer rows than, as many as, more than T + 1
def test_row_selection_and_clamp(L):
    T = 12
    track = np.stack([np.arange(L), -np.arange(L)], axis=1).astype(np.float32)  # row j is (j, -j)
    for offset in (0, 5, L + 3):
        rows = goal_rows(track, T, offset)
        assert rows.shape == (T, 2) and rows.dtype == np.float32
        want = [min(offset + t + 1, L - 1) for t in range(T)]
        np.testing.assert_array_equal(rows[:, 0], np.float32(want))
        np.testing.assert_array_equal(rows[:, 1], -np.float32(want))
    assert (goal_rows(track, T, L + 3) == track[-1]).all()  # past the last row the goal stays at its last place
    if L > T + 1:
        assert goal_rows(track, T, 0)[-1, 0] == T and goal_rows(track, T, 5)[-1, 0] == min(T + 5, L - 1)


def test_one_rollout_meets_the_goal_where_it_is():
    """One rollout along y = 0, 0.1 m per step.  The goal is 100 m away in every row but one, where it is 5 mm beside the
    path where step `there - 1 - offset` -- the step that sees that row -- ends: within the tolerance of 0.05 m of that state
    alone.  The cost chain freezes there -- and nowhere when that row lies in the past."""
    T, L, there = 12, 9, 6
    st = np.zeros((1, T + 1, 3), np.float32)
    st[0, :, 0] = np.float32(0.1) * np.arange(T + 1, dtype=np.float32)
    track = np.repeat(np.float32([[50.0, 100.0]]), L, axis=0)
    _, params, _, _, _, _ = _problem(T, 0, 1.0)
    params["goal_tolerance"] = 0.05
    p = oracle_params(params)
    for offset in range(there):  # row `there` is what step there - 1 - offset sees: put the goal where that step ends
        track[there] = st[0, there - offset, 0], np.float32(0.005)
        froze = freeze_step(p, goal_rows(track, T, offset), st)
        assert froze[0] == there - 1 - offset, (offset, froze)
    assert freeze_step(p, goal_rows(track, T, there), st)[0] == T  # (row `there` lies in the past)
    track[there] = st[0, there, 0], np.float32(0.005)
    # frozen: what comes after adds nothing -- the cost equals that of a horizon cut behind the freeze, control terms apart
    u, noise = np.zeros((T, 2), np.float32), np.zeros((1, T, 2), np.float32)
    counts = np.zeros((1, T), np.int64)
    full = chain(p, counts, st, noise, u, goal_rows(track, T, 0))
    cut = chain(p, counts[:, :there], st[:, :there + 1], noise[:, :there], u[:there], goal_rows(track, T, 0)[:there])
    assert _same_bits(full, cut)
    d2 = goal_d2(goal_rows(track, T, 0), st)
    want = np.float32(0)
    for t in range(there):
        want = np.float32(np.float64(want) + p.dist_weight * d2[0, t])
    assert full[0] == want  # (reached: no terminal term)


def test_moving_rows_change_the_costs():
    """A goal that crosses the fan of rollouts: the costs differ from the row-0 static goal's, and at offset 5 from offset 0's."""
    T = 37
    rng, params, pos, rad, u, noise = _problem(T, 3, 1.0)
    p = oracle_params(params)
    goal = np.float64(params["xgoal"])
    track = (goal[None] + np.arange(T + 6)[:, None] * np.array([-0.03, 0.02])).astype(np.float32)
    static = O.rollout_barebone(p, pos, rad, noise, u)
    at0 = goal_track_costs(p, track, noise, u, 0, pos[:, None], rad)
    at5 = goal_track_costs(p, track, noise, u, 5, pos[:, None], rad)
    assert (at0 != static).any() and (at5 != at0).any()
    one = goal_track_costs(p, track[:1], noise, u, 7, pos[:, None], rad)  # a track of one row: the static goal, any offset
    assert _same_bits(one, static)


def test_header_declares_and_binding_covers_set_goal_tracks():
    from mppi_numba_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mppi_hip.h")).read(), flags=re.S)
    found = re.search(r"\bint\s+mppi_planner_set_goal_tracks\s*\(([^)]*)\)", text)
    assert found, "include/mppi_hip.h does not declare mppi_planner_set_goal_tracks"
    assert len(found.group(1).split(",")) == 4
    assert len(_lib.SIGNATURES["mppi_planner_set_goal_tracks"]) == 4
    assert hasattr(_lib.load(), "mppi_planner_set_goal_tracks"), "libmppi_hip.so does not export mppi_planner_set_goal_tracks"


def test_a_constant_velocity_track_is_a_goal_track():
    from mppi_numba_amd.barebone import constant_velocity_tracks
    track = constant_velocity_tracks([[1.0, 2.0]], [[0.5, -0.25]], 0.1, 6)[0]
    assert track.shape == (6, 2) and track.dtype == np.float32
    np.testing.assert_array_equal(track[4], np.float32([1.0 + 0.5 * 0.4, 2.0 - 0.25 * 0.4]))
