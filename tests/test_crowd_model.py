"""CPU proof of the algebra behind the barebone planner's crowd mode: counting the discs a step's position touches and then
adding obs_cost once per hit (tests/crowd_model.py, the order of k_rollout_barebone_crowd) gives the bits of one rounded
addition per disc, hit or not (tests/track_model.py, the order of k_rollout_barebone) -- and so, on tracks that do not
move, the bits of oracle.rollout_barebone.  Plus the C ABI's new entry points: declared and bound."""
import os
import re

import numpy as np
import pytest

from crowd_model import crowd_costs, crowd_discs, hit_counts
from oracle import oracle as O
from track_model import oracle_params, reached_goal, track_costs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OBS_PENALTY = 1e6
N = 128
CASES = [(T, K, wscale) for T in (30, 37) for K in (0, 1, 5, 70) for wscale in (1.0, 2.0)]


def _problem(T, K, wscale, dt=0.1):
    """wscale 1.0: the heading increments the GPU takes by rotation; 2.0: full sincos.  T = 37: the goal within reach."""
    rng = np.random.default_rng(1000 * T + 10 * K + int(wscale))
    x0 = np.array([rng.uniform(-1, 1), rng.uniform(-1, 1), np.pi / 4 + rng.uniform(-0.3, 0.3)])
    goal = x0[:2] + (np.array([1.6, 1.6]) if T == 37 else rng.uniform(3, 6, 2))
    params = dict(dt=dt, x0=x0, xgoal=goal, goal_tolerance=0.5, dist_weight=10, lambda_weight=1.0, num_opt=1,
                  u_std=np.array([1.0, 1.0]), vrange=np.array([0.0, 2.0]), wrange=np.array([-np.pi, np.pi]) * wscale,
                  obs_penalty=OBS_PENALTY)
    pos, rad = crowd_discs(rng, K, x0, goal)
    u = np.stack([rng.uniform(0.8, 1.8, T), rng.uniform(-0.2, 0.2, T)], 1).astype(np.float32)
    noise = rng.normal(0, 0.5, (N, T, 2)).astype(np.float32)
    return rng, params, pos, rad, u, noise


def _same_bits(a, b):
    return (a.view(np.int32) == b.view(np.int32)).all()


@pytest.fixture(scope="module")
def seen():
    """What the cases have shown between them (checked by the last test of the module)."""
    return dict(multi=0, above=0, reached=0.0, cases=0)


@pytest.mark.parametrize("T,K,wscale", CASES)
def test_crowd_model_equals_the_track_model(T, K, wscale, seen):
    from mppi_numba_amd.barebone import constant_velocity_tracks
    rng, params, pos, rad, u, noise = _problem(T, K, wscale)
    p = oracle_params(params)
    L = T + 1
    tracks = constant_velocity_tracks(pos, rng.normal(0, 0.3, (K, 2)), 0.1, L)
    for offset in (0, 7, L + 4):
        want = track_costs(p, tracks, rad, noise, u, offset=offset)
        got = crowd_costs(p, tracks, rad, noise, u, offset=offset)
        assert _same_bits(got, want), "T %d, K %d, offset %d: %d of %d costs differ" % (T, K, offset, (got != want).sum(), N)
    counts, _ = hit_counts(p, tracks, rad, noise, u)
    assert counts.max() <= K
    got = crowd_costs(p, tracks, rad, noise, u)
    seen["cases"] += 1
    seen["multi"] += int((counts >= 2).sum())
    seen["above"] += int((got > OBS_PENALTY).sum())
    seen["reached"] = max(seen["reached"], float(reached_goal(p, noise[:, :T - 1], u[:T - 1]).mean()))
    if K >= 5:  # the discs laid on top of each other on the straight line: a bad input otherwise, not a pass
        assert (counts >= 2).any(), "bad input: no (rollout, step) pair is inside two discs"
        assert (got > OBS_PENALTY).any(), "bad input: no rollout costs more than obs_penalty"
    if T == 37:
        early = reached_goal(p, noise[:, :T - 1], u[:T - 1])  # (within the goal tolerance BEFORE the last step)
        assert early.mean() >= 0.10, "bad input: only %.1f %% of the rollouts reach the goal early" % (100 * early.mean())


@pytest.mark.parametrize("T,K,wscale", CASES)
def test_crowd_model_equals_the_oracle_on_constant_tracks(T, K, wscale):
    _, params, pos, rad, u, noise = _problem(T, K, wscale)
    p = oracle_params(params)
    ref = O.rollout_barebone(p, pos, rad, noise, u)
    for L, offset in ((1, 0), (T + 1, 0), (T + 1, 7)):
        got = crowd_costs(p, np.repeat(pos[:, None, :], L, axis=1), rad, noise, u, offset=offset)
        assert _same_bits(got, ref), "T %d, K %d, L %d: %d of %d costs differ" % (T, K, L, (got != ref).sum(), N)


def test_the_cases_mean_something(seen):
    assert seen["cases"] == len(CASES)
    assert seen["multi"] > 0 and seen["above"] > 0 and seen["reached"] >= 0.10, seen


def test_header_declares_and_binding_covers_the_crowd_entry_points():
    from mppi_numba_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mppi_hip.h")).read(), flags=re.S)
    for name in ("mppi_planner_set_crowd", "mppi_planner_get_crowd"):
        found = re.search(r"\bint\s+%s\s*\(([^)]*)\)" % name, text)
        assert found, "include/mppi_hip.h does not declare %s" % name
        assert len(found.group(1).split(",")) == 2, name
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name]) == 2, name
        assert hasattr(_lib.load(), name), "libmppi_hip.so does not export %s" % name


def test_config_keyword():
    from mppi_numba_amd.barebone import Config
    assert Config(T=1.0, dt=0.1).crowd is False
    assert Config(T=1.0, dt=0.1, crowd=True).crowd is True
