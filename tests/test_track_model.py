"""CPU checks of the moving-disc feature: the numpy cost model the GPU tests compare against (tests/track_model.py) equals
the oracle bit for bit where the oracle has an answer (tracks that do not move), the host-side track helper, and the
C ABI's new entry points are declared and bound."""
import os
import re

import numpy as np

from oracle import oracle as O
from track_model import oracle_params, reached_goal, track_costs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _problem(seed, n=1024, T=50, dt=0.1):
    rng = np.random.default_rng(seed)
    K = int(rng.integers(0, 6))
    x0 = np.array([rng.uniform(-1, 1), rng.uniform(-1, 1), rng.uniform(-np.pi, np.pi)])
    goal = x0[:2] + (rng.uniform(1, 6, 2) if seed % 3 else 0.8)  # every third goal within reach of the horizon
    params = dict(dt=dt, x0=x0, xgoal=goal, goal_tolerance=0.5, dist_weight=10, lambda_weight=1.0, num_opt=1,
                  u_std=np.array([1.0, 1.0]), vrange=np.array([0.0, 2.0]),
                  wrange=np.array([-np.pi, np.pi]) * (1 + seed % 2), obs_penalty=1e6)
    s = rng.uniform(0, 1, (K, 1))
    pos = (x0[:2] * (1 - s) + goal * s + rng.normal(0, 0.5, (K, 2))).astype(np.float32)
    rad = rng.uniform(0.2, 0.8, K).astype(np.float32)
    u = np.stack([rng.uniform(0.2, 1.8, T), rng.uniform(-1, 1, T)], 1).astype(np.float32)
    noise = rng.normal(0, 1, (n, T, 2)).astype(np.float32)
    return rng, params, pos, rad, u, noise


def test_model_equals_the_oracle_on_tracks_that_do_not_move():
    T, dt = 50, 0.1
    some_reached = moved = 0
    for seed in range(12):
        rng, params, pos, rad, u, noise = _problem(seed, T=T, dt=dt)
        p = oracle_params(params)
        ref = O.rollout_barebone(p, pos, rad, noise, u)
        L = 1 if seed % 2 else T + 1
        tracks = np.repeat(pos[:, None, :], L, axis=1)
        got = track_costs(p, tracks, rad, noise, u)
        differ = int((got.view(np.int32) != ref.view(np.int32)).sum())
        assert differ == 0, "problem %d (K = %d, L = %d): %d of %d costs differ" % (seed, len(rad), L, differ, len(ref))
        # any offset on tracks that do not move changes nothing
        assert (track_costs(p, tracks, rad, noise, u, offset=7).view(np.int32) == ref.view(np.int32)).all()
        if seed % 3 == 0:
            some_reached += int(reached_goal(p, noise, u).sum())
        if len(rad):
            from mppi_numba_amd.barebone import constant_velocity_tracks
            tr = constant_velocity_tracks(pos, rng.normal(0, 0.6, (len(rad), 2)), dt, T + 1)
            moved += int((track_costs(p, tr, rad, noise, u) != ref).sum())
    assert some_reached > 0, "no rollout of the problems with a near goal reached it: the freeze is not exercised"
    assert moved > 0, "moving the discs changed no cost: the model ignores the rows"


def test_model_offset_equals_sliced_tracks():
    from mppi_numba_amd.barebone import constant_velocity_tracks
    rng, params, pos, rad, u, noise = _problem(4, n=256, T=30)
    p = oracle_params(params)
    tr = constant_velocity_tracks(pos, rng.normal(0, 0.6, (len(rad), 2)), 0.1, 31)
    for s in (3, 17):
        a, b = track_costs(p, tr, rad, noise, u, offset=s), track_costs(p, tr[:, s:], rad, noise, u)
        assert (a.view(np.int32) == b.view(np.int32)).all()
    last = O.rollout_barebone(p, tr[:, -1], rad, noise, u)
    for s in (30, 38):
        assert (track_costs(p, tr, rad, noise, u, offset=s).view(np.int32) == last.view(np.int32)).all()


def test_constant_velocity_tracks():
    from mppi_numba_amd.barebone import constant_velocity_tracks
    pos = np.array([[1.0, 2.0], [0.1, -0.3], [5.0, 4.5]])
    vel = np.array([[0.5, -0.25], [0.0, 0.0], [-0.6, 0.3]])
    tr = constant_velocity_tracks(pos, vel, 0.1, 51)
    assert tr.shape == (3, 51, 2) and tr.dtype == np.float32 and tr.flags["C_CONTIGUOUS"]
    assert (tr[:, 0] == pos.astype(np.float32)).all()
    assert (tr[1] == np.float32([0.1, -0.3])).all()  # a disc that stands still: every row the float32 of its position
    # one value by hand: disc 0 after 20 rows = 2.0 s: (1 + 0.5 * 2, 2 - 0.25 * 2) = (2, 1.5), exact in float32
    assert tr[0, 20, 0] == np.float32(2.0) and tr[0, 20, 1] == np.float32(1.5)
    # evaluated in float64, rounded once: 5.0 - 0.6 * (7 * 0.1)
    assert tr[2, 7, 0] == np.float32(5.0 + (-0.6) * (7 * 0.1))
    assert constant_velocity_tracks(pos[:1], vel[:1], 0.1, 1).shape == (1, 1, 2)
    assert constant_velocity_tracks(np.zeros((0, 2)), np.zeros((0, 2)), 0.1, 4).shape == (0, 4, 2)


def test_header_declares_and_binding_covers_the_track_entry_points():
    from mppi_numba_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mppi_hip.h")).read(), flags=re.S)
    for name, n_args in (("mppi_planner_set_disc_tracks", 6), ("mppi_planner_set_track_offsets", 3),
                         ("mppi_planner_get_track_offsets", 3)):
        found = re.search(r"\bint\s+%s\s*\(([^)]*)\)" % name, text)
        assert found, "include/mppi_hip.h does not declare %s" % name
        assert len(found.group(1).split(",")) == n_args, name
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name]) == n_args, name
        assert hasattr(_lib.load(), name), "libmppi_hip.so does not export %s" % name
