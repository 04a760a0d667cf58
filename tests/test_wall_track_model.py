"""CPU checks of the wall tracks' model (tests/wall_track_model.py; the row selection of k_rollout_barebone_crowd's
CrowdWallTracks form) and of the two host helpers that make wall tracks, barebone.swept_walls and
barebone.constant_velocity_walls."""
import os
import re

import numpy as np
import pytest

from test_crowd_model import _problem
from track_model import oracle_params
from wall_model import hit, states, wall_hits_of_states
from wall_track_model import wall_track_costs, wall_track_hits_of_states

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def some_walls(rng, count, x0, goal):
    """Walls around the segment start -> goal, half-widths 0 .. 0.2."""
    s = rng.uniform(0.0, 1.0, (count, 1))
    a = x0[:2] * (1 - s) + goal * s + rng.normal(0, 0.5, (count, 2))
    seg = np.stack([a, a + rng.uniform(-1.0, 1.0, (count, 2))], axis=1).astype(np.float32)
    return seg, rng.uniform(0.0, 0.2, count).astype(np.float32)


@pytest.mark.parametrize("T,W,Lw", [(30, 5, 1), (37, 70, 12), (37, 70, 43)])
def test_equal_rows_are_static_walls(T, W, Lw):
    rng, params, _, _, u, noise = _problem(T, 0, 1.0)
    seg, hw = some_walls(rng, W, params["x0"], params["xgoal"])
    st = states(oracle_params(params), noise, u)
    want = wall_hits_of_states(st, seg, hw)
    assert want.any(), "bad input: no step hits a wall"
    tracks = np.repeat(seg[:, None], Lw, axis=1)
    for offset in (0, 5, Lw + 3):
        got = wall_track_hits_of_states(st, tracks, hw, offset)
        assert got.dtype == want.dtype and (got == want).all(), (T, W, Lw, offset)


def test_row_selection():
    """One rollout along y = 0, 0.1 m per step; one wall along the whole path, 5 mm beside it, that is THERE in one row only
    (every other row holds it 100 m away).  Step t sees row min(offset + t, Lw - 1): the one hit is at step row - offset."""
    T, Lw, there = 12, 9, 6
    st = np.zeros((1, T + 1, 3), np.float32)
    st[0, :, 0] = np.float32(0.1) * np.arange(T + 1, dtype=np.float32)
    near, far = np.float32([[-1.0, 0.005], [10.0, 0.005]]), np.float32([[-1.0, 100.0], [10.0, 100.0]])
    tracks = np.repeat(far[None, None], Lw, axis=1)
    tracks[0, there] = near
    assert wall_hits_of_states(st, near[None], 0.01).all() and not wall_hits_of_states(st, far[None], 0.01).any()
    for offset in range(there + 1):
        want = np.zeros((1, T), np.int64)
        want[0, there - offset] = 1
        assert (wall_track_hits_of_states(st, tracks, 0.01, offset) == want).all(), offset
    assert not wall_track_hits_of_states(st, tracks, 0.01, there + 1).any()  # (row `there` lies in the past)
    # the clamp: a wall that arrives in the LAST row stays -- every step from Lw - 1 - offset on, every step past the end
    tracks[0, there], tracks[0, Lw - 1] = far, near
    for offset in (0, 3, Lw - 1, Lw + 3):
        want = (np.arange(T) + offset >= Lw - 1).astype(np.int64)[None]
        assert (wall_track_hits_of_states(st, tracks, 0.01, offset) == want).all(), offset


def test_costs_are_the_chain_on_disc_hits_plus_wall_hits():
    """Disc rows are instants (row offset + t + 1), wall rows intervals (row offset + t); each clamps against its own count."""
    from crowd_model import hit_counts
    from mppi_numba_amd.barebone import constant_velocity_tracks, constant_velocity_walls
    from wall_model import chain
    T, K, W = 30, 5, 9
    rng, params, pos, rad, u, noise = _problem(T, K, 1.0)
    p = oracle_params(params)
    seg, hw = some_walls(rng, W, params["x0"], params["xgoal"])
    discs = constant_velocity_tracks(pos, rng.normal(0, 0.3, (K, 2)), 0.1, T + 1)
    walls = constant_velocity_walls(seg, rng.normal(0, 0.3, (W, 2)), 0.1, 12)
    for offset in (0, 4):
        disc_counts, st = hit_counts(p, discs, rad, noise, u, offset)
        wall_counts = wall_track_hits_of_states(st, walls, hw, offset)
        assert wall_counts.any() and (wall_counts != wall_hits_of_states(st, walls[:, 0], hw)).any()
        got = wall_track_costs(p, discs, rad, walls, hw, noise, u, offset)
        want = chain(p, disc_counts + wall_counts, st, noise, u)
        assert (got.view(np.int32) == want.view(np.int32)).all()


def disc_test(robot, centre, r):
    """crowd_model.hit_counts' test of one position against one disc: the float32 difference widened, not (d2 - r*r > 0)."""
    ex = (robot[..., 0] - centre[..., 0]).astype(np.float64)
    ey = (robot[..., 1] - centre[..., 1]).astype(np.float64)
    rr = np.float64(np.float32(r)) * np.float64(np.float32(r))
    return ~(ex * ex + ey * ey - rr > 0.0)


def test_swept_walls_are_conservative():
    """2 000 pairs of bodies, each moving linearly within every control interval, the sum of their radii r.  Whenever 64
    samples per interval find the two within r at the SAME instant, the model reports a hit in that interval: the segment
    the robot covers against the capsule the other sweeps.  A quarter of the pairs swap places head-on within one interval:
    the post-step test against the disc's row (an instant) misses some of those, which is the hole swept walls close."""
    from mppi_numba_amd.barebone import swept_walls
    rng = np.random.default_rng(31)
    pairs, L, r, m = 2000, 7, np.float32(0.3), 64
    robot = np.cumsum(rng.uniform(-0.5, 0.5, (pairs, L, 2)), axis=1)
    other = robot + rng.normal(0, 0.6, (pairs, L, 2))
    swap = np.arange(pairs) % 4 == 0  # interval 2: each ends where the other began, 0.5 .. 1 m apart
    bearing = rng.uniform(-np.pi, np.pi, pairs)
    apart = rng.uniform(0.5, 1.0, (pairs, 1)) * np.stack([np.cos(bearing), np.sin(bearing)], axis=1)
    other[swap, 2] = robot[swap, 2] + apart[swap]
    robot[swap, 3], other[swap, 3] = other[swap, 2], robot[swap, 2]
    robot, other = robot.astype(np.float32), other.astype(np.float32)
    walls = swept_walls(other)
    assert walls.shape == (pairs, L - 1, 2, 2) and walls.dtype == np.float32
    np.testing.assert_array_equal(walls[:, :, 0], other[:, :-1])
    np.testing.assert_array_equal(walls[:, :, 1], other[:, 1:])
    s = np.linspace(0.0, 1.0, m)[None, None, :, None]
    R, O_ = robot.astype(np.float64), other.astype(np.float64)
    gap = (R[:, :-1, None] + s * (R[:, 1:, None] - R[:, :-1, None])) - (O_[:, :-1, None] + s * (O_[:, 1:, None] - O_[:, :-1, None]))
    collide = np.sqrt((gap ** 2).sum(axis=3)).min(axis=2) <= np.float64(r)  # (pairs, L - 1): a true collision in the interval
    model = hit(robot[:, :-1], robot[:, 1:], walls[:, :, 0], walls[:, :, 1], r)
    # ... and through the track model's row selection, every pair a one-wall scene (the same verdicts)
    for i in range(0, pairs, 40):
        got = wall_track_hits_of_states(robot[i:i + 1], walls[i:i + 1], r, 0)
        assert (got[0] == model[i]).all(), i
    missed = collide[:, 2] & ~disc_test(robot[:, 2], other[:, 2], r) & ~disc_test(robot[:, 3], other[:, 3], r) & swap
    print("swept walls: %d of %d intervals collide, the model hits %d; %d head-on swaps the disc test misses"
          % (collide.sum(), collide.size, model.sum(), missed.sum()))
    assert missed.sum() >= 1, "bad input: no head-on swap that the post-step disc test misses"
    assert collide.sum() >= 500 and (~collide).sum() >= 500
    assert model[collide].all(), "%d true collisions are not hit" % (~model[collide]).sum()
    assert (model & ~collide).any() and not model.all()  # (conservative: some near misses are hit, not everything)


def test_swept_walls_shapes():
    from mppi_numba_amd.barebone import swept_walls
    one = swept_walls(np.float64([[[1.0, 2.0]], [[3.0, 0.1]]]))  # L = 1: the degenerate segment [c_0, c_0]
    assert one.shape == (2, 1, 2, 2) and one.dtype == np.float32 and one.flags["C_CONTIGUOUS"]
    np.testing.assert_array_equal(one[:, 0, 0], np.float32([[1.0, 2.0], [3.0, 0.1]]))
    np.testing.assert_array_equal(one[:, 0, 1], one[:, 0, 0])
    for L in (1, 2, 5):
        none = swept_walls(np.zeros((0, L, 2)))
        assert none.shape == (0, max(L - 1, 1), 2, 2) and none.dtype == np.float32
    two = swept_walls([[[0.0, 0.0], [1.0, 0.5]]])
    np.testing.assert_array_equal(two, np.float32([[[[0.0, 0.0], [1.0, 0.5]]]]))
    with pytest.raises(ValueError):
        swept_walls(np.zeros((3, 2)))


def test_constant_velocity_walls():
    from mppi_numba_amd.barebone import constant_velocity_walls
    rng = np.random.default_rng(5)
    W, rows, dt = 6, 9, 0.1
    seg, vel = rng.uniform(-3, 3, (W, 2, 2)), rng.uniform(-1, 1, (W, 2))
    for at in (0.5, 0.0, 1.0):
        got = constant_velocity_walls(seg, vel, dt, rows, at=at) if at != 0.5 else constant_velocity_walls(seg, vel, dt, rows)
        assert got.shape == (W, rows, 2, 2) and got.dtype == np.float32 and got.flags["C_CONTIGUOUS"]
        for j in range(rows):  # float64 throughout, rounded once
            want = (seg + vel[:, None, :] * ((np.float64(j) + at) * dt)).astype(np.float32)
            np.testing.assert_array_equal(got[:, j], want)
    np.testing.assert_array_equal(constant_velocity_walls(seg, vel, dt, rows, at=0)[:, 0], seg.astype(np.float32))
    assert constant_velocity_walls(np.zeros((0, 2, 2)), np.zeros((0, 2)), dt, 3).shape == (0, 3, 2, 2)


def test_header_declares_and_binding_covers_set_wall_tracks():
    from mppi_numba_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mppi_hip.h")).read(), flags=re.S)
    found = re.search(r"\bint\s+mppi_planner_set_wall_tracks\s*\(([^)]*)\)", text)
    assert found, "include/mppi_hip.h does not declare mppi_planner_set_wall_tracks"
    assert len(found.group(1).split(",")) == 6
    assert len(_lib.SIGNATURES["mppi_planner_set_wall_tracks"]) == 6
    assert hasattr(_lib.load(), "mppi_planner_set_wall_tracks"), "libmppi_hip.so does not export mppi_planner_set_wall_tracks"
