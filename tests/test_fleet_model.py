"""CPU checks of the fleet model (tests/fleet_model.py; mppi_planner_set_fleet): the order of a reader's walls and the
rounding of its half-widths, that the fleet rows are wall tracks read from "now" whatever the offset of the disc tracks is,
and that the C ABI's four entry points are declared and bound."""
import os
import re

import numpy as np
import pytest

import fleet_model
from crowd_model import hit_counts
from test_crowd_model import _problem
from track_model import oracle_params
from wall_model import chain, states
from wall_track_model import wall_track_costs, wall_track_hits_of_states

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and (a.view(np.int32) == b.view(np.int32)).all()


def three_robots(T, wscale=1.0):
    """Reader 0 is test_crowd_model's problem; robot 1 comes towards it along its diagonal, robot 2 crosses the diagonal
    from the side -- so that rollouts of robot 0 meet both plans in the middle of the horizon.  Some of robot 2's controls
    lie outside vrange / wrange: the clip takes part."""
    rng, params, _, _, u0, noise = _problem(T, 0, wscale)
    x0 = np.asarray(params["x0"], np.float64)
    along = np.array([np.cos(np.pi / 4), np.sin(np.pi / 4)])
    across = np.array([-along[1], along[0]])
    x0s = np.stack([x0,
                    np.concatenate([x0[:2] + 3.0 * along, [np.pi / 4 + np.pi]]),
                    np.concatenate([x0[:2] + 1.6 * along - 1.2 * across, [np.pi / 4 + np.pi / 2]])])
    us = np.stack([u0,
                   np.stack([np.full(T, 1.0), rng.uniform(-0.1, 0.1, T)], 1),
                   np.stack([rng.uniform(0.6, 2.6, T), rng.uniform(-4.0, 4.0, T) * 0.05], 1)]).astype(np.float32)
    us[2, 3, 1], us[2, 4, 0] = 40.0, -1.0
    return rng, params, x0s, us, noise


def test_skip_self_order_and_halfwidth_rounding():
    from mppi_numba_amd.barebone import fleet_others, swept_walls
    want = np.array([[1, 2], [0, 2], [0, 1]])
    np.testing.assert_array_equal(fleet_model.others(3), want)
    np.testing.assert_array_equal(fleet_others(3), want)
    np.testing.assert_array_equal(fleet_others(66), fleet_model.others(66))
    assert fleet_others(2).tolist() == [[1], [0]]
    radii, margin = np.array([0.1, 0.2, 0.3]), 0.05
    hw = fleet_model.halfwidths(radii, margin, 3)
    assert hw.dtype == np.float32 and hw.shape == (3, 2)
    r32 = radii.astype(np.float32)
    one_rounding, two_roundings = np.empty((3, 2), np.float32), np.empty((3, 2), np.float32)
    for a in range(3):
        for k, b in enumerate(want[a]):
            one_rounding[a, k] = np.float32(np.float64(r32[a]) + np.float64(r32[b]) + np.float64(margin))
            two_roundings[a, k] = np.float32(np.float32(r32[a] + r32[b]) + np.float32(margin))
    assert same_bits(hw, one_rounding)
    assert (one_rounding != two_roundings).any(), "bad input: summing in float32 gives the same half-widths"
    for a in range(3):
        for k, b in enumerate(want[a]):
            assert hw[a, k] == hw[b, list(want[b]).index(a)]
    assert same_bits(fleet_model.halfwidths(0.25, 0.0, 3), np.full((3, 2), 0.5, np.float32))
    # the walls: swept_walls of the others' plans, the plans the oracle's own state rollouts with zero noise
    T = 12
    _, params, x0s, us, _ = three_robots(T)
    st = fleet_model.plans(params, x0s, us)
    walls = fleet_model.fleet_walls(params, x0s, us)
    assert walls.shape == (3, 2, T, 2, 2) and walls.dtype == np.float32
    for b in range(3):
        p = oracle_params(dict(params, x0=x0s[b]))
        assert same_bits(st[b], states(p, np.zeros((1, T, 2), np.float32), us[b])[0])
        unclipped = states(oracle_params(dict(params, x0=x0s[b], vrange=np.array([-1e3, 1e3]), wrange=np.array([-1e3, 1e3]))),
                           np.zeros((1, T, 2), np.float32), us[b])[0]
        assert (b == 2) == (not same_bits(st[b], unclipped)), "robot 2's plan, and only its, shows the clip"
    for a in range(3):
        for k, b in enumerate(want[a]):
            assert same_bits(walls[a, k], swept_walls(st[b][None, :, :2])[0])
            assert same_bits(walls[a, k, :, 0], st[b, :-1, :2]) and same_bits(walls[a, k, :, 1], st[b, 1:, :2])
    parked = fleet_model.fleet_walls(params, x0s, us, parked=np.array([False, True, False]))
    assert same_bits(parked[0, 0], np.broadcast_to(x0s[1, :2].astype(np.float32), (T, 2, 2)).copy())
    assert same_bits(parked[0, 1], walls[0, 1]) and same_bits(parked[1], walls[1])


@pytest.mark.parametrize("T,W", [(30, 0), (37, 3)])
def test_fleet_rows_are_wall_tracks_read_from_now(T, W):
    """Disc offset 0: the costs are wall_track_costs on the same walls.  Disc tracks at offset 5: the disc rows move on,
    the fleet rows do not -- the costs differ from wall_track_costs(..., offset=5) and equal the chain on disc hits at 5
    plus wall hits at 0."""
    from mppi_numba_amd.barebone import constant_velocity_tracks
    rng, params, x0s, us, noise = three_robots(T)
    p = oracle_params(params)
    walls = fleet_model.fleet_walls(params, x0s, us)
    hw = fleet_model.halfwidths([0.25, 0.3, 0.2], 0.05, 3)
    room = np.float32([[[-3, -3], [9, -3]], [[9, -3], [9, 9]], [[0.5, 2.5], [2.5, 0.5]]])[:W]
    wt, h = fleet_model.reader_walls(walls[0], hw[0], room, np.float32([0.05, 0.05, 0.1])[:W])
    assert wt.shape == (2 + W, T, 2, 2) and h.shape == (2 + W,)
    K = 5
    disc_pos = (x0s[0, :2] + rng.uniform(0.5, 3.5, (K, 2))).astype(np.float32)
    discs = constant_velocity_tracks(disc_pos, rng.normal(0, 0.4, (K, 2)), 0.1, T + 6)
    rad = rng.uniform(0.2, 0.5, K).astype(np.float32)
    counts0, st = hit_counts(p, discs, rad, noise, us[0], 0)
    counts5, _ = hit_counts(p, discs, rad, noise, us[0], 5)
    fleet = fleet_model.fleet_hits(st, wt, h)
    assert fleet[:, :].any() and wall_track_hits_of_states(st, wt[:2], h[:2], 0).any(), "bad input: no step hits a fleet wall"
    assert (counts0 != counts5).any(), "bad input: the disc offset shows nowhere"
    assert (fleet != wall_track_hits_of_states(st, wt, h, 5)).any(), "bad input: the walls read at offset 5 hit the same steps"
    at0 = fleet_model.fleet_costs(p, wt, h, noise, us[0], discs, rad, offset=0)
    assert same_bits(at0, wall_track_costs(p, discs, rad, wt, h, noise, us[0], 0))
    at5 = fleet_model.fleet_costs(p, wt, h, noise, us[0], discs, rad, offset=5)
    assert same_bits(at5, chain(p, counts5 + fleet, st, noise, us[0]))
    assert not same_bits(at5, wall_track_costs(p, discs, rad, wt, h, noise, us[0], 5)), "the fleet rows followed the offset"
    assert not same_bits(at5, at0)
    without = fleet_model.fleet_costs(p, wt[2:], h[2:], noise, us[0], discs, rad, offset=5)
    assert not same_bits(at5, without), "bad input: the fleet changes no cost"


def test_header_declares_and_binding_covers_the_fleet_entry_points():
    from mppi_numba_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mppi_hip.h")).read(), flags=re.S)
    for name, args in (("mppi_planner_set_fleet", 3), ("mppi_planner_get_fleet", 2), ("mppi_planner_fleet_refresh", 1),
                       ("mppi_planner_get_fleet_walls", 2)):
        found = re.search(r"\bint\s+%s\s*\(([^)]*)\)" % name, text)
        assert found, "include/mppi_hip.h does not declare %s" % name
        assert len(found.group(1).split(",")) == args
        assert len(_lib.SIGNATURES[name]) == args
        assert hasattr(_lib.load(), name), "libmppi_hip.so does not export %s" % name
