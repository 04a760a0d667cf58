"""CPU-only: the scenes of tests/occupancy_cases.py mean something on the model -- in every one of them between 5 % and 95 %
of the (rollout, step) pairs hit the grid, some pair is near at a ring without hitting, some test point lies outside the
grid and some rollout reaches the goal; and the grid changes the model's costs."""
import numpy as np
import pytest

import clearance_cases
import goal_track_model
import occupancy_cases as cases
import occupancy_model as om
from test_gpu_barebone_batch import oracle_params, problem_params


@pytest.mark.parametrize("name", cases.NAMES)
def test_a_single_scene_means_something(name):
    c = cases.single_case(name)
    rows = None if c["goal_track"] is None else goal_track_model.goal_rows(c["goal_track"], cases.T, c["offset"])
    share = cases.the_input_means_something(c["grid"], c["st"], c["rings"], c["footprint"], c["p"], rows)
    with_grid = cases.model_costs(c)
    empty = om.Grid((c["grid"].x_min, c["grid"].y_min), c["grid"].res, np.zeros_like(c["grid"].cells), c["grid"].inflate, c["grid"].substeps)
    without = cases.model_costs(c, empty)
    assert (with_grid >= without).all() and (with_grid != without).any(), "bad input: the grid costs nothing"
    print("%s: %.3f of the pairs hit, grid %d x %d" % (name, share, c["grid"].ny, c["grid"].nx))


def test_the_batch_means_something():
    c = cases.batch_case()
    reached = []
    for b in range(c["B"]):
        p = oracle_params(problem_params(c["params"], c["x0s"][b], c["goals"][b]))
        reached.append(cases.the_input_means_something(c["grid"], c["sts"][b], c["rings"], None, p, alone=False))
    assert any(reached), "bad input: no rollout of any problem reaches its goal"


def test_the_fleets_mean_something():
    disc = clearance_cases.disc_fleet_case()
    reached = []
    grid, _, ps, sts = cases.disc_fleet_scene()
    for b, st in enumerate(sts):
        reached.append(cases.the_input_means_something(grid, st, disc["rings"], None, ps[b], alone=False))
    assert any(reached), "bad input: no robot of the disc fleet reaches its goal"
    body = clearance_cases.body_fleet_case()
    reached = []
    grid, _, ps, sts = cases.body_fleet_scene()
    for a, st in enumerate(sts):
        reached.append(cases.the_input_means_something(grid, st, body["rings"], body["footprint"], ps[a], alone=False))
    assert any(reached), "bad input: no robot of the fleet of bodies reaches its goal"
