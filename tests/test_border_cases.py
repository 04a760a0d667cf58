"""The inputs of tests/test_gpu_border.py (tests/border_cases.py), held on the CPU to what makes them a test of the clamp.

For every (kind, start) a GPU case runs:
  (a) on the `nominal` world the numpy model of the time-parallel kernel (tests/scan_exact_model.py), which CLAMPS through
      scan_model._cell_index, is bit-equal to the oracle, which WRAPS on the low side: with the copy property the two
      read the same bytes, so the oracle is the clamp's reference;
  (b) a low start on the same world WITHOUT the copy property gives other oracle costs: the case discriminates;
  (c) flipping the obstacle bit of the outermost cells changes the oracle's cost of at least 90 % of the rollouts: the
      cases pay the border cells;
  (d) the analytic bound on the most negative index is at most R, the width of the copies.
"""
import numpy as np
import pytest

import border_cases as BC
from oracle import oracle as O
from scan_exact_model import scan_exact_rollout

N = 96


def oracle_params(w, params):
    return O.make_params(params, w["res"], w["xlimits"], w["ylimits"], np.asarray(BC.BOUNDS, dtype=np.float32),
                         np.asarray(BC.BOUNDS, dtype=np.float32))


def inputs(params, t_steps, seed=3):
    """Noise of the task's standard deviations, and controls that drive ahead at half the top speed."""
    rng = np.random.default_rng(seed)
    noise = (rng.standard_normal((N, t_steps, 2)) * np.asarray(params["u_std"])).astype(np.float32)
    u = np.tile(np.array([0.5 * params["vrange"][1], 0.1], dtype=np.float32), (t_steps, 1))
    return noise, u


def oracle_costs(w, params, noise, u, obstacle=None):
    return O.rollout_det(oracle_params(w, params), w["lin"], w["ang"], w["obstacle"] if obstacle is None else obstacle,
                         w["unknown"], noise, u)


PAIRS = sorted({(kind, name) for kind, names in BC.GPU_CASES.values() for name in names})
WORLDS = {}


def the_world(kind, copies=True):
    if (kind, copies) not in WORLDS:
        WORLDS[kind, copies] = BC.world(kind, copies=copies)
    return WORLDS[kind, copies]


def test_every_layer_has_the_copy_property_and_no_zero_traction():
    for kind in BC.KINDS:
        w = the_world(kind)
        for name in ("lin", "ang", "risk", "obstacle", "unknown", "lin_pmf", "ang_pmf", "risk_pmf"):
            assert BC.has_copy_property(w[name]), (kind, name)
        assert w["lin"].min() >= 42 and w["lin"].max() <= 100 and w["ang"].min() >= 42, kind
        assert w["lin"].shape == (1, BC.ROWS, BC.COLS) and w["obstacle"].shape == (BC.ROWS, BC.COLS)
        assert not BC.has_copy_property(the_world(kind, copies=False)["obstacle"])
    assert len(np.unique(the_world("nominal")["lin"])) == 1 and len(np.unique(the_world("nominal")["ang"])) == 1
    assert len(np.unique(the_world("cellwise")["lin"])) == 5 and not np.array_equal(the_world("cellwise")["lin"], the_world("cellwise")["ang"])


def test_the_starts_are_where_their_names_say():
    w = the_world("nominal")
    cells = BC.start_cells()
    for name, (cx, cy, th) in cells.items():
        x0, goal = BC.start(w, name)
        xi = int(np.floor(np.float32(np.float32(x0[0]) - np.float32(w["xlimits"][0])) / np.float32(w["res"])))
        yi = int(np.floor(np.float32(np.float32(x0[1]) - np.float32(w["ylimits"][0])) / np.float32(w["res"])))
        assert (xi, yi) == (cx, cy), name
        inside = 0 <= cx < BC.COLS and 0 <= cy < BC.ROWS
        assert inside == (not name.startswith(("out_", "far_"))), name
        if name.startswith("out_"):
            assert 1 <= max(-cx, -cy, cx - BC.COLS + 1, cy - BC.ROWS + 1) <= 5, name
        if name != "mid":  # heading outwards: the goal lies further from the map's centre
            centre = np.array([w["xlimits"][0] + 0.5 * BC.COLS * w["res"], w["ylimits"][0] + 0.5 * BC.ROWS * w["res"]])
            assert np.linalg.norm(goal - centre) > np.linalg.norm(x0[:2] - centre) + 3.0, name
    assert cells["far_hi"][0] - BC.COLS > BC.ROWS and cells["far_hi"][1] - BC.ROWS > BC.ROWS
    # the low starts: those that head for a low border
    assert {n for n, (_, _, th) in cells.items() if n != "mid" and min(np.cos(th), np.sin(th)) < -0.1} == set(BC.LOW_STARTS)
    assert {name for _, name in PAIRS} == set(cells)  # every named start runs on the GPU


@pytest.mark.parametrize("kind,name", PAIRS)
def test_conditions_on_the_inputs(kind, name):
    w = the_world(kind)
    params = BC.params(w, name)
    noise, u = inputs(params, BC.T_STEPS)
    want = oracle_costs(w, params, noise, u)
    assert np.isfinite(want).all()
    # (d)
    assert BC.negative_index_bound(w, name) <= BC.R, name
    if name == "mid":  # the control: no exits, nothing more to hold
        return
    # (a)
    if kind == "nominal":
        got, failed = scan_exact_rollout(oracle_params(w, params), w["lin"], w["ang"], w["obstacle"], w["unknown"], noise, u)
        assert not failed.any()
        assert np.array_equal(got, want), (name, int((got != want).sum()))
    # (b)
    if name in BC.LOW_STARTS:
        plain = the_world(kind, copies=False)
        assert (oracle_costs(plain, params, noise, u) != want).mean() >= 0.5, name
    # (c)
    flipped = oracle_costs(w, params, noise, u, obstacle=BC.flip_outermost_obstacles(w["obstacle"]))
    share = float((flipped != want).mean())
    assert share >= 0.9, (name, share)


def test_conditions_on_the_long_horizon_case():
    case = BC.PIPE_T105
    w = the_world(case["kind"])
    params = BC.params(w, case["start"], vrange=np.array([0.0, case["vmax"]]))
    noise, u = inputs(params, case["t_steps"])
    want = oracle_costs(w, params, noise, u)
    assert BC.negative_index_bound(w, case["start"], t_steps=case["t_steps"], vmax=case["vmax"]) <= BC.R
    flipped = oracle_costs(w, params, noise, u, obstacle=BC.flip_outermost_obstacles(w["obstacle"]))
    assert (flipped != want).mean() >= 0.9
