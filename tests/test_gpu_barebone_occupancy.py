"""Occupancy-grid obstacles for the barebone planner in crowd mode (params['occupancy'], mppi_planner_set_occupancy): a
costmap as one more counted obstacle.  k_occupancy_field builds the clearance field, the grid forms of
k_rollout_barebone_crowd look it up behind a step's last wall tile, k_guide_field blocks the guide's cells with it.  Every
comparison is bit for bit -- with tests/occupancy_model.py on the scenes of tests/occupancy_cases.py
(tests/test_occupancy_cases.py shows on the CPU that they mean something), and handle against handle.  The model's states are
the exact ones, so the comparisons with it run in exact math; in fast math the statements are relations between handles."""
import ctypes as C
import gc

import numpy as np
import pytest

import clearance_cases
import guide_model
import occupancy_cases as cases
import occupancy_model as om
from clearance_cases import NO_DISCS, ring_params
from occupancy_cases import T, occupancy_params
from test_gpu_barebone_batch import ERR_INVALID, assert_bits, make_params, oracle_params, problem_params, problems
from test_gpu_barebone_crowd import cfg_of, shape_of
from test_gpu_barebone_disc_samples import sample_params, sample_set
from test_gpu_barebone_fleet import ROOM, ROOM_HW, fleet_ending
from test_gpu_barebone_guide import five_walls, guide_of
from test_gpu_barebone_tracks import rollout_with
from test_gpu_barebone_walls import wall_params

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def release_the_handles():
    """A planner and its device-array views refer to each other, so a handle lives until the cycle collector runs."""
    yield
    gc.collect()


def grid_params(params, origin, res, cells, inflate=0.0, substeps=1):
    return dict(params, occupancy=dict(origin=origin, resolution=res, cells=cells, inflate=inflate, substeps=substeps))


def tail_of(grid, F=0, R=0):
    return (" footprint=%d" % F if F else "") + (" rings=%d" % R if R else "") + " grid=%dx%d" % (grid.nx, grid.ny)


# ---- 1. the field --------------------------------------------------------------------------------------------------------
def field_cells():
    rng = np.random.default_rng(3)
    out = [("1x1", np.ones((1, 1), np.uint8)), ("1x1 free", np.zeros((1, 1), np.uint8)), ("1x70", rng.uniform(size=(1, 70)) < 0.1),
           ("65x3", rng.uniform(size=(65, 3)) < 0.2), ("64x64", rng.uniform(size=(64, 64)) < 0.01), ("70x129", rng.uniform(size=(70, 129)) < 0.05),
           ("empty", np.zeros((37, 70), bool)), ("full", np.ones((20, 67), np.int32) * 9)]
    corner = np.zeros((70, 129), np.int64)
    corner[-1, -1] = -1  # (any non-zero value of any integer dtype)
    out.append(("corner", corner))
    big = np.zeros((512, 512), bool)
    big[rng.integers(0, 512, 40), rng.integers(0, 512, 40)] = True
    big[0, 511] = big[511, 0] = True
    out.append(("512x512", big))
    return out


FIELDS = field_cells()


@pytest.mark.parametrize("name", [name for name, _ in FIELDS])
def test_the_field_equals_the_model(name):
    from mppi_numba_amd.barebone import MPPI_Numba
    cells = dict(FIELDS)[name]
    planner = MPPI_Numba(cfg_of(70, T, True))
    planner.setup(grid_params(make_params(0.1, 1.0), (0.0, 0.0), 0.1, cells))
    got = planner.occupancy_field()
    want = om.field_of(cells)
    assert got.shape == want.shape and got.dtype == np.uint32
    assert (got == want).all(), "%s: %d of %d cells differ" % (name, (got != want).sum(), want.size)
    assert planner.occupancy_fields_built == 1
    planner.occupancy_field()
    assert planner.occupancy_fields_built == 1, "unchanged cells build no field"
    if name == "70x129":  # new cells of the same shape: one more build, into the same arrays
        other = np.roll(np.asarray(cells), 7, axis=1)
        planner.params["occupancy"]["cells"] = other
        assert (planner.occupancy_field() == om.field_of(other)).all() and planner.occupancy_fields_built == 2


# ---- 2. costs against the model ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", cases.NAMES)
def test_costs_equal_the_model(name):
    from mppi_numba_amd.barebone import MPPI_Numba
    c = cases.single_case(name)
    planner = MPPI_Numba(cfg_of(c["n"], T, True))
    planner.set_params(occupancy_params(c["params"], c["grid"]))
    planner.move_mppi_task_vars_to_device()  # (hands the tracks over: offset 0)
    planner.set_track_offset(c["offset"])
    got, _, _, kernel = rollout_with(planner, c["u_in"], c["noise"])
    chunk = shape_of(kernel)[1]
    assert T > chunk and kernel.startswith("k_rollout_barebone_crowd exact=1"), kernel
    assert kernel.endswith(tail_of(c["grid"], c["F"], c["R"])), kernel
    assert ("rotation=1" in kernel) == (c["wscale"] == 1.0), kernel
    assert (" walls=%d" % c["W"] in kernel) == (c["W"] > 0), kernel
    assert ("goal_rows" in kernel) == (c["goal_track"] is not None), kernel
    assert (planner.occupancy_field() == c["grid"].field).all()
    assert_bits(got, cases.model_costs(c), "%s vs the model" % name)


def test_batch_with_per_problem_discs_and_walls():
    """B = 3 problems of n = 128, each with its own disc set and wall set, one ring set, one grid: problem b equals a single
    planner bit for bit, and the model."""
    from mppi_numba_amd.barebone import MPPI_Batch, MPPI_Numba
    case = cases.batch_case()
    B, n, rings, grid = case["B"], case["n"], case["rings"], case["grid"]
    full = occupancy_params(ring_params(case["params"], rings), grid)
    batch = MPPI_Batch(cfg_of(n, T, True), B)
    batch.setup(full, case["x0s"], case["goals"], obstacle_sets=case["sets"], wall_sets=case["wall_sets"])
    costs, u_out, _, kernel = rollout_with(batch, case["u_in"], case["noise"].reshape(B * n, T, 2))
    shape_of(kernel)
    assert "problems=%d" % B in kernel and kernel.endswith(tail_of(grid, 0, len(rings))), kernel
    single = MPPI_Numba(cfg_of(n, T, True))
    for b in range(B):
        pb = problem_params(case["params"], case["x0s"][b], case["goals"][b], case["sets"][b])
        seg, hw = case["wall_sets"][b]
        single.set_params(occupancy_params(ring_params(wall_params(pb, seg, hw) if len(hw) else pb, rings), grid))
        want, want_u, _, single_kernel = rollout_with(single, case["u_in"][b], case["noise"][b])
        assert single_kernel.endswith(tail_of(grid, 0, len(rings))) and "problems" not in single_kernel, single_kernel
        what = "problem %d (%d discs, %d walls)" % (b, case["counts"][b], case["wcounts"][b])
        assert_bits(costs[b], want, what + " vs a single handle")
        assert_bits(u_out[b], want_u, what + ": u vs a single handle")
        model = om.costs(oracle_params(pb), grid, rings, case["sets"][b][0][:, None, :], case["sets"][b][1], seg if len(hw) else None, hw,
                         case["noise"][b], case["u_in"][b])
        assert_bits(costs[b], model, what + " vs the model")


def test_the_disc_fleet_with_a_grid():
    """In a disc fleet the body is the point: the fleet's walls as ever, the grid one more obstacle."""
    from mppi_numba_amd.barebone import MPPI_Batch
    case = clearance_cases.disc_fleet_case()
    grid, goals, ps, _ = cases.disc_fleet_scene()
    B, n, t, W, rings = case["B"], case["n"], case["t"], case["W"], case["rings"]
    batch = MPPI_Batch(cfg_of(n, t, True), B)
    batch.setup(occupancy_params(ring_params(wall_params(case["params"], ROOM[:W], ROOM_HW[:W]), rings), grid), case["x0s"], goals)
    batch.set_fleet(np.asarray(clearance_cases.FLEET_RADII), clearance_cases.FLEET_MARGIN)
    costs, _, _, kernel = rollout_with(batch, case["us"], case["noise"].reshape(B * n, t, 2))
    shape_of(kernel)
    assert kernel.endswith(fleet_ending(B, W, t) + tail_of(grid, 0, len(rings))) and "problems=%d" % B in kernel, kernel
    for b in range(B):
        _, wt, h = case["readers"][b]
        model = om.costs(ps[b], grid, rings, *NO_DISCS, wt, h, case["noise"][b], case["us"][b], wall_offset=0)
        assert_bits(costs[b], model, "robot %d of the disc fleet vs the model" % b)


def test_the_fleet_of_bodies_with_a_grid():
    """In a fleet of bodies the body is the fleet's."""
    from mppi_numba_amd.barebone import MPPI_Batch
    case = clearance_cases.body_fleet_case()
    grid, goals, ps, _ = cases.body_fleet_scene()
    B, n, t, W, F, rings = case["B"], case["n"], case["t"], case["W"], case["F"], case["rings"]
    batch = MPPI_Batch(cfg_of(n, t, True), B)
    batch.setup(occupancy_params(ring_params(wall_params(case["params"], ROOM[:W], ROOM_HW[:W]), rings), grid), case["x0s"], goals)
    batch.set_fleet_bodies(case["footprint"], case["margin"])
    costs, _, _, kernel = rollout_with(batch, case["us"], case["noise"].reshape(B * n, t, 2))
    shape_of(kernel)
    assert " walls=%d wall_rows=%d fleet=%d" % (case["grouped"] + W, t, B) in kernel, kernel
    assert kernel.endswith(tail_of(grid, F, len(rings))), kernel
    for a in range(B):
        _, seg, hw = case["readers"][a]
        model = om.costs(ps[a], grid, rings, *NO_DISCS, seg, hw, case["noise"][a], case["us"][a], case["footprint"], wall_offset=0,
                         group=case["group"], grouped=case["grouped"])
        assert_bits(costs[a], model, "robot %d of the fleet of bodies vs the model" % a)


# ---- 3. an empty grid is no grid; 4. fast math ---------------------------------------------------------------------------
@pytest.mark.parametrize("math", ["exact", "fast"])
@pytest.mark.parametrize("name", ["point", "point-discs-walls-M3", "point-R2-tracks+5", "F3-R2-M3-wall-tracks+5"])
def test_an_empty_grid_is_no_grid_and_a_grid_only_adds(math, name):
    """All cells 0: the costs of the same launch without the key, bit for bit, in either math -- which holds "a point robot
    is the one-disc body (0, 0, 0)" to the bits of the plain forms.  With the scene's cells: no cost falls, some rise."""
    from mppi_numba_amd.barebone import MPPI_Numba
    c = cases.single_case(name)
    grid = c["grid"]
    planner = MPPI_Numba(cfg_of(c["n"], T, True, math))

    def run(params):
        planner.set_params(params)
        planner.move_mppi_task_vars_to_device()
        planner.set_track_offset(c["offset"])
        return rollout_with(planner, c["u_in"], c["noise"])

    plain, plain_u, _, plain_kernel = run(c["params"])
    assert "grid" not in plain_kernel, plain_kernel
    empty = om.Grid((grid.x_min, grid.y_min), grid.res, np.zeros_like(grid.cells), grid.inflate, grid.substeps)
    held, held_u, _, kernel = run(occupancy_params(c["params"], empty))
    assert kernel.endswith(tail_of(grid, c["F"], c["R"])) and ("exact=%d" % (math == "exact")) in kernel, kernel
    assert (planner.occupancy_field() == om.FAR).all()
    assert_bits(held, plain, "%s math, %s: an empty grid vs no grid" % (math, name))
    assert_bits(held_u, plain_u, "... and the update")
    paid, _, _, kernel = run(occupancy_params(c["params"], grid))
    assert kernel.endswith(tail_of(grid, c["F"], c["R"])), kernel
    assert (paid >= plain).all() and (paid != plain).any(), "%s math, %s: the grid's cells cost nothing, or make a rollout cheaper" % (math, name)
    if math == "exact":
        assert_bits(paid, cases.model_costs(c), "... and the model")
    after, after_u, _, after_kernel = run(c["params"])  # the key has gone
    assert after_kernel == plain_kernel, (plain_kernel, after_kernel)
    assert_bits(after, plain, "the key has gone: the costs of before")
    assert_bits(after_u, plain_u, "... and the update")
    with pytest.raises(ValueError):
        planner.occupancy_field()


# ---- 5. refusals ---------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_handle_as_it_was():
    from mppi_numba_amd import _lib
    from mppi_numba_amd.barebone import MPPI_Numba
    lib = _lib.load()
    n = 128
    params = make_params(0.1, 1.0)
    cells = np.zeros((20, 30), np.uint8)
    cells[5:9, 10:20] = 1
    held = grid_params(params, (0.0, 0.0), 0.1, cells, 0.1, 2)
    good = dict(x_min=0.0, y_min=0.0, res=0.1, nx=30, ny=20, inflate=0.1, substeps=2)

    def raw(handle, grid_cells=cells, **changes):
        a = dict(good, **changes)
        data = np.ascontiguousarray(grid_cells, np.uint8)
        return lib.mppi_planner_set_occupancy(handle, 1, a["x_min"], a["y_min"], a["res"], a["nx"], a["ny"], a["inflate"], a["substeps"],
                                              _lib.ptr(data, C.c_ubyte))

    def refused(planner, p, word, error=_lib.MppiError):
        planner.set_params(p)
        with pytest.raises(error) as err:
            planner.solve()
        if error is _lib.MppiError:
            assert err.value.code == ERR_INVALID
        assert word in str(err.value), str(err.value)

    planner = MPPI_Numba(cfg_of(n, T, False))
    planner.setup(params)
    assert np.isfinite(planner.solve()).all()
    plain = planner.last_rollout_kernel()
    refused(planner, held, "crowd")  # no crowd mode: no grid
    assert raw(planner._handle) == ERR_INVALID and "crowd" in lib.mppi_last_error().decode()
    planner.set_params(params)
    assert np.isfinite(planner.solve()).all() and planner.last_rollout_kernel() == plain
    planner.set_crowd(True)
    planner.set_params(held)
    assert np.isfinite(planner.solve()).all()
    kernel = planner.last_rollout_kernel()
    assert kernel.startswith("k_rollout_barebone_crowd") and kernel.endswith(" grid=30x20"), kernel
    field = planner.occupancy_field()

    def still_held():
        planner.set_params(held)
        assert np.isfinite(planner.solve()).all() and planner.last_rollout_kernel() == kernel
        assert (planner.occupancy_field() == field).all() and planner.occupancy_fields_built == 1

    bad = [(dict(x_min=np.nan), "finite"), (dict(res=np.inf), "finite"), (dict(inflate=np.nan), "finite"), (dict(res=0.0), "resolution"),
           (dict(res=-0.1), "resolution"), (dict(inflate=-0.01), "inflate"), (dict(nx=0), "cells"), (dict(ny=-3), "cells"),
           (dict(nx=513), "cells"), (dict(ny=513), "cells"), (dict(substeps=0), "substeps"), (dict(substeps=9), "substeps")]
    for changes, word in bad:
        big = np.zeros((max(1, changes.get("ny", 20)), max(1, changes.get("nx", 30))), np.uint8)
        assert raw(planner._handle, big, **changes) == ERR_INVALID, changes
        assert word in lib.mppi_last_error().decode(), (changes, lib.mppi_last_error().decode())
    assert lib.mppi_planner_set_occupancy(planner._handle, 1, 0.0, 0.0, 0.1, 30, 20, 0.1, 2, None) == ERR_INVALID
    assert raw(planner._handle) == 0  # (what it holds: nothing happens)
    still_held()
    for broken in (dict(cells=np.zeros((20, 30))), dict(cells=np.zeros(30, np.uint8)), dict(substeps=9), dict(origin=(0.0, 0.0, 0.0))):
        refused(planner, dict(params, occupancy=dict(held["occupancy"], **broken)), "occupancy", ValueError)
    refused(planner, dict(params, occupancy=dict(held["occupancy"], resolution=-1.0)), "resolution")  # (the library's, through the mirror)
    still_held()
    with pytest.raises(_lib.MppiError) as err:  # the grid holds the handle in crowd mode
        planner.set_crowd(False)
    assert err.value.code == ERR_INVALID and "occupancy" in str(err.value), str(err.value)
    assert planner.crowd
    still_held()
    # a grid, then samples
    smp, rad = sample_set(6, 3)
    sampled = sample_params(params, smp, rad, 1.0)
    refused(planner, dict(sampled, occupancy=held["occupancy"]), "obstacle_track_samples", ValueError)
    assert lib.mppi_planner_set_disc_track_samples(planner._handle, 3, 6, smp.shape[2], _lib.ptr(np.ascontiguousarray(smp), C.c_float),
                                                   _lib.ptr(rad, C.c_float)) == ERR_INVALID
    assert "occupancy" in lib.mppi_last_error().decode()
    still_held()
    # samples, then a grid
    planner.set_params(sampled)
    assert np.isfinite(planner.solve()).all()
    with_samples = planner.last_rollout_kernel()
    assert " samples=3" in with_samples and "grid" not in with_samples, with_samples
    assert raw(planner._handle) == ERR_INVALID and "samples" in lib.mppi_last_error().decode()
    assert np.isfinite(planner.solve()).all() and planner.last_rollout_kernel() == with_samples
    # the samples go, the grid comes, in one change of the params -- and back
    planner.set_params(held)
    assert np.isfinite(planner.solve()).all() and planner.last_rollout_kernel() == kernel
    planner.set_params(sampled)
    assert np.isfinite(planner.solve()).all() and planner.last_rollout_kernel() == with_samples
    # both keys go: crowd mode can go
    planner.set_params(params)
    assert np.isfinite(planner.solve()).all() and planner.last_rollout_kernel() == plain
    planner.set_crowd(False)
    # a sharded handle
    cfg = _lib.PlannerCfg(device=0, mode=_lib.MODE_BAREBONE, num_control_rollouts=n, num_steps=T, num_grid_samples=1,
                          num_vis_state_rollouts=1, rng=_lib.RNG_PHILOX, math=_lib.MATH_EXACT, rank=0, world_size=2, num_instances=1, seed=1)
    handle = C.c_void_p()
    _lib.call("mppi_planner_create", C.byref(cfg), C.byref(handle))
    try:
        assert lib.mppi_planner_set_crowd(handle, 1) == 0
        assert raw(handle) == ERR_INVALID and "unsharded" in lib.mppi_last_error().decode()
    finally:
        lib.mppi_planner_destroy(handle)
    # a map mode has no grid
    from mppi_numba_amd.mppi import MPPI_Numba as MapPlanner
    from test_gpu_batch import make_world
    mcfg, lin, ang, mparams = make_world("c2", 128, 20)
    mapped = MapPlanner(mcfg)
    mapped.setup(mparams, lin, ang)
    assert raw(mapped._handle) == ERR_INVALID and "barebone" in lib.mppi_last_error().decode()


# ---- 6. graph replay -----------------------------------------------------------------------------------------------------
def test_graph_replay_new_cells_and_a_new_inflation():
    """New cells of the same shape land in the same arrays: no new capture.  A new inflation changes the thresholds, by-value
    arguments of the captured launches: a new capture."""
    from mppi_numba_amd.barebone import MPPI_Batch
    B, n, t = 4, 128, 30
    rng = np.random.default_rng(9)
    x0s, goals = problems(rng, B)
    cells = cases.scatter(31, (90, 90), 0.03)
    occ = dict(origin=(-2.0, -2.0), resolution=0.1, cells=cells, inflate=0.2, substeps=2)
    params = dict(make_params(0.1, 1.0, num_opt=5), occupancy=occ)
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
    assert kernel.startswith("k_rollout_barebone_crowd") and kernel.endswith(" grid=90x90"), kernel
    assert graphed.graph_stats()["replays"] >= 4, graphed.graph_stats()
    captures = graphed.graph_stats()["captures"]
    other = cases.scatter(32, (90, 90), 0.2)
    for planner in (direct, graphed):  # new cells of the same shape
        planner.params["occupancy"] = dict(occ, cells=other)
    a_, b_, c_ = step_all()
    np.testing.assert_array_equal(a_, b_)
    assert not np.array_equal(a_, c_), "bad input: other cells, the same controls"
    assert graphed.graph_stats()["captures"] == captures, "new cells of the same shape: no new capture"
    assert graphed.occupancy_fields_built == 2 and (graphed.occupancy_field() == om.field_of(other)).all()
    for planner in (direct, graphed):  # the first cells again, then a new inflation
        planner.params["occupancy"] = dict(occ)
    a_, b_, _ = step_all()
    np.testing.assert_array_equal(a_, b_)
    assert graphed.graph_stats()["captures"] == captures
    for planner in (direct, graphed):
        planner.params["occupancy"] = dict(occ, inflate=0.45)
    a_, b_, c_ = step_all()
    np.testing.assert_array_equal(a_, b_)
    assert not np.array_equal(a_, c_), "another inflation, the same controls"
    assert graphed.graph_stats()["captures"] > captures
    a_, b_, _ = step_all()
    np.testing.assert_array_equal(a_, b_)


# ---- 7. the guide --------------------------------------------------------------------------------------------------------
GUIDE = guide_of((0.0, 0.0), 0.1, (33, 31), inflate=0.0708, lead=0.6, pace=0.1)
OCC_ORIGIN, OCC_RES, OCC_SHAPE, OCC_INFLATE = (0.05, -0.05), 0.08, (45, 41), 0.04  # (the two grids do not coincide)


def guide_task(walls, cells):
    p = make_params(0.1, 1.0, num_opt=1)
    p["x0"], p["xgoal"] = np.array([0.15, 0.15, 0.8]), np.array([2.9, 3.1])
    if walls is not None:
        p["wall_segments"], p["wall_halfwidth"] = walls
    p["guide"] = GUIDE
    return grid_params(p, OCC_ORIGIN, OCC_RES, cells, OCC_INFLATE)


def guide_model_field(p):
    g, o = p["guide"], p["occupancy"]
    grid = om.Grid(o["origin"], o["resolution"], o["cells"], o["inflate"])
    guide = guide_model.Grid(g["origin"], g["resolution"], g["shape"], g["inflate"])
    return om.guide_field(guide, grid, p["xgoal"], p.get("wall_segments"), p.get("wall_halfwidth"))


@pytest.mark.parametrize("split", [0, 3])
def test_the_guide_sees_the_grid(split):
    """The room of tests/test_gpu_barebone_guide.py: only as a grid (split 0), or its first three walls as walls and the
    rest as a grid."""
    from mppi_numba_amd.barebone import MPPI_Numba, rasterise_obstacles
    seg, hw = five_walls()
    hw = np.broadcast_to(np.asarray(hw, np.float32), (len(seg),))
    cells = rasterise_obstacles(OCC_ORIGIN, OCC_RES, OCC_SHAPE, seg[split:], np.maximum(hw[split:], 0.05))
    p = guide_task((seg[:split], hw[:split]) if split else None, cells)
    planner = MPPI_Numba(cfg_of(128, T, True))
    planner.setup(p)
    planner.solve()
    want = guide_model_field(p)
    guide = guide_model.Grid(GUIDE["origin"], GUIDE["resolution"], GUIDE["shape"], GUIDE["inflate"])
    by_walls = guide_model.blocked_cells(guide, seg[:split], hw[:split]) if split else np.zeros(GUIDE["shape"], bool)
    without = guide_model.field_of(by_walls, guide_model.goal_cell(guide, p["xgoal"]))  # (the walls alone)
    assert (want != without).any() and (want < guide_model.UNREACHED).any(), "bad input: the grid blocks nothing, or everything"
    assert (planner.guide_field() == want).all(), "%d cells differ" % (planner.guide_field() != want).sum()
    kernel = planner.last_rollout_kernel()
    assert "guide=31x33" in kernel and kernel.endswith(" grid=41x45"), kernel
    assert planner.guide_fields_built == 1 and planner.occupancy_fields_built == 1
    planner.params["occupancy"] = dict(p["occupancy"], cells=cells.copy())  # the same cells as a new object
    planner.solve()
    assert planner.guide_fields_built == 1 and planner.occupancy_fields_built == 1, "unchanged cells build nothing"
    fewer = cells.copy()
    fewer[: OCC_SHAPE[0] // 2] = 0
    planner.params["occupancy"] = dict(p["occupancy"], cells=fewer)
    planner.solve()
    assert planner.guide_fields_built == 2 and planner.occupancy_fields_built == 2, "new cells build both fields once"
    q = dict(p, occupancy=dict(p["occupancy"], cells=fewer))
    assert (guide_model_field(q) != want).any(), "bad input: the new cells block the same guide cells"
    assert (planner.guide_field() == guide_model_field(q)).all()
    planner.params.pop("occupancy")  # the grid goes: the walls alone
    planner.solve()
    assert planner.guide_fields_built == 3 and (planner.guide_field() == without).all()


# ---- 8. behaviour --------------------------------------------------------------------------------------------------------
def test_a_room_that_arrives_as_a_grid():
    """A wall across the way with a doorway to the side, given only as rasterise_obstacles' cells; the goal lies behind the
    wall.  N = 1024, T = 30, the notebook's loop.  With the key and the guide over it the goal is reached and no applied
    state is a hit by the model; a twin without the key reaches the goal through the wall."""
    from mppi_numba_amd.barebone import MPPI_Numba, rasterise_obstacles
    n, t, dt, max_steps = 1024, 30, 0.1, 200
    origin, res, shape = (-1.0, -3.0), 0.1, (75, 55)
    wall = np.float32([[[1.5, -3.5], [1.5, 0.8]], [[1.5, 2.0], [1.5, 5.0]]])  # the doorway: 0.8 < y < 2.0
    cells = rasterise_obstacles(origin, res, shape, wall, 0.1)
    assert cells.any() and not cells[:, :20].any()
    params = make_params(dt, 1.0, num_opt=2)
    params["x0"], params["xgoal"], params["goal_tolerance"] = np.array([0.0, 0.0, 0.0]), np.array([3.2, 0.0]), 0.3
    inflate = 0.15
    keyed = dict(grid_params(params, origin, res, cells, inflate, 2), guide=guide_of(origin, res, shape, inflate=0.1, lead=0.45, pace=0.15))
    grid = om.Grid(origin, res, cells, inflate)
    thr = om.threshold(grid.inflate, 0.0, 0.0, grid.res)
    hits, arrived = {}, {}
    for name, p in (("with", keyed), ("without", params)):
        planner = MPPI_Numba(cfg_of(n, t, True, seed=11))
        planner.setup(p)
        x, applied = params["x0"].astype(np.float64), []
        for step in range(max_steps):
            useq = planner.solve()
            assert np.isfinite(useq).all()
            v, w = float(useq[0, 0]), float(useq[0, 1])
            x = x + dt * np.array([v * np.cos(x[2]), v * np.sin(x[2]), w])
            applied.append(x.copy())
            planner.shift_and_update(x, useq, num_shifts=1)
            if np.linalg.norm(x[:2] - params["xgoal"]) <= params["goal_tolerance"]:
                break
        assert planner.last_rollout_kernel().endswith(" grid=55x75") == (name == "with"), planner.last_rollout_kernel()
        applied = np.array(applied)
        hits[name] = int(om.point_levels(grid, applied[:, 0], applied[:, 1], np.asarray([thr]))[0].sum())
        arrived[name] = bool(np.linalg.norm(x[:2] - params["xgoal"]) <= params["goal_tolerance"])
        print("the room as a grid, %s the key: %d steps, arrived %s, %d applied states hit" % (name, step + 1, arrived[name], hits[name]))
    assert arrived["with"], "with the key: the goal is not reached"
    assert hits["with"] == 0, "with the key: %d applied states are hits" % hits["with"]
    assert arrived["without"] and hits["without"] >= 1, "the twin without the key: arrived %s, %d hits" % (arrived["without"], hits["without"])
