"""Clearance rings for the barebone planner in crowd mode (params['clearance_rings'], mppi_planner_set_clearance_rings): a
soft cost for passing close, as a staircase of up to four rings.  The ring forms of k_rollout_barebone_crowd count, per step,
the hits and for every ring the obstacles the step would touch were they a margin larger; every comparison of costs is bit
for bit -- with tests/clearance_model.py on the inputs of tests/clearance_cases.py (tests/test_clearance_model.py shows on the
CPU that they allow it), and handle against handle where a ring must equal an inflated copy of the obstacles.  The model's
states are the exact ones, so the comparisons with it run in exact math; in fast math the statements are the equalities
between handles."""
import ctypes as C
import gc

import numpy as np
import pytest

import clearance_cases as cases
import clearance_model as cm
import fleet_model
from clearance_cases import FOOTPRINTS, RINGS, ring_params, without_rings
from test_footprint_model import dyadic
from test_gpu_barebone_batch import ERR_INVALID, assert_bits, make_params, oracle_params
from test_gpu_barebone_crowd import cfg_of, shape_of
from test_gpu_barebone_disc_samples import sample_params, sample_set
from test_gpu_barebone_fleet import ROOM, ROOM_HW, fleet_ending
from test_gpu_barebone_footprint import body_params
from test_gpu_barebone_goal_tracks import goal_params
from test_gpu_barebone_tracks import rollout_with, track_params
from test_gpu_barebone_wall_tracks import track_wall_params
from test_gpu_barebone_walls import N, OBS_PENALTY, task, wall_params, without_walls
from wall_model import wall_costs

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def release_the_handles():
    """A planner and its device-array views refer to each other, so a handle lives until the cycle collector runs."""
    yield
    gc.collect()


def check_kernel(kernel, R, t, wscale, F=0, exact=True):
    chunk = shape_of(kernel)[1]
    assert t > chunk, kernel
    assert kernel.endswith((" footprint=%d" % F if F else "") + " rings=%d" % R), kernel
    assert ("footprint" in kernel) == bool(F), kernel
    assert ("rotation=1" in kernel) == (exact and wscale == 1.0) and ("exact=%d" % exact) in kernel, kernel


# ---- 1. costs against the model: the point robot -------------------------------------------------------------------------
@pytest.mark.parametrize("R,K,W,t,wscale", cases.point_cases())
def test_costs_equal_the_model(R, K, W, t, wscale):
    """Static discs, then tracks at offsets 0 and 5, on one handle.  K = 70: two disc tiles; W = 65: two wall tiles;
    N = 200: a partial last tile."""
    from mppi_numba_amd.barebone import MPPI_Numba
    params, u_in, noise = task(t, wscale)
    p = oracle_params(without_walls(params))
    rings = RINGS[R]
    planner = MPPI_Numba(cfg_of(N, t, True))
    differs = False
    for kind in ("static", "tracks"):
        full, tracks, rad, seg, hw = cases.scene(K, W, kind, t, wscale)
        planner.set_params(ring_params(full, rings))
        for offset in ((0, 5) if kind == "tracks" else (0,)):
            model = cm.costs(p, rings, tracks, rad, seg, hw, noise, u_in, offset=offset)
            planner.move_mppi_task_vars_to_device()  # (hands the tracks over the first time: offset 0)
            planner.set_track_offset(offset)
            got, _, _, kernel = rollout_with(planner, u_in, noise)
            check_kernel(kernel, R, t, wscale)
            assert ("tracks=%d" % (t + 1) in kernel) == (kind == "tracks"), kernel
            assert (" walls=%d" % W in kernel) == (W > 0), kernel
            assert_bits(got, model, "R = %d, %d discs (%s, offset %d), %d walls vs the model" % (R, K, kind, offset, W))
            plain = wall_costs(p, tracks, rad, *((seg, hw) if W else cases.NO_WALLS), noise, u_in, offset)
            differs = differs or (plain.view(np.int32) != model.view(np.int32)).any()
    np.testing.assert_array_equal(planner.clearance_rings, rings)
    assert differs == bool(K or W), "bad input: the rings cost nothing"


# ---- 2. ... and a body ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("F,t,wscale", cases.body_cases())
def test_costs_with_a_footprint_equal_the_model(F, t, wscale):
    from mppi_numba_amd.barebone import MPPI_Numba
    R, K, W = 2, 70, 65
    params, u_in, noise = task(t, wscale)
    p = oracle_params(without_walls(params))
    rings, fp = RINGS[R], FOOTPRINTS[F]
    planner = MPPI_Numba(cfg_of(N, t, True))
    for kind in ("static", "tracks"):
        full, tracks, rad, seg, hw = cases.scene(K, W, kind, t, wscale)
        planner.set_params(ring_params(body_params(full, fp), rings))
        for offset in ((0, 5) if kind == "tracks" else (0,)):
            model = cm.costs(p, rings, tracks, rad, seg, hw, noise, u_in, footprint=fp, offset=offset)
            planner.move_mppi_task_vars_to_device()
            planner.set_track_offset(offset)
            got, _, _, kernel = rollout_with(planner, u_in, noise)
            check_kernel(kernel, R, t, wscale, F)
            assert_bits(got, model, "F = %d, R = %d, %s discs at offset %d vs the model" % (F, R, kind, offset))
            free = rings.copy()
            free[:, 1] = 0.0
            assert (model != cm.costs(p, free, tracks, rad, seg, hw, noise, u_in, footprint=fp, offset=offset)).any(), "bad input"


def test_wall_tracks_beside_the_rings():
    from mppi_numba_amd.barebone import MPPI_Numba
    t, wscale, R, F = 37, 1.0, 2, 3
    params, u_in, noise = task(t, wscale)
    p = oracle_params(without_walls(params))
    where, rad, wtracks, hw, _ = cases.wall_track_case(t)
    rings, fp = RINGS[R], FOOTPRINTS[F]
    planner = MPPI_Numba(cfg_of(N, t, True))
    planner.set_params(ring_params(body_params(track_wall_params(track_params(params, where, rad), wtracks, hw), fp), rings))
    for offset in (0, 5):
        model = cm.costs(p, rings, where, rad, wtracks, hw, noise, u_in, footprint=fp, offset=offset)
        assert (model != cm.costs(p, rings, where, rad, wtracks[:, 0], hw, noise, u_in, footprint=fp, offset=offset)).any(), \
            "bad input: the rows cannot be told apart"
        planner.move_mppi_task_vars_to_device()
        planner.set_track_offset(offset)
        got, _, _, kernel = rollout_with(planner, u_in, noise)
        check_kernel(kernel, R, t, wscale, F)
        assert " walls=65 wall_rows=%d" % (t + 1) in kernel, kernel
        assert_bits(got, model, "wall tracks at offset %d vs the model" % offset)


def test_a_goal_track_beside_the_rings():
    from mppi_numba_amd.barebone import MPPI_Numba
    t, wscale, R, F = 37, 1.0, 2, 3
    params, u_in, noise = task(t, wscale)
    track = cases.wall_track_case(t)[4]
    p = oracle_params(dict(without_walls(params), xgoal=track[0]))
    rings, fp = RINGS[R], FOOTPRINTS[F]
    full, tracks, rad, seg, hw = cases.scene(3, 1, "static", t, wscale)
    planner = MPPI_Numba(cfg_of(N, t, True))
    planner.set_params(ring_params(body_params(goal_params(full, track), fp), rings))
    got, _, _, kernel = rollout_with(planner, u_in, noise)
    shape_of(kernel)
    assert kernel.endswith(" walls=1 goal_rows=%d footprint=%d rings=%d" % (t + 1, F, R)), kernel
    model = cm.costs(p, rings, tracks, rad, seg, hw, noise, u_in, footprint=fp, goal_track=track)
    assert (model != cm.costs(p, rings, tracks, rad, seg, hw, noise, u_in, footprint=fp, goal_track=track[:1])).any(), \
        "bad input: the goal's rows cannot be told apart"
    assert_bits(got, model, "a goal track beside the rings vs the model")
    # ... and the point robot's goal form
    planner.set_params(ring_params(goal_params(full, track), rings))
    got, _, _, kernel = rollout_with(planner, u_in, noise)
    assert kernel.endswith(" walls=1 goal_rows=%d rings=%d" % (t + 1, R)), kernel
    assert_bits(got, cm.costs(p, rings, tracks, rad, seg, hw, noise, u_in, goal_track=track), "... and without the body")


# ---- 3. rings as inflated copies: against the kernels without rings ------------------------------------------------------
def inflated(full, margins):
    """The params of `full` (static discs and static walls, dyadic sizes) with every obstacle once at its own size and once
    more per margin at size + margin (exact in float32)."""
    pos, rad = np.asarray(full["obstacle_positions"], np.float32), np.asarray(full["obstacle_radius"], np.float32)
    seg, hw = np.asarray(full["wall_segments"], np.float32), np.asarray(full["wall_halfwidth"], np.float32)
    grown = [np.float32(0.0)] + [np.float32(m) for m in margins]
    for m in grown:
        assert ((rad + m).astype(np.float64) == rad.astype(np.float64) + np.float64(m)).all()
        assert ((hw + m).astype(np.float64) == hw.astype(np.float64) + np.float64(m)).all()
    out = dict(full)
    out["obstacle_positions"], out["obstacle_radius"] = np.concatenate([pos] * len(grown)), np.concatenate([rad + m for m in grown])
    out["wall_segments"], out["wall_halfwidth"] = np.concatenate([seg] * len(grown)), np.concatenate([hw + m for m in grown])
    return out


@pytest.mark.parametrize("math", ["exact", "fast"])
@pytest.mark.parametrize("K,W,F", [(3, 1, 0), (70, 65, 0), (70, 65, 1)])
@pytest.mark.parametrize("t,wscale", cases.TASKS)
def test_rings_are_inflated_copies(math, K, W, F, t, wscale):
    """Every penalty equals obs_penalty, radii, half-widths and margins are dyadic: R rings cost, bit for bit, what a handle
    without rings is charged that holds the discs and walls once at their own size and once more per ring at
    size + margin.  F = 1: one body disc off the axis with a dyadic rho, in both handles."""
    from mppi_numba_amd.barebone import MPPI_Numba
    params, u_in, noise = task(t, wscale)
    full = cases.scene(K, W, "static", t, wscale)[0]
    full["obstacle_radius"], full["wall_halfwidth"] = dyadic(full["obstacle_radius"]), dyadic(full["wall_halfwidth"])
    margins = (0.25, 0.5)
    rings = np.float32([[m, OBS_PENALTY] for m in margins])
    fp = np.float32([[0.25, 0.125, 5.0 / 64]])
    with_body = (lambda q: body_params(q, fp)) if F else (lambda q: q)
    ringed, copies = MPPI_Numba(cfg_of(N, t, True, math)), MPPI_Numba(cfg_of(N, t, True, math))
    copies.set_params(with_body(inflated(full, margins)))
    want, want_u, _, copy_kernel = rollout_with(copies, u_in, noise)
    assert "rings" not in copy_kernel and " walls=%d" % (3 * W) in copy_kernel, copy_kernel
    ringed.set_params(ring_params(with_body(full), rings))
    got, got_u, _, kernel = rollout_with(ringed, u_in, noise)
    check_kernel(kernel, 2, t, wscale, F, math == "exact")
    assert_bits(got, want, "%s math, %d discs, %d walls, F = %d: two rings vs two inflated copies" % (math, K, W, F))
    assert_bits(got_u, want_u, "... and the update")
    copies.set_params(with_body(full))
    assert (rollout_with(copies, u_in, noise)[0] != want).any(), "bad input: the copies cost nothing"
    if math == "exact":
        p = oracle_params(without_walls(params))
        model = cm.costs(p, rings, np.asarray(full["obstacle_positions"], np.float32)[:, None, :], full["obstacle_radius"],
                         full["wall_segments"], full["wall_halfwidth"], noise, u_in, footprint=fp if F else None)
        assert_bits(got, model, "... and the model")


# ---- 4. a ring of penalty 0; the key comes and goes ----------------------------------------------------------------------
@pytest.mark.parametrize("math", ["exact", "fast"])
def test_a_free_ring_and_clearing_the_key(math):
    from mppi_numba_amd.barebone import MPPI_Numba
    t, wscale = 37, 1.0
    params, u_in, noise = task(t, wscale)
    full = cases.scene(70, 65, "static", t, wscale)[0]
    planner = MPPI_Numba(cfg_of(N, t, True, math))
    planner.set_params(full)
    before, before_u, _, before_kernel = rollout_with(planner, u_in, noise)
    assert planner.clearance_rings is None and "rings" not in before_kernel
    free = np.float32([[0.1, 0.0], [0.4, 0.0]])
    planner.set_params(ring_params(full, free))
    held, held_u, _, kernel = rollout_with(planner, u_in, noise)
    check_kernel(kernel, 2, t, wscale, 0, math == "exact")
    assert kernel != before_kernel
    np.testing.assert_array_equal(planner.clearance_rings, free)
    assert_bits(held, before, "%s math: rings that cost nothing vs no rings" % math)
    assert_bits(held_u, before_u, "... and the update")
    planner.set_params(ring_params(full, RINGS[4]))
    paid, _, _, kernel = rollout_with(planner, u_in, noise)
    check_kernel(kernel, 4, t, wscale, 0, math == "exact")
    assert (paid != before).any()
    planner.set_params(full)
    after, after_u, _, after_kernel = rollout_with(planner, u_in, noise)
    assert after_kernel == before_kernel, (before_kernel, after_kernel)
    assert planner.clearance_rings is None
    assert_bits(after, before, "the key has gone: the costs without rings")
    assert_bits(after_u, before_u, "... and the update")
    # no discs, no walls: rings still launch the crowd kernel; without them the default form is back
    bare = MPPI_Numba(cfg_of(N, t, True, math))
    bare.set_params(ring_params(params, RINGS[1]))
    alone, _, _, kernel = rollout_with(bare, u_in, noise)
    check_kernel(kernel, 1, t, wscale, 0, math == "exact")
    bare.set_params(params)
    plain, _, _, plain_kernel = rollout_with(bare, u_in, noise)
    assert plain_kernel.startswith("k_rollout_barebone exact"), plain_kernel
    assert_bits(alone, plain, "nothing to be near to: the costs of the default form")


# ---- 5. a batch ----------------------------------------------------------------------------------------------------------
def test_batch_with_per_problem_discs_and_walls():
    """B = 3 problems of n = 64, each with its own disc set and wall set, one ring set: problem b equals a single planner
    bit for bit, and the model."""
    from mppi_numba_amd.barebone import MPPI_Batch, MPPI_Numba
    case = cases.batch_case()
    B, n, t, rings = case["B"], case["n"], case["t"], case["rings"]
    batch = MPPI_Batch(cfg_of(n, t, True), B)
    batch.setup(ring_params(case["params"], rings), case["x0s"], case["goals"], obstacle_sets=case["sets"], wall_sets=case["wall_sets"])
    costs, u_out, _, kernel = rollout_with(batch, case["u_in"], case["noise"].reshape(B * n, t, 2))
    shape_of(kernel)
    assert "problems=%d" % B in kernel and kernel.endswith(" rings=%d" % len(rings)), kernel
    single = MPPI_Numba(cfg_of(n, t, True))
    for b in range(B):
        pb, p, tracks, rad, seg, hw = cases.batch_problem(case, b)
        single.set_params(ring_params(wall_params(pb, seg, hw) if seg is not None else pb, rings))
        want, want_u, _, single_kernel = rollout_with(single, case["u_in"][b], case["noise"][b])
        assert single_kernel.endswith(" rings=%d" % len(rings)) and "problems" not in single_kernel, single_kernel
        what = "problem %d (%d discs, %d walls)" % (b, case["counts"][b], case["wcounts"][b])
        assert_bits(costs[b], want, what + " vs a single handle")
        assert_bits(u_out[b], want_u, what + ": u vs a single handle")
        model = cm.costs(p, rings, tracks, rad, seg, hw, case["noise"][b], case["u_in"][b])
        assert_bits(costs[b], model, what + " vs the model")
        assert (model != wall_costs(p, tracks, rad, *((seg, hw) if seg is not None else cases.NO_WALLS), case["noise"][b], case["u_in"][b])).any()


# ---- 6. the fleets -------------------------------------------------------------------------------------------------------
def test_the_disc_fleet_with_rings():
    """The fleet's walls are walls like any other: fleet_model's rows, the ring model's counts."""
    from mppi_numba_amd.barebone import MPPI_Batch
    case = cases.disc_fleet_case()
    B, n, t, W, rings = case["B"], case["n"], case["t"], case["W"], case["rings"]
    batch = MPPI_Batch(cfg_of(n, t, True), B)
    batch.setup(ring_params(wall_params(case["params"], ROOM[:W], ROOM_HW[:W]), rings), case["x0s"], case["goals"])
    batch.set_fleet(np.asarray(cases.FLEET_RADII), cases.FLEET_MARGIN)
    costs, _, _, kernel = rollout_with(batch, case["us"], case["noise"].reshape(B * n, t, 2))
    shape_of(kernel)
    assert kernel.endswith(fleet_ending(B, W, t) + " rings=%d" % len(rings)) and "problems=%d" % B in kernel, kernel
    seg = batch.fleet_walls()[0]
    assert_bits(seg, fleet_model.fleet_walls(case["params"], case["x0s"], case["us"]), "the fleet's walls vs the model")
    differs = False
    for b in range(B):
        p, wt, h = case["readers"][b]
        model = cm.costs(p, rings, *cases.NO_DISCS, wt, h, case["noise"][b], case["us"][b], wall_offset=0)
        assert_bits(costs[b], model, "robot %d of the disc fleet vs the model" % b)
        differs = differs or (model != fleet_model.fleet_costs(p, wt, h, case["noise"][b], case["us"][b])).any()
    assert differs, "bad input: the rings cost nothing"


def test_the_fleet_of_bodies_with_rings():
    """F = 3, four slots a robot: a robot is near at ring l ONCE, however many of its slots are -- every level's mask is
    folded on its own.  tests/test_clearance_model.py asserts on the model that some (rollout, step) has two body discs of
    one robot inside a ring and none hit; here, that counting per slot would give other costs than the device's."""
    from mppi_numba_amd.barebone import MPPI_Batch
    case = cases.body_fleet_case()
    B, n, t, W, F, rings = case["B"], case["n"], case["t"], case["W"], case["F"], case["rings"]
    batch = MPPI_Batch(cfg_of(n, t, True), B)
    batch.setup(ring_params(wall_params(case["params"], ROOM[:W], ROOM_HW[:W]), rings), case["x0s"], case["goals"])
    batch.set_fleet_bodies(case["footprint"], case["margin"])
    costs, _, _, kernel = rollout_with(batch, case["us"], case["noise"].reshape(B * n, t, 2))
    shape_of(kernel)
    assert " walls=%d wall_rows=%d fleet=%d" % (case["grouped"] + W, t, B) in kernel, kernel
    assert kernel.endswith(" footprint=%d rings=%d" % (F, len(rings))), kernel
    per_slot_differs = False
    for a in range(B):
        p, seg, hw = case["readers"][a]
        args = (p, rings) + cases.NO_DISCS + (seg, hw, case["noise"][a], case["us"][a], case["footprint"])
        model = cm.costs(*args, wall_offset=0, group=case["group"], grouped=case["grouped"])
        assert_bits(costs[a], model, "robot %d of the fleet of bodies vs the model" % a)
        per_slot_differs = per_slot_differs or (model != cm.costs(*args, wall_offset=0)).any()
    assert per_slot_differs, "bad input: counting per slot gives the same costs"


# ---- 7. refusals ---------------------------------------------------------------------------------------------------------
def test_refusals():
    from mppi_numba_amd import _lib
    from mppi_numba_amd.barebone import MPPI_Numba
    n, t = 128, 30
    params = make_params(0.1, 1.0)
    lib = _lib.load()

    def raw(planner, rows):
        rows = np.ascontiguousarray(rows, np.float32)
        return lib.mppi_planner_set_clearance_rings(planner._handle, _lib.ptr(rows, C.c_float), len(rows))

    def refused(planner, p, word, error=_lib.MppiError):
        planner.set_params(p)
        with pytest.raises(error) as err:
            planner.solve()
        if error is _lib.MppiError:
            assert err.value.code == ERR_INVALID
        assert word in str(err.value), str(err.value)

    planner = MPPI_Numba(cfg_of(n, t, False))
    planner.setup(params)
    assert np.isfinite(planner.solve()).all()
    plain = planner.last_rollout_kernel()
    refused(planner, ring_params(params, RINGS[2]), "crowd")  # no crowd mode: no rings
    assert planner.clearance_rings is None
    planner.set_params(params)
    assert np.isfinite(planner.solve()).all() and planner.last_rollout_kernel() == plain
    planner.set_crowd(True)
    planner.set_params(ring_params(params, RINGS[2]))
    assert np.isfinite(planner.solve()).all()
    held = planner.last_rollout_kernel()
    assert held.startswith("k_rollout_barebone_crowd") and held.endswith(" rings=2"), held

    def still_held():
        np.testing.assert_array_equal(planner.clearance_rings, RINGS[2])
        planner.set_params(ring_params(params, RINGS[2]))
        assert np.isfinite(planner.solve()).all() and planner.last_rollout_kernel() == held

    for bad in (np.ones((5, 2), np.float32), np.zeros((0, 2), np.float32), np.ones((2, 3), np.float32), np.ones(2, np.float32)):
        refused(planner, ring_params(params, bad), "clearance_rings", ValueError)  # R = 5, R = 0, a wrong shape
    five = np.float32([[0.1 * (l + 1), 1.0] for l in range(5)])
    assert raw(planner, five) == ERR_INVALID and "5" in lib.mppi_last_error().decode()
    still_held()
    for rows, word in (([[0.3, 1.0], [0.3, 1.0]], "exceed"), ([[0.3, 1.0], [0.1, 1.0]], "exceed"), ([[0.0, 1.0]], "positive"),
                       ([[-0.1, 1.0]], "positive"), ([[0.1, -1.0]], "negative"), ([[np.nan, 1.0]], "finite"), ([[0.1, np.nan]], "finite"),
                       ([[np.inf, 1.0]], "finite"), ([[0.1, 1.0], [0.2, np.inf]], "finite")):
        refused(planner, ring_params(params, np.float32(rows)), word)
        assert raw(planner, np.float32(rows)) == ERR_INVALID
        still_held()
    with pytest.raises(_lib.MppiError) as err:  # the rings hold the handle in crowd mode
        planner.set_crowd(False)
    assert err.value.code == ERR_INVALID and "rings" in str(err.value), str(err.value)
    assert planner.crowd
    still_held()
    # rings, then samples
    smp, rad = sample_set(6, 3)
    sampled = sample_params(params, smp, rad, 1.0)
    refused(planner, ring_params(sampled, RINGS[2]), "rings")
    assert lib.mppi_planner_set_disc_track_samples(planner._handle, 3, 6, smp.shape[2], _lib.ptr(np.ascontiguousarray(smp), C.c_float),
                                                   _lib.ptr(rad, C.c_float)) == ERR_INVALID
    still_held()
    # samples, then rings
    planner.set_params(sampled)
    assert np.isfinite(planner.solve()).all()
    with_samples = planner.last_rollout_kernel()
    assert " samples=3" in with_samples and "rings" not in with_samples and planner.clearance_rings is None, with_samples
    refused(planner, ring_params(sampled, RINGS[2]), "samples")
    assert raw(planner, RINGS[2]) == ERR_INVALID and "samples" in lib.mppi_last_error().decode()
    assert planner.clearance_rings is None
    planner.set_params(sampled)
    assert np.isfinite(planner.solve()).all() and planner.last_rollout_kernel() == with_samples
    # both keys go: crowd mode can go
    planner.set_params(params)
    assert np.isfinite(planner.solve()).all() and planner.last_rollout_kernel() == plain
    planner.set_crowd(False)
    # a map mode has no rings
    from mppi_numba_amd.mppi import MPPI_Numba as MapPlanner
    from test_gpu_batch import make_world
    mcfg, lin, ang, mparams = make_world("c2", 128, 20)
    mapped = MapPlanner(mcfg)
    mapped.setup(mparams, lin, ang)
    assert raw(mapped, RINGS[2]) == ERR_INVALID and "barebone" in lib.mppi_last_error().decode()


# ---- 8. graph replay -----------------------------------------------------------------------------------------------------
def test_graph_replay_and_changed_rings():
    """The rings' rows are by-value arguments of the captured launches: changed rings must not replay them."""
    from mppi_numba_amd.barebone import MPPI_Batch
    from test_gpu_barebone_batch import problems
    B, n, t = 4, 128, 30
    rng = np.random.default_rng(9)
    x0s, goals = problems(rng, B)
    a = rng.uniform(-1.0, 4.0, (70, 2))
    seg = np.stack([a, a + rng.uniform(-1.0, 1.0, (70, 2))], axis=1).astype(np.float32)
    hw = rng.uniform(0.0, 0.15, 70).astype(np.float32)
    params = ring_params(wall_params(make_params(0.1, 1.0, num_opt=5), seg, hw), RINGS[2])
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
    assert kernel.startswith("k_rollout_barebone_crowd") and kernel.endswith(" walls=70 rings=2"), kernel
    assert graphed.graph_stats()["replays"] >= 4, graphed.graph_stats()
    captures = graphed.graph_stats()["captures"]
    for planner in (direct, graphed):  # the same rows as a new object: nothing changes
        planner.params["clearance_rings"] = RINGS[2].copy()
    a_, b_, c_ = step_all()
    np.testing.assert_array_equal(a_, b_)
    np.testing.assert_array_equal(a_, c_)
    assert graphed.graph_stats()["captures"] == captures, "the same rings again: no new capture"
    wider = RINGS[2].copy()  # the same count, other rows: only the by-value argument differs
    wider[:, 0] += np.float32(0.3)
    for planner in (direct, graphed):
        planner.params["clearance_rings"] = wider
    a_, b_, c_ = step_all()
    np.testing.assert_array_equal(a_, b_)
    assert not np.array_equal(a_, c_), "other rings, the same controls"
    assert graphed.graph_stats()["captures"] > captures
    a_, b_, _ = step_all()
    np.testing.assert_array_equal(a_, b_)


# ---- 9. behaviour --------------------------------------------------------------------------------------------------------
def test_the_plan_keeps_its_distance():
    """One scene, fixed seed, N = 1024, T = 30: from (0, 0, 0) to (6, 0) past a disc of radius 0.5 at (3, 0.3), the notebook's
    control loop -- solve() of num_opt = 1 iteration, a float64 Euler step with the first control, shift_and_update -- until
    the goal is reached.  (One solve() from rest ends 0.575 m short of the disc, with and without rings alike: the plan has to be followed.)
    The smallest gap between any step's noise-free plan (fleet_model.plans: the rollout of the solved controls without
    noise, its first state the robot's own) and the disc is strictly larger with clearance_staircase(0.5, obs_penalty / 4, 4)
    than on a twin handle without rings."""
    from mppi_numba_amd.barebone import MPPI_Numba, clearance_staircase
    n, t, dt, max_steps = 1024, 30, 0.1, 100
    centre, radius = np.float32([3.0, 0.3]), np.float32(0.5)
    params = make_params(dt, 1.0, discs=(centre[None], radius[None]))
    params["x0"], params["xgoal"] = np.array([0.0, 0.0, 0.0]), np.array([6.0, 0.0])
    rings = clearance_staircase(0.5, OBS_PENALTY / 4, 4)
    gaps, steps = {}, {}
    for name, p in (("without", params), ("with", ring_params(params, rings))):
        planner = MPPI_Numba(cfg_of(n, t, True, seed=11))
        planner.setup(p)
        x, gap = params["x0"].astype(np.float64), np.inf
        for step in range(max_steps):
            useq = planner.solve()
            assert np.isfinite(useq).all()
            plan = fleet_model.plans(without_rings(params), x[None], useq[None])[0]
            gap = min(gap, float(np.linalg.norm(plan[:, :2].astype(np.float64) - centre.astype(np.float64), axis=1).min() - float(radius)))
            v, w = float(useq[0, 0]), float(useq[0, 1])
            x = x + dt * np.array([v * np.cos(x[2]), v * np.sin(x[2]), w])
            planner.shift_and_update(x, useq, num_shifts=1)
            if np.linalg.norm(x[:2] - params["xgoal"]) <= params["goal_tolerance"]:
                break
        assert planner.last_rollout_kernel().endswith(" rings=4") == (name == "with"), planner.last_rollout_kernel()
        assert np.linalg.norm(x[:2] - params["xgoal"]) <= params["goal_tolerance"], "%s rings: the goal is not reached" % name
        gaps[name], steps[name] = gap, step + 1
    print("smallest gap between a plan and the disc: %.4f m without rings (%d steps), %.4f m with (%d steps)" % (
        gaps["without"], steps["without"], gaps["with"], steps["with"]))
    assert gaps["with"] > gaps["without"], gaps
