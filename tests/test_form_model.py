"""tests/form_model.py and the inputs of tests/form_cases.py, on the CPU: (a) the composition gives, bit for bit, what each
feature's own model gives on that feature; (b) no disc verdict of the sweep's inputs is near enough to its boundary for the
kernel's fma to flip it; (c) the inputs mean something -- the statements that make a pass of
tests/test_gpu_barebone_form_models.py worth having."""
import functools

import numpy as np
import pytest

import clearance_model as cm
import disc_samples_model
import footprint_model
import form_cases as fc
import form_model
import goal_track_model
import wall_model
import wall_track_model
from form_cases import ALPHA, BODY, N, OFFSETS, RING_ROWS, S


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype == np.float32 and a.shape == b.shape and (a.view(np.int32) == b.view(np.int32)).all()


def plain(sc):
    return fc.oracle_of(sc, fc.ROWS[0])


# ---- (a) the composition equals the feature models --------------------------------------------------------------------------
@pytest.mark.parametrize("K,W,wscale", [(7, 10, 1.5), (70, 74, 1.0)])
@pytest.mark.parametrize("offset", OFFSETS)
def test_the_composition_equals_the_feature_models(K, W, wscale, offset):
    sc = fc.scene(K, W, wscale)
    p, goal = plain(sc), sc["goal_track"]
    pg = fc.oracle_of(sc, ("tracks", "tracks", True, (), False))
    u, noise = sc["u"][1], sc["noise"][1]
    tracks, rad, seg, hw, wtracks = sc["tracks"], sc["rad"], sc["seg"], sc["hw"], sc["wtracks"]
    smp, srad = sc["samples"], sc["sample_rad"]
    # walls, static and with tracks
    assert same_bits(form_model.costs(p, tracks, rad, seg, hw, noise, u, offset=offset),
                     wall_model.wall_costs(p, tracks, rad, seg, hw, noise, u, offset))
    assert same_bits(form_model.costs(p, sc["pos"][:, None], rad, seg, hw, noise, u),
                     wall_model.wall_costs(p, sc["pos"][:, None], rad, seg, hw, noise, u))
    assert same_bits(form_model.costs(p, tracks, rad, wtracks, hw, noise, u, offset=offset),
                     wall_track_model.wall_track_costs(p, tracks, rad, wtracks, hw, noise, u, offset))
    # a goal track, with and without walls
    assert same_bits(form_model.costs(pg, tracks, rad, wtracks, hw, noise, u, goal_track=goal, offset=offset),
                     goal_track_model.goal_track_costs(pg, goal, noise, u, offset, tracks, rad, wtracks, hw))
    assert same_bits(form_model.costs(pg, tracks, rad, None, None, noise, u, goal_track=goal, offset=offset),
                     goal_track_model.goal_track_costs(pg, goal, noise, u, offset, tracks, rad))
    # disc samples: the columns and the tail, beside static walls, and beside wall tracks and a goal track
    assert same_bits(form_model.sample_costs(p, smp, srad, seg, hw, noise, u, offset=offset),
                     disc_samples_model.sample_costs(p, smp, srad, noise, u, offset=offset, wall_segments=seg, halfwidths=hw))
    assert same_bits(form_model.costs(pg, smp, srad, wtracks, hw, noise, u, goal_track=goal, alpha=ALPHA, offset=offset),
                     disc_samples_model.costs(pg, smp, srad, noise, u, ALPHA, offset=offset, wall_tracks=wtracks, halfwidths=hw,
                                              goal_track=goal))
    # rings, with and without a body
    assert same_bits(form_model.costs(p, tracks, rad, wtracks, hw, noise, u, rings=RING_ROWS, offset=offset),
                     cm.costs(p, RING_ROWS, tracks, rad, wtracks, hw, noise, u, offset=offset))
    assert same_bits(form_model.costs(pg, tracks, rad, seg, hw, noise, u, footprint=BODY, rings=RING_ROWS, goal_track=goal, offset=offset),
                     cm.costs(pg, RING_ROWS, tracks, rad, seg, hw, noise, u, footprint=BODY, offset=offset, goal_track=goal))
    # a body: plain, with a goal track, under samples
    assert same_bits(form_model.costs(p, tracks, rad, wtracks, hw, noise, u, footprint=BODY, offset=offset),
                     footprint_model.costs(p, BODY, tracks, rad, wtracks, hw, noise, u, offset))
    assert same_bits(form_model.costs(pg, tracks, rad, seg, hw, noise, u, footprint=BODY, goal_track=goal, offset=offset),
                     footprint_model.costs(pg, BODY, tracks, rad, seg, hw, noise, u, offset, goal_track=goal))
    assert same_bits(form_model.sample_costs(p, smp, srad, wtracks, hw, noise, u, footprint=BODY, offset=offset),
                     footprint_model.sample_costs(p, BODY, smp, srad, wtracks, hw, noise, u, offset))
    assert same_bits(form_model.costs(p, smp, srad, wtracks, hw, noise, u, footprint=BODY, alpha=ALPHA, offset=offset),
                     footprint_model.sampled_costs(p, BODY, smp, srad, wtracks, hw, noise, u, ALPHA, offset))


def test_the_sweep_holds_the_table_of_forms():
    """32 rows, 32 forms: the 12 plain ones and the 20 with samples, rings or a footprint (crowd_form_legal of
    csrc/barebone_plan.h); half of the 20 reach theirs through the one-row normalisation."""
    forms = [fc.form_of(row) for row in fc.ROWS]
    assert len(fc.ROWS) == 32 and len(set(forms)) == 32
    assert sum(1 for f in forms if not (f[3] or f[4] or f[5])) == 12
    for tracks, walls, goal, samples, rings, footprint in forms:
        extra = samples or rings or footprint
        assert not (samples and rings) and (not extra or (tracks and walls != "static"))
    assert sum(row[4] for row in fc.EXTRA_ROWS) == 10
    for extra in fc.EXTRAS:
        assert {row[4] for row in fc.EXTRA_ROWS if row[3] == extra} == {False, True}


# ---- (b) no disc verdict can flip ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,W,wscale", fc.scenes())
def test_no_disc_verdict_of_the_sweep_can_flip(K, W, wscale):
    """The bound and its reason are those of test_clearance_model.py::test_no_disc_verdict_of_the_gpu_inputs_can_flip: the
    kernel's fma(ex, ex, ey * ey) - rr and the model's ex * ex + ey * ey - rr differ by a few ulps of a number below
    50^2 m^2, some 1e-12; every disc test of the sweep -- every problem, offset, ring margin and body disc, every sample on
    its own -- is 1e-9 away from its boundary at the least."""
    sc = fc.scene(K, W, wscale)
    sets = [("static discs", sc["pos"][:, None], sc["rad"]), ("disc tracks", sc["tracks"], sc["rad"])]
    sets += [("sample %d" % s, sc["samples"][s], sc["sample_rad"]) for s in range(S)]
    sets += [("sample %d of one row" % s, sc["samples1"][s], sc["sample1_rad"]) for s in range(S)]
    assert all(np.abs(tracks).max() < 50.0 for _, tracks, _ in sets)
    least = np.inf
    for b in range(fc.B):
        st = wall_model.states(plain(sc), sc["noise"][b], sc["u"][b])
        assert np.abs(st[:, :, :2]).max() < 50.0
        for what, tracks, rad in sets:
            for footprint in (None, BODY):
                for offset in (OFFSETS if tracks.shape[1] > 1 else OFFSETS[:1]):
                    margin = cm.smallest_disc_margin(st, RING_ROWS, tracks, rad, footprint, offset)
                    assert margin >= 1e-9, "problem %d, %s, body %s, offset %d: %.3g" % (b, what, footprint is not None, offset, margin)
                    least = min(least, margin)
    print("K = %d, wscale %g: smallest disc margin %.3g" % (K, wscale, least))


@pytest.mark.parametrize("wscale", fc.WSCALES)
def test_no_disc_verdict_of_the_mixed_batch_can_flip(wscale):
    """Problems 0 and 1 are the sweep's (fewer discs of the same set: no new test); problem 2 has no discs of its own and
    meets the shared samples of the samples row."""
    sc = fc.scene(70, 74, wscale)
    u, noise = fc.mixed_inputs(wscale)
    st = wall_model.states(plain(sc), noise[2], u[2])
    for s in range(S):
        assert cm.smallest_disc_margin(st, RING_ROWS, sc["samples"][s], sc["sample_rad"], BODY, fc.MIXED_OFFSETS[2]) >= 1e-9
    for b in (0, 1):
        st = wall_model.states(plain(sc), noise[b], u[b])
        for tracks, rad in [(sc["tracks"], sc["rad"])] + [(sc["samples"][s], sc["sample_rad"]) for s in range(S)]:
            for footprint in (None, BODY):
                assert cm.smallest_disc_margin(st, RING_ROWS, tracks, rad, footprint, fc.MIXED_OFFSETS[b]) >= 1e-9


# ---- (c) the input means something -------------------------------------------------------------------------------------------
def differ(a, b):
    return a.view(np.int32) != b.view(np.int32)


@functools.lru_cache(maxsize=None)
def _walled_lanes(K, W, wscale, moving, body, b):
    sc = fc.scene(K, W, wscale)
    st = wall_model.states(plain(sc), sc["noise"][b], sc["u"][b])
    none = sc["tracks"][:0], sc["rad"][:0]
    return cm.level_masks(st, [0.0], *none, sc["wtracks"] if moving else sc["seg"], sc["hw"], BODY if body else None)[1][0]


def walled_lanes(sc, row, b):
    """(n, T, W) bool: the model's per-wall hits of problem b in a row -- of the walls the row is given (static ones, or
    tracks), by the point robot or the body."""
    return _walled_lanes(sc["K"], sc["W"], sc["wscale"], row[1] == "tracks" and not row[4], "footprint" in row[3], b)


FULL = ("tracks", "tracks", True, (), False)  # the plain row with everything that moves


@pytest.mark.parametrize("K,W,wscale", fc.scenes())
def test_the_input_means_something(K, W, wscale):
    sc = fc.scene(K, W, wscale)
    idle = W % 64  # the lanes of the partial wall tile from here on hold a rollout and no wall
    for b in range(fc.B):
        what = "bad input (K = %d, W = %d, wscale %g, problem %d): " % (K, W, wscale, b)
        costs = {row: fc.model(K, W, wscale, row, b)[0] for row in fc.ROWS}
        for row, c in costs.items():
            assert len(np.unique(c)) > N // 2, what + "the costs of %s are alike" % (row,)
        # walls: hits on the rollouts of the idle lanes, in every kind of wall walk; walls of the second tile; two hits a step
        for row in [r for r in fc.ROWS if r[1] != "none"]:
            masks = walled_lanes(sc, row, b)
            hit = masks.any(axis=(1, 2))
            assert hit[idle:].sum() > (N - idle) // 2, what + "%s: %d of the %d rollouts in lanes >= %d hit a wall" % (row, hit[idle:].sum(), N - idle, idle)
            if (row[0], "none") + row[2:] in costs:
                assert differ(costs[row], costs[(row[0], "none") + row[2:]])[idle:].any(), what + "%s: the walls cost the idle lanes' rollouts nothing" % (row,)
            if W > 64:
                assert masks[:, :, :64].any() and masks[:, :, 64:].any(), what + "%s: a wall tile is not hit" % (row,)
            assert masks.sum(axis=2).max() >= 2, what + "%s: no (rollout, step) has two wall hits" % (row,)
        # discs: hit at all, and of the second tile
        discs, rad, _, _, _ = fc.model_args(sc, FULL)
        st = wall_model.states(plain(sc), sc["noise"][b], sc["u"][b])
        disc_masks = cm.level_masks(st, [0.0], discs, rad, None, None)[0][0]
        assert disc_masks.sum(axis=2).max() >= 2, what + "no (rollout, step) has two disc hits"
        if K > 64:
            assert disc_masks[:, :, 64:].any(), what + "no disc of the second tile is hit"
        # the rings, the body, the goal track's rows, the samples
        for row in fc.EXTRA_ROWS:
            discs, rad, seg, hw, kw = fc.model_args(sc, row)
            for feature, says in (("rings", "the rings cost nothing"), ("footprint", "the body changes nothing against the point robot")):
                if kw[feature] is not None:
                    without = form_model.costs(fc.oracle_of(sc, row), discs, rad, seg, hw, sc["noise"][b], sc["u"][b], **dict(kw, **{feature: None}))
                    assert differ(costs[row], without).any(), what + "%s: %s" % (row, says)
        for row in [r for r in fc.ROWS if r[2]]:
            still = form_model.costs(fc.oracle_of(sc, row), *fc.model_args(sc, row)[:4], sc["noise"][b], sc["u"][b],
                                     **dict(fc.model_args(sc, row)[4], goal_track=sc["goal_track"][:1]))
            assert differ(costs[row], still).any(), what + "%s: the goal's rows cannot be told apart" % (row,)
        for row in [r for r in fc.ROWS if "samples" in r[3]]:
            per = fc.model(K, W, wscale, row, b)[1]
            assert per.shape == (N, S)
            assert (np.ptp(per, axis=1) > 0).any(), what + "%s: every rollout costs the same under every sample" % (row,)
            assert (np.diff(per, axis=1) > 0).any(), what + "%s: the descending order is the sample order" % (row,)
            assert differ(costs[row], disc_samples_model.cvar_tail(per, 1.0)).any(), what + "%s: the CVaR is the mean" % (row,)
        # the offset: every row that holds something that moves costs otherwise at offset 3
        for row in fc.ROWS:
            moved = differ(fc.model(K, W, wscale, row, b, OFFSETS[1])[0], costs[row]).any()
            assert moved == fc.moves(row), what + "%s: offset %d changes %s" % (row, OFFSETS[1], "something" if moved else "nothing")
    for row in fc.ROWS:
        assert differ(fc.model(K, W, wscale, row, 0)[0], fc.model(K, W, wscale, row, 1)[0]).any(), "problem 1 is a copy of problem 0"


def test_the_recorded_miscount_lies_in_the_sweep():
    """The form of the recorded miscount -- exact, no rotation, batched, CrowdWallTracks + CrowdFootprint, ten walls in one
    tile, lanes 10 to 63 idle: in both problems of that row every one of the 54 rollouts in those lanes hits a wall (the
    thick walls lie across the diagonal every rollout sets out along), before its freeze, so that the hit shows in its cost.
    A kernel that hands those lanes a stale value there cannot equal the model."""
    K, W, wscale = 7, 10, 1.5
    sc = fc.scene(K, W, wscale)
    row = ("tracks", "tracks", False, ("footprint",), False)
    assert row in fc.ROWS and fc.form_of(row) == (True, "tracks", False, False, False, True)
    for b in range(fc.B):
        hit = walled_lanes(sc, row, b).any(axis=(1, 2))
        print("problem %d: %d of the %d rollouts in lanes %d to 63 hit a wall" % (b, hit[W:].sum(), N - W, W))
        assert hit[W:].all()
        free = form_model.costs(fc.oracle_of(sc, row), sc["tracks"], sc["rad"], None, None, sc["noise"][b], sc["u"][b], footprint=BODY)
        assert differ(fc.model(K, W, wscale, row, b)[0], free)[W:].all()


@pytest.mark.parametrize("wscale", fc.WSCALES)
def test_the_mixed_batch_means_something(wscale):
    """Every problem's costs are its own: those of its own sets, not of a neighbour's."""
    for row in fc.MIXED_ROWS:
        costs = [fc.mixed_model(wscale, row, b) for b in range(3)]
        for b in range(3):
            assert len(np.unique(costs[b])) > N // 2
        sc = fc.scene(70, 74, wscale)
        u, noise = fc.mixed_inputs(wscale)
        for b, other in ((0, 1), (1, 0), (2, 0)):  # problem b with another problem's discs and walls: other costs
            discs, rad, seg, hw, kw = fc.model_args(sc, row, fc.MIXED_DISCS[other], fc.MIXED_WALLS[other])
            swapped = form_model.costs(fc.oracle_of(sc, row), discs, rad, seg, hw, noise[b], u[b], offset=fc.MIXED_OFFSETS[b], **kw)
            assert differ(costs[b], swapped).any(), "bad input: %s, problem %d costs the same with the sets of problem %d" % (row, b, other)
