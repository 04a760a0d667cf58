"""CPU checks of the clearance rings' model (tests/clearance_model.py), of clearance_staircase, and of the inputs of the GPU
comparisons (tests/clearance_cases.py): the (num, den) form of the wall test is wall_model.hit at margin 0 and
footprint_model.hit with rho for a margin, and both equal exact rational arithmetic; the counts are monotone; a ring of
penalty 0 leaves the chain's bits; and no disc verdict of the GPU inputs is near enough to its boundary for the kernel's fma
to flip it."""
from fractions import Fraction

import numpy as np
import pytest

import clearance_cases as cases
import clearance_model as cm
import fleet_body_model
import footprint_model
import wall_model
from test_wall_model import hit_exact, random_cases

DYADIC_MARGINS = np.float32([0.0, 0.125, 0.25, 0.5])


def same_bits(a, b):
    return a.shape == b.shape and (a.view(np.int32) == b.view(np.int32)).all()


def degenerate_cases():
    """Zero-length steps, zero-length walls, both, collinear overlapping and disjoint segments, steps that end exactly h from
    a wall and from a wall's end -- dyadic data, so that `exactly` is exact."""
    rows = []
    for h in (0.0, 0.125, 0.25):
        for off in (-0.25, -0.125, 0.0, 0.125, 0.25, 0.375):
            rows += [([0.5, off], [0.5, off], [0, 0], [1, 0], h),          # a zero-length step beside the wall
                     ([1.0 + off, 0], [1.0 + off, 0], [0, 0], [1, 0], h),  # ... and on its line, around its end
                     ([off, 0.25], [off + 0.25, 0.25], [0.5, 0.5], [0.5, 0.5], h),  # a zero-length wall
                     ([off, off], [off, off], [0.25, 0.25], [0.25, 0.25], h),       # both
                     ([off, 0], [off + 0.5, 0], [0, 0], [1, 0], h),                 # collinear, overlapping or touching
                     ([1.5 + off, 0], [2.0 + off, 0], [0, 0], [1, 0], h),           # collinear, apart
                     ([0.25, off], [0.75, off], [0, 0], [1, 0], h),                 # parallel at |off|: touching at exactly h
                     ([0.5, -off], [0.5, off], [0, 0], [1, 0], h),                  # across
                     ([1.0, off], [1.5, off + 0.25], [0, 0], [1, 0], h)]            # from above the wall's end
    P, Q, A, B, h = (np.float32([r[i] for r in rows]) for i in range(5))
    return P, Q, A, B, h


def test_the_parts_form_is_the_wall_test():
    """More than 10^5 random inputs and the degenerate ones: at margin 0 wall_model.hit, with a margin footprint_model.hit
    with rho := the margin (H = h + m in double)."""
    rng = np.random.default_rng(31)
    total = 0
    for lattice, count in ((True, 60000), (False, 60000), (None, 0)):
        P, Q, A, B, h = degenerate_cases() if lattice is None else random_cases(rng, count, lattice)
        parts = cm.wall_parts(P, Q, A, B)
        assert (cm.wall_verdict(parts, h.astype(np.float64)) == wall_model.hit(P, Q, A, B, h)).all(), lattice
        for m in (np.float32(0.125), np.float32(0.1), np.float32(0.37)):
            got = cm.wall_verdict(parts, h.astype(np.float64) + np.float64(m))
            want = footprint_model.hit(P, Q, A, B, h, np.full(len(h), m, np.float32))
            assert (got == want).all(), (lattice, m)
            assert got.any() and not got.all()
        total += len(h)
    assert total >= 100000


def test_the_parts_form_equals_exact_arithmetic():
    """Against fractions.Fraction, as tests/test_wall_model.py holds wall_model.hit: lattice cases (distances that equal the
    half-width exactly), continuous ones and the degenerate ones, at dyadic margins so that h + m is exact."""
    rng = np.random.default_rng(37)
    for lattice in (True, False, None):
        P, Q, A, B, h = degenerate_cases() if lattice is None else random_cases(rng, 1500, lattice)
        parts = cm.wall_parts(P, Q, A, B)
        for m in DYADIC_MARGINS:
            H = h.astype(np.float64) + np.float64(m)
            got = cm.wall_verdict(parts, H)
            want = np.array([hit_exact(P[i], Q[i], A[i], B[i], Fraction(float(H[i]))) for i in range(len(h))])
            assert (got == want).all(), "lattice %s, margin %g: %d verdicts differ" % (lattice, m, (got != want).sum())
    P, Q, A, B, h = degenerate_cases()
    touching = cm.wall_verdict(cm.wall_parts(P, Q, A, B), h.astype(np.float64))
    assert touching.any() and not touching.all()


@pytest.mark.parametrize("t,wscale", cases.TASKS)
def test_level_zero_is_the_existing_models(t, wscale):
    """Margin 0: crowd_model's disc hits + wall_model's wall hits for the point robot, footprint_model's for a body."""
    params, u_in, noise = cases.task(t, wscale)
    _, tracks, rad, seg, hw = cases.scene(70, 65, "static", t, wscale)
    st = cases.states_of(t, wscale)
    p = cases.oracle_params(cases.without_walls(params))
    hits = cm.hit_counts(st, tracks, rad, seg, hw)
    assert same_bits(wall_model.chain(p, hits, st, noise, u_in), wall_model.wall_costs(p, tracks, rad, seg, hw, noise, u_in))
    fp = cases.FOOTPRINTS[3]
    discs, walls = footprint_model.footprint_hits(st, fp, tracks, rad, seg, hw)
    assert (cm.hit_counts(st, tracks, rad, seg, hw, footprint=fp) == discs + walls).all()


@pytest.mark.parametrize("t,wscale", cases.TASKS)
def test_counts_are_monotone_and_a_free_ring_is_free(t, wscale):
    params, u_in, noise = cases.task(t, wscale)
    p = cases.oracle_params(cases.without_walls(params))
    st = cases.states_of(t, wscale)
    _, tracks, rad, seg, hw = cases.scene(70, 65, "tracks", t, wscale)
    for fp in (None, cases.FOOTPRINTS[3]):
        hits = cm.hit_counts(st, tracks, rad, seg, hw, footprint=fp, offset=5)
        near = cm.ring_counts(st, cases.RINGS[4], tracks, rad, seg, hw, footprint=fp, offset=5)
        assert near.shape == (4,) + hits.shape
        assert (near[0] >= hits).all() and (np.diff(near, axis=0) >= 0).all()
        assert (near[0] > hits).any() and all((near[l + 1] > near[l]).any() for l in range(3)), "bad input: a ring that holds nothing new"
        plain = wall_model.chain(p, hits, st, noise, u_in)
        free = cases.RINGS[4].copy()
        free[:, 1] = 0.0
        assert same_bits(cm.chain(p, hits, near, free, st, noise, u_in), plain)
        paid = cm.chain(p, hits, near, cases.RINGS[4], st, noise, u_in)
        assert not same_bits(paid, plain) and (paid >= plain).all()
        # a ring that costs obs_cost is a second copy of the obstacles, m larger: the chain on hits + n_1
        as_hits = np.float32([[cases.RINGS[4][0, 0], p.obs_cost]])
        assert same_bits(cm.chain(p, hits, near[:1], as_hits, st, noise, u_in), wall_model.chain(p, hits + near[0], st, noise, u_in))


def test_clearance_staircase():
    from mppi_numba_amd.barebone import MAX_CLEARANCE_RINGS, clearance_staircase
    assert MAX_CLEARANCE_RINGS == cm.MAX_RINGS == 4
    for reach, peak, count in ((0.5, 2.5e5, 4), (0.3, 100.0, 1), (1.25, 0.0, 3), (0.07, 3.0, 2)):
        rows = clearance_staircase(reach, peak, count)
        assert rows.dtype == np.float32 and rows.shape == (count, 2) and rows.flags["C_CONTIGUOUS"]
        F = [peak * (1.0 - (l - 1.0) / count) ** 2 for l in range(1, count + 2)]
        assert F[-1] == 0.0
        want = np.array([[reach * l / count, F[l - 1] - F[l]] for l in range(1, count + 1)])
        np.testing.assert_array_equal(rows, want.astype(np.float32))
        cm.rows_of(rows)  # (margins ascending and positive, penalties not negative: what the library takes)
        # an obstacle at gap g in (m_{l-1}, m_l] is inside the rings l .. count and pays F_l: on top of peak (1 - g/reach)^2
        for l in range(1, count + 1):
            paid = rows[l - 1:, 1].astype(np.float64).sum()
            assert abs(paid - F[l - 1]) <= 1e-6 * max(peak, 1.0)
            g = reach * l / count
            assert F[l - 1] >= peak * (1.0 - g / reach) ** 2 - 1e-9 * max(peak, 1.0)
    for args in ((0.0, 1.0, 2), (-0.5, 1.0, 2), (0.5, -1.0, 2), (0.5, 1.0, 0), (0.5, 1.0, 5), (np.nan, 1.0, 2), (0.5, np.inf, 2), (0.5, 1.0, 2.5)):
        with pytest.raises(ValueError):
            clearance_staircase(*args)


def test_no_disc_verdict_of_the_gpu_inputs_can_flip():
    """The kernel forms fma(ex, ex, ey * ey), the model ex * ex + ey * ey: they differ by less than 2^-52 (ex^2 + ey^2), under
    1e-12 below 50 m.  Every disc test of every input set the GPU comparisons use, at every ring radius (the hit's
    included), is at least 1e-9 from its boundary."""
    seen = 0
    for label, st, rings, tracks, rad, fp, offset in cases.disc_input_sets():
        assert np.abs(st[..., :2]).max() < 50.0 and np.abs(tracks).max() < 50.0, label
        least = cm.smallest_disc_margin(st, rings, tracks, rad, fp, offset)
        assert least >= 1e-9, "%s: a disc test within %.3g of its boundary -- change the input" % (label, least)
        seen += 1
    assert seen >= 40


def test_the_fleet_inputs_mean_something():
    """The fleet of bodies' case: level 0 is fleet_body_model's count; at some (rollout, step) two DIFFERENT body discs of
    one other robot lie inside a ring while none of its slots is hit, and counting per slot changes the costs."""
    case = cases.body_fleet_case()
    B, F, group, grouped, rings = case["B"], case["F"], case["group"], case["grouped"], case["rings"]
    walls = fleet_body_model.body_walls(case["params"], case["x0s"], case["us"], case["footprint"])
    hw = fleet_body_model.halfwidths(case["footprint"], case["margin"])
    pinned = False
    for a in range(B):
        p, seg, shw = case["readers"][a]
        st = wall_model.states(p, case["noise"][a], case["us"][a])
        hits = cm.hit_counts(st, cases.NO_DISCS[0], cases.NO_DISCS[1], seg, shw, case["footprint"], wall_offset=0, group=group, grouped=grouped)
        want = fleet_body_model.wall_counts(st, case["footprint"], walls[a], hw, cases.ROOM[:case["W"]], cases.ROOM_HW[:case["W"]])
        assert (hits == want).all()
        margins = np.concatenate([[0.0], rings[:, 0].astype(np.float64)])
        masks = cm.level_masks(st, margins, cases.NO_DISCS[0], cases.NO_DISCS[1], seg, shw, case["footprint"], wall_offset=0)[1]
        slots = masks[..., :grouped].reshape(masks.shape[:3] + (B - 1, group))[..., :F]  # (1 + R, n, T, robot, body disc)
        two_near_none_hit = (slots[1:].sum(axis=-1) >= 2) & ~slots[0].any(axis=-1)[None]
        folded = cm.costs(p, rings, *cases.NO_DISCS, seg, shw, case["noise"][a], case["us"][a], case["footprint"], wall_offset=0,
                          group=group, grouped=grouped)
        per_slot = cm.costs(p, rings, *cases.NO_DISCS, seg, shw, case["noise"][a], case["us"][a], case["footprint"], wall_offset=0)
        pinned = pinned or (two_near_none_hit.any() and not same_bits(folded, per_slot))
    assert pinned, "bad input: the fold per ring never matters"
