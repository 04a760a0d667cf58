"""CPU checks of the body footprint's model (tests/footprint_model.py) and of the helpers of mppi_numba_amd.barebone:
the equalities the definition promises, bit for bit; the body's wall test against exact rational arithmetic; the rectangle
cover; and the two statements about the GPU tests' inputs -- they are robust (no centre changes when sine and cosine move by
1e-15, five times what a device's sincos may differ from libm's: the condition under which the GPU comparison may demand
every bit) and they mean something."""
import functools

import numpy as np
import pytest

import footprint_model as fm
from test_gpu_barebone_walls import N, building, discs_of, task, without_walls
from test_wall_model import hit_exact, random_cases
from track_model import oracle_params
from wall_model import active_steps, states, wall_costs

# the eight-row footprint of the GPU comparison: a cover of a 1.2 m x 0.4 m cart, the reference point itself, two discs
# off the axis (one of radius 0) and a bumper
EIGHT = np.float32([[.45, 0, .25], [.15, 0, .25], [-.15, 0, .25], [-.45, 0, .25], [0, 0, 0], [.3, .2, .125], [-.3, -.2, 0], [.6, 0, .05]])
TASKS = ((30, 1.0), (37, 1.5))


def same_bits(a, b):
    return a.shape == b.shape and (a.view(np.int32) == b.view(np.int32)).all()


@functools.lru_cache(maxsize=None)
def scene(t, wscale):
    """The task of test_gpu_barebone_walls with its 65 walls and 70 static discs, and the oracle's states."""
    params, u_in, noise = task(t, wscale)
    p = oracle_params(without_walls(params))
    seg, hw = building(65)
    pos, rad = discs_of(70, "static", t, params)
    st = states(p, noise, u_in)
    st.setflags(write=False)
    return p, u_in, noise, seg, hw, pos[:, None, :], rad, st


def dyadic(v):
    """float32 multiples of 1/64: sums of two of them are exact in float32."""
    return (np.round(np.asarray(v, np.float64) * 64) / 64).astype(np.float32)


@pytest.mark.parametrize("t,wscale", TASKS)
def test_the_point_footprint_is_the_point_model(t, wscale):
    p, u_in, noise, seg, hw, tracks, rad, st = scene(t, wscale)
    want = wall_costs(p, tracks, rad, seg, hw, noise, u_in)
    assert same_bits(fm.costs(p, [[0, 0, 0]], tracks, rad, seg, hw, noise, u_in), want)
    assert (want > 1e6).any() and len(np.unique(want)) > N // 2
    assert same_bits(fm.centres(st, [[0, 0, 0.3]])[..., 0, :], st[..., :2])  # a row (0, 0, rho): the centre is (x, y)


@pytest.mark.parametrize("t,wscale", TASKS)
def test_a_centred_disc_is_the_point_model_with_larger_obstacles(t, wscale):
    p, u_in, noise, seg, hw, tracks, rad, st = scene(t, wscale)
    rad, hw, rho = dyadic(rad), dyadic(hw), np.float32(5.0 / 64)
    want = wall_costs(p, tracks, rad + rho, seg, hw + rho, noise, u_in)
    assert ((rad + rho).astype(np.float64) == rad.astype(np.float64) + np.float64(rho)).all()
    got = fm.costs(p, [[0, 0, rho]], tracks, rad, seg, hw, noise, u_in)
    assert same_bits(got, want)
    assert not same_bits(got, wall_costs(p, tracks, rad, seg, hw, noise, u_in)), "bad input: rho changes nothing"


@pytest.mark.parametrize("t,wscale", TASKS)
def test_a_row_repeated_is_the_row_once(t, wscale):
    p, u_in, noise, seg, hw, tracks, rad, st = scene(t, wscale)
    once = fm.costs(p, EIGHT[[0, 5]], tracks, rad, seg, hw, noise, u_in)
    twice = fm.costs(p, EIGHT[[0, 5, 0, 0, 5]], tracks, rad, seg, hw, noise, u_in)
    assert same_bits(once, twice)


def test_the_bodys_wall_test_equals_exact_arithmetic():
    """The chord of every body disc against a wall of half-width h + rho (the sum exact in double for these values), the
    verdicts OR-ed: the model in double against fractions.Fraction.  Lattice cases (everything exact, plenty of distances
    that equal h + rho) and continuous ones."""
    rng = np.random.default_rng(11)
    fp = np.float32([[0.25, 0, 0.125], [-0.25, 0.125, 0.0], [0, -0.25, 0.3]])
    total = 0
    for lattice in (True, False):
        count = 300
        P, Q, A, B, h = random_cases(rng, count, lattice)
        th = rng.integers(-4, 5, (count, 2)) * (np.pi / 4) if lattice else rng.uniform(-np.pi, np.pi, (count, 2))
        pre = fm.centres(np.concatenate([P, th[:, :1]], axis=1), fp)   # (count, F, 2)
        post = fm.centres(np.concatenate([Q, th[:, 1:]], axis=1), fp)
        each = fm.hit(pre, post, A[:, None], B[:, None], h[:, None], fp[None, :, 2])  # (count, F)
        want = np.array([[hit_exact(pre[i, f], post[i, f], A[i], B[i], float(h[i]) + float(fp[f, 2])) for f in range(len(fp))]
                         for i in range(count)])
        assert (each == want).all(), "lattice %d: %d verdicts differ" % (lattice, (each != want).sum())
        body = each.any(axis=1)
        assert body.any() and not body.all() and (each.sum(axis=1) == 1).any(), lattice
        total += count
    assert total >= 600


@pytest.mark.parametrize("front,rear,width,count", [(0.5, 0.5, 0.4, None), (0.8, 0.2, 0.3, 8), (0.3, 0.1, 0.6, None), (1.0, 1.0, 0.1, None)])
def test_rectangle_footprint_covers_its_rectangle(front, rear, width, count):
    from mppi_numba_amd.barebone import rectangle_footprint
    fp = rectangle_footprint(front, rear, width, count)
    length = front + rear
    F = count if count is not None else min(max(int(np.ceil(length / width)), 1), 8)
    assert fp.dtype == np.float32 and fp.shape == (F, 3) and fp.flags["C_CONTIGUOUS"]
    want = np.zeros((F, 3))
    want[:, 0] = -rear + (np.arange(F) + 0.5) * length / F
    want[:, 2] = np.sqrt((length / (2 * F)) ** 2 + (width / 2) ** 2)
    np.testing.assert_array_equal(fp, want.astype(np.float32))
    # dense sampling, the border included; 1e-6 m: the float32 rounding of centres and radii of about a metre is below 1e-7
    xs, ys = np.meshgrid(np.linspace(-rear, front, 401), np.linspace(-width / 2, width / 2, 201))
    pts = np.stack([xs.ravel(), ys.ravel()], axis=1)
    d = np.linalg.norm(pts[:, None, :] - fp[None, :, :2].astype(np.float64), axis=2) - fp[None, :, 2].astype(np.float64)
    assert d.min(axis=1).max() <= 1e-6
    # ... and no wider than it must be: the corners of the pieces lie ON the circles
    corner = np.array([-rear, width / 2])
    assert abs(np.linalg.norm(corner - fp[0, :2]) - fp[0, 2]) <= 1e-6


def test_rectangle_footprint_refuses_nonsense():
    from mppi_numba_amd.barebone import rectangle_footprint
    for args in ((0.5, 0.5, 0.4, 9), (0.5, 0.5, 0.4, 0), (0.0, 0.0, 0.4, None), (0.5, 0.5, -0.1, None), (np.nan, 0.5, 0.4, None)):
        with pytest.raises(ValueError):
            rectangle_footprint(*args)
    assert rectangle_footprint(2.0, 2.0, 0.1).shape == (8, 3)  # (clipped)


def test_body_discs_equal_the_models_centres():
    from mppi_numba_amd.barebone import body_discs
    st = scene(37, 1.5)[7]
    got = body_discs(st, EIGHT)
    assert got.dtype == np.float32 and got.shape == st.shape[:2] + (8, 2)
    assert same_bits(got, fm.centres(st, EIGHT))
    assert same_bits(body_discs(st[3, 5].astype(np.float64), EIGHT[:3]), fm.centres(st[3, 5], EIGHT[:3]))
    for bad in (np.zeros((9, 3)), np.zeros((0, 3)), np.zeros((3, 2)), np.zeros(3)):
        with pytest.raises(ValueError):
            body_discs(st, bad)


@pytest.mark.parametrize("t,wscale,values", [(30, 1.0, 99200), (37, 1.5, 121600)])
def test_the_inputs_are_robust(t, wscale, values):
    """Sine and cosine moved by +-1e-15, all four sign pairs: no centre of the GPU comparison's inputs changes.  (The device's
    sincos_f64 is within 2e-16 of libm's; the rounding to float32 hides that unless a sum lies within it of a rounding
    boundary -- none of these does, with a factor of five to spare.)"""
    st = scene(t, wscale)[7]
    base = fm.centres(st, EIGHT)
    assert base.size == values
    for ds in (-1e-15, 1e-15):
        for dc in (-1e-15, 1e-15):
            moved = fm.centres(st, EIGHT, ds, dc)
            assert (moved.view(np.int32) != base.view(np.int32)).sum() == 0, (ds, dc)


@pytest.mark.parametrize("t,wscale", TASKS)
def test_the_inputs_mean_something(t, wscale):
    p, u_in, noise, seg, hw, tracks, rad, st = scene(t, wscale)
    assert st.shape == (N, t + 1, 3)
    ctr = fm.centres(st, EIGHT)
    d_each = fm.disc_touches(ctr, EIGHT, tracks, rad)   # (n, T, F, K)
    w_each = fm.wall_touches(ctr, EIGHT, seg, hw)       # (n, T, F, W)
    body = d_each.any(axis=2).sum(axis=2) + w_each.any(axis=2).sum(axis=2)
    point = fm.footprint_hits(st, [[0, 0, 0]], tracks, rad, seg, hw)
    point = point[0] + point[1]
    assert ((body > 0) & (point == 0)).any(), "no (rollout, step) where the body hits and the reference point does not"
    assert (d_each.sum(axis=2) >= 2).any() and (w_each.sum(axis=2) >= 2).any(), "no obstacle touched by two body discs"
    assert body.sum() < d_each.sum() + w_each.sum(), "any, not sum: the rule never matters"
    assert (w_each.any(axis=2) & ~w_each.all(axis=2)).any(), "no wall that one body disc hits and another clears"
    assert (~active_steps(p, st) & (body > 0)).any(), "no hit after the freeze"
    got = fm.costs(p, EIGHT, tracks, rad, seg, hw, noise, u_in)
    assert not same_bits(got, wall_costs(p, tracks, rad, seg, hw, noise, u_in))
