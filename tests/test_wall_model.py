"""CPU checks of the wall obstacles' model (tests/wall_model.py; the arithmetic of k_rollout_barebone_crowd<..., WALLS>):
its float64 verdicts against the same formula in exact rational arithmetic and against a dense-sampling distance between
the two segments, the zero-wall case against crowd_model, and barebone.polyline_walls."""
import os
import re
from fractions import Fraction

import numpy as np
import pytest

from crowd_model import crowd_costs
from test_crowd_model import _problem, _same_bits
from track_model import oracle_params
from wall_model import hit, wall_costs, wall_hits

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HALFWIDTHS = (0.0, 0.05, 0.3)


def _near_exact(wx, wy, ux, uy, LL, hh):
    s = wx * ux + wy * uy
    if s <= 0:
        return wx * wx + wy * wy <= hh
    if s >= LL:
        vx, vy = wx - ux, wy - uy
        return vx * vx + vy * vy <= hh
    c = wx * uy - wy * ux
    return c * c <= hh * LL


def hit_exact(P, Q, A, B, h):
    """wall_model.hit in fractions.Fraction on the float32 inputs as they are: no rounding anywhere."""
    px, py, qx, qy, ax, ay, bx, by, h = (Fraction(float(v)) for v in (*P, *Q, *A, *B, h))
    dx, dy, ex, ey = bx - ax, by - ay, qx - px, qy - py
    hh, LLd, LLe = h * h, dx * dx + dy * dy, ex * ex + ey * ey
    pax, pay, qax, qay = px - ax, py - ay, qx - ax, qy - ay
    apx, apy, bpx, bpy = ax - px, ay - py, bx - px, by - py
    o1, o2 = dx * pay - dy * pax, dx * qay - dy * qax
    o3, o4 = ex * apy - ey * apx, ex * bpy - ey * bpx
    crossing = ((o1 > 0 and o2 < 0) or (o1 < 0 and o2 > 0)) and ((o3 > 0 and o4 < 0) or (o3 < 0 and o4 > 0))
    return bool(crossing or _near_exact(pax, pay, dx, dy, LLd, hh) or _near_exact(qax, qay, dx, dy, LLd, hh) or
                _near_exact(apx, apy, ex, ey, LLe, hh) or _near_exact(bpx, bpy, ex, ey, LLe, hh))


def random_cases(rng, count, lattice):
    """(P, Q, A, B, h) float32.  lattice: coordinates on multiples of 1/8, steps and walls along the lattice too -- plenty
    of touching endpoints, collinear and degenerate segments, distances that equal h exactly; else continuous."""
    if lattice:
        P, A = (rng.integers(-12, 13, (count, 2)) / 8.0 for _ in range(2))
        Q, B = P + rng.integers(-2, 3, (count, 2)) / 8.0, A + rng.integers(-8, 9, (count, 2)) / 8.0
    else:
        A, P = rng.uniform(-1.5, 1.5, (count, 2)), rng.uniform(-1.5, 1.5, (count, 2))
        B = A + rng.uniform(-1.0, 1.0, (count, 2))
        Q = P + rng.uniform(-0.18, 0.18, (count, 2))
    h = rng.choice(HALFWIDTHS, count)
    return tuple(np.asarray(v, np.float32) for v in (P, Q, A, B, h))


def test_model_equals_exact_arithmetic():
    rng = np.random.default_rng(2024)
    total = 0
    for lattice in (True, False):
        P, Q, A, B, h = random_cases(rng, 10000, lattice)
        got = hit(P, Q, A, B, h)
        want = np.array([hit_exact(P[i], Q[i], A[i], B[i], h[i]) for i in range(len(h))])
        assert (got == want).all(), "lattice %d: %d verdicts differ" % (lattice, (got != want).sum())
        for hw in HALFWIDTHS:  # both verdicts occur at every half-width: the cases mean something
            sel = h == np.float32(hw)
            assert got[sel].any() and not got[sel].all(), (lattice, hw)
        total += len(h)
    assert total >= 20000


def sampled_distance(P, Q, A, B, m):
    """Smallest distance between m points on PQ and m points on AB, (count,) float64."""
    s = np.linspace(0.0, 1.0, m)
    out = np.empty(len(P))
    for i0 in range(0, len(P), 64):
        sl = slice(i0, i0 + 64)
        p, q, a, b = (v[sl].astype(np.float64) for v in (P, Q, A, B))
        X = p[:, None, :] + s[None, :, None] * (q - p)[:, None, :]   # (c, m, 2)
        Y = a[:, None, :] + s[None, :, None] * (b - a)[:, None, :]
        d2 = ((X[:, :, None, :] - Y[:, None, :, :]) ** 2).sum(axis=3)
        out[sl] = np.sqrt(d2.reshape(len(p), -1).min(axis=1))
    return out


def test_model_equals_geometry():
    """The closest pair of points is within half a sample spacing of a sampled pair on either segment, so the sampled
    distance exceeds the true one by at most (|PQ| + |AB|) / (2 (m - 1)): outside that band around h the verdicts must agree."""
    rng = np.random.default_rng(7)
    m = 256
    P, Q, A, B, h = random_cases(rng, 3000, lattice=False)
    got = hit(P, Q, A, B, h)
    dist = sampled_distance(P, Q, A, B, m)
    length = np.linalg.norm((Q - P).astype(np.float64), axis=1) + np.linalg.norm((B - A).astype(np.float64), axis=1)
    resolution = length / (2 * (m - 1)) + 1e-9
    clear = np.abs(dist - h.astype(np.float64)) > resolution
    share = 1.0 - clear.mean()
    print("dense sampling: %.2f %% of %d cases inside the resolution band, %d hits" % (100 * share, len(h), got.sum()))
    assert share <= 0.02, "bad input: %.1f %% of the cases are inside the sampling resolution" % (100 * share)
    want = dist <= h.astype(np.float64)
    assert (got[clear] == want[clear]).all(), "%d verdicts differ from the geometry" % (got[clear] != want[clear]).sum()
    assert got[clear].any() and not got[clear].all()


@pytest.mark.parametrize("T,K", [(30, 5), (37, 70), (37, 0)])
def test_zero_walls_equal_the_crowd_model(T, K):
    from mppi_numba_amd.barebone import constant_velocity_tracks
    rng, params, pos, rad, u, noise = _problem(T, K, 1.0)
    p = oracle_params(params)
    none, no_hw = np.zeros((0, 2, 2), np.float32), np.zeros(0, np.float32)
    assert wall_hits(p, none, no_hw, noise, u).shape == noise.shape[:2]
    static = np.repeat(pos[:, None, :], 1, axis=1)
    moving = constant_velocity_tracks(pos, rng.normal(0, 0.3, (K, 2)), 0.1, T + 1)
    for tracks, offset in ((static, 0), (moving, 0), (moving, 7)):
        got = wall_costs(p, tracks, rad, none, no_hw, noise, u, offset=offset)
        assert _same_bits(got, crowd_costs(p, tracks, rad, noise, u, offset=offset)), (T, K, offset)


def test_polyline_walls():
    from mppi_numba_amd.barebone import polyline_walls
    pts = [[0, 0], [4, 0], [4, 3], [0.1, 3]]
    open_ = polyline_walls(pts)
    assert open_.dtype == np.float32 and open_.shape == (3, 2, 2) and open_.flags["C_CONTIGUOUS"]
    np.testing.assert_array_equal(open_[:, 0], np.float32(pts[:-1]))
    np.testing.assert_array_equal(open_[:, 1], np.float32(pts[1:]))
    closed = polyline_walls(np.array(pts, dtype=np.float64), closed=True)
    assert closed.dtype == np.float32 and closed.shape == (4, 2, 2)
    np.testing.assert_array_equal(closed[:3], open_)
    np.testing.assert_array_equal(closed[3], np.float32([pts[3], pts[0]]))
    assert polyline_walls([[1.0, 2.0]]).shape == (0, 2, 2) and polyline_walls([[1.0, 2.0]]).dtype == np.float32
    assert polyline_walls([[1.0, 2.0]], closed=True).shape == (0, 2, 2)
    assert polyline_walls(np.zeros((0, 2))).shape == (0, 2, 2)
    assert polyline_walls([[0, 0], [1, 1]], closed=True).shape == (1, 2, 2)  # (two points close nothing)


def test_header_declares_and_binding_covers_set_walls():
    from mppi_numba_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mppi_hip.h")).read(), flags=re.S)
    found = re.search(r"\bint\s+mppi_planner_set_walls\s*\(([^)]*)\)", text)
    assert found, "include/mppi_hip.h does not declare mppi_planner_set_walls"
    assert len(found.group(1).split(",")) == 4
    assert len(_lib.SIGNATURES["mppi_planner_set_walls"]) == 4
    assert hasattr(_lib.load(), "mppi_planner_set_walls"), "libmppi_hip.so does not export mppi_planner_set_walls"
