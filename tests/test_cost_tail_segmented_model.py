"""tests/cost_tail_segmented_model.py against the reference's walk: the same bits on EVERY rollout -- safe ones, ties of
both roundings, binade crossings up, down and both, costs that land exactly on a binade edge, tiny, subnormal, zero and
negative costs -- for horizons on both sides of the piece and group sizes; and the round histogram of C2-like inputs
(printed; recorded in profiles/HISTORY.md), which sets what the kernel's tail may expect."""
import numpy as np
import pytest

from cost_tail_segmented_model import MAX_ROUNDS, c2_like, print_round_shares, round_shares, segmented, walk

f32, f64 = np.float32, np.float64
HORIZONS = [1, 4, 5, 8, 9, 100, 104]


def ulp_of(c0):
    return np.ldexp(1.0, np.frexp(c0.astype(f64))[1].astype(np.int64) - 1 - 23)


def same_bits(got, want):
    return np.array_equal(got.view(np.uint32), want.view(np.uint32))


@pytest.mark.parametrize("t", HORIZONS)
def test_c2_like_costs_have_the_bits_of_the_walk(t):
    rng = np.random.default_rng(100 + t)
    c0, a = c2_like(4_000, t, rng)
    got, rounds = segmented(c0, a)
    assert same_bits(got, walk(c0, a))
    assert rounds.min() >= 1 and rounds.max() <= MAX_ROUNDS


@pytest.mark.parametrize("t", HORIZONS)
def test_forced_ties_of_both_roundings(t):
    rng = np.random.default_rng(200 + t)
    c0, a = c2_like(2_000, t, rng)
    q = ulp_of(c0)
    at = min(t - 1, 6)
    half = len(c0) // 2
    # second rounding (the float32 store): exact odd multiples of half an ulp
    a[:half, at] = (rng.integers(-9, 10, half) + 0.5) * q[:half]
    # first rounding (the float64 sum): odd multiples of half a unit of the sum's grid, on top of whole ulps
    a[half:, at] = (rng.integers(-9, 10, len(c0) - half) * 2.0 ** 29 + rng.integers(-4, 5, len(c0) - half) + 0.5) * (q[half:] * 2.0 ** -29)
    got, rounds = segmented(c0, a)
    assert same_bits(got, walk(c0, a))
    # the tie's piece is walked: another round follows unless the piece was the last one
    if at // 4 < (t - 1) // 4:
        assert rounds.min() >= 2


@pytest.mark.parametrize("t", HORIZONS)
@pytest.mark.parametrize("way", ["up", "down", "up_then_down"])
def test_forced_crossings(t, way):
    rng = np.random.default_rng(300 + t)
    n = 2_000
    _, a = c2_like(n, t, rng)
    edge = np.ldexp(1.0, rng.integers(12, 14, n))
    first, second = 0, min(t - 1, 5)
    if way == "up":
        c0 = (edge - rng.uniform(0.5, 3.0, n)).astype(f32)
        a[:, first] = rng.uniform(4.0, 9.0, n)
    elif way == "down":
        c0 = (edge + rng.uniform(0.5, 3.0, n)).astype(f32)
        a[:, first] = -rng.uniform(4.0, 9.0, n)
    else:
        c0 = (edge - rng.uniform(0.5, 3.0, n)).astype(f32)
        a[:, first] = rng.uniform(4.0, 9.0, n)
        a[:, second] += -rng.uniform(30.0, 40.0, n)
    want = walk(c0, a)
    got, rounds = segmented(c0, a)
    assert same_bits(got, want)
    if t >= 5:      # (more than one piece: the crossing's piece is walked and a round in the new binade follows)
        assert rounds.min() >= 2
    if way == "up_then_down" and t >= 100:
        assert (rounds >= 3).mean() > 0.9   # (first and second lie in pieces 0 and 1)
    # and with fewer rounds than the input needs, the remainder is walked: the same bits again
    for cap in (0, 1, 2):
        assert same_bits(segmented(c0, a, max_rounds=cap)[0], want)


@pytest.mark.parametrize("t", HORIZONS)
def test_costs_that_land_exactly_on_a_binade_edge(t):
    rng = np.random.default_rng(400 + t)
    n = 1_500
    _, a = c2_like(n, t, rng)
    k = rng.integers(12, 14, n)
    edge = np.ldexp(1.0, k)
    q_lo, q_hi = np.ldexp(1.0, k - 24), np.ldexp(1.0, k - 23)      # ulps below / above the edge
    steps = rng.integers(1, 40, n)
    at = min(t - 1, 2)
    third = n // 3
    c0 = np.empty(n, f32)
    c0[:third] = (edge - steps * q_lo)[:third]                     # from below, onto the edge
    a[:third, :at + 1] = 0.0
    a[:third, at] = (steps * q_lo)[:third]
    c0[third:2 * third] = (edge + steps * q_hi)[third:2 * third]   # from above, onto the edge
    a[third:2 * third, :at + 1] = 0.0
    a[third:2 * third, at] = -(steps * q_hi)[third:2 * third]
    c0[2 * third:] = edge[2 * third:]                              # starts on the edge
    want = walk(c0, a)
    if t > at + 1:  # (the construction works: the cost IS the edge behind step `at`)
        assert np.array_equal(walk(c0[:2 * third], a[:2 * third, :at + 1]), edge[:2 * third].astype(f32))
    got, _ = segmented(c0, a)
    assert same_bits(got, want)


@pytest.mark.parametrize("t", HORIZONS)
def test_tiny_subnormal_zero_and_negative_costs(t):
    rng = np.random.default_rng(500 + t)
    n = 1_000
    c0, a = c2_like(n, t, rng)
    # scale-free: the C2-like problem 2^-110 times as large (all costs normal, far below 1) -- the integer form as usual
    s = 2.0 ** -110
    c_small, a_small = (c0.astype(f64) * s).astype(f32), a * s
    got, rounds = segmented(c_small, a_small)
    assert same_bits(got, walk(c_small, a_small)) and rounds.min() >= 1
    assert np.array_equal(rounds, segmented(c0, a)[1])   # ... round for round what the unscaled problem takes
    # down at the subnormals, at zero and below: the walk rule
    for c_start in (np.full(n, 2.0 ** -140, f32), np.zeros(n, f32), -c0, rng.uniform(0.0, 1.0, n).astype(f32)):
        for scale in (2.0 ** -135, 1.0):
            got, rounds = segmented(c_start, a * scale)
            assert same_bits(got, walk(c_start, a * scale))
    # costs that stay below 1 with terms of order 1 turn negative on the way: a round never starts from such a cost
    c_low = rng.uniform(0.0, 1.0, n).astype(f32)
    got, rounds = segmented(np.zeros(n, f32), a)
    assert (rounds == 0).all()
    got, rounds = segmented(-c0, a)
    assert (rounds == 0).all() and same_bits(got, walk(-c0, a))
    assert same_bits(segmented(c_low, a)[0], walk(c_low, a))


def test_the_round_histogram_of_c2_like_inputs():
    """Printed (pytest -s) and recorded in profiles/HISTORY.md: the share of tiles of 32 whose slowest rollout needs
    1, 2, ... rounds.  MAX_ROUNDS is the smallest cap no rollout of 10^6 exceeds (the 10^6 run: print_round_shares();
    ten launches' worth of it here)."""
    rounds = print_round_shares(n=81_920, max_rounds=64)
    shares, top = round_shares(rounds)
    assert top <= MAX_ROUNDS
    assert 0.6 < shares[1] < 0.9          # (test_cost_tail_model.py: a quarter of the tiles holds an unsafe rollout)
    assert shares.get(2, 0.0) > 0.1       # ... for most of them one walked piece is the end of it,
    assert sum(s for r, s in shares.items() if r >= 3) > 0.02   # but not for all: a cost beside an edge keeps crossing it
    per_launch = rounds.reshape(-1, 8192).max(axis=1)
    assert per_launch.min() >= 3          # ... and every launch of 256 tiles holds such a tile
