"""tests/philox_model.py against things that do not share its code: the Random123 known answers, a scalar Philox in
Python integers with a per-cell loop of draw_bin's rule (csrc/rng_kernels.h), a scalar emulation of the byte-parallel
arithmetic of load_packed_thresholds / draw_packed_pair, and the distributions the draws must follow.  No GPU: the
kernels are held to the model in tests/test_gpu_philox_exact.py."""
import math

import numpy as np
import pytest

import philox_model as M


# ---- the block function ---------------------------------------------------------------------------------------------
def philox_scalar(counter, key):
    """Philox4x32-10 on Python integers"""
    c, k = list(counter), list(key)
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c[0], 0xCD9E8D57 * c[2]
        c = [(p1 >> 32) ^ c[1] ^ k[0], p1 & 0xFFFFFFFF, (p0 >> 32) ^ c[3] ^ k[1], p0 & 0xFFFFFFFF]
        k = [(k[0] + 0x9E3779B9) & 0xFFFFFFFF, (k[1] + 0xBB67AE85) & 0xFFFFFFFF]
    return c


@pytest.mark.parametrize("counter,key,want", [
    ([0, 0, 0, 0], [0, 0], [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]),
    ([0xFFFFFFFF] * 4, [0xFFFFFFFF] * 2, [0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd]),
])
def test_random123_known_answers(counter, key, want):
    got = M.philox4x32_10([np.uint64(w) for w in counter], [np.uint64(w) for w in key])
    assert [int(w) for w in got] == want
    assert philox_scalar(counter, key) == want


def test_vectorised_block_equals_the_scalar_one():
    rng = np.random.default_rng(5)
    c = rng.integers(0, 2 ** 32, size=(4, 50), dtype=np.uint64)
    k = rng.integers(0, 2 ** 32, size=2, dtype=np.uint64)
    got = M.philox4x32_10(list(c), list(k))
    for i in range(c.shape[1]):
        assert [int(w[i]) for w in got] == philox_scalar([int(v) for v in c[:, i]], [int(v) for v in k])


# ---- the map draws: a per-cell loop ----------------------------------------------------------------------------------
def int8(v):
    return (int(v) + 128) % 256 - 128


def f32_uniform_scalar(x):
    return float(np.float32((float(np.float32(x)) + 1.0) * 2.0 ** -32))


def draw_bin(column, table, target):
    cum = 0
    for b, mass in enumerate(column):
        cum = int8(cum + int(mass))
        if target <= cum:
            return int(table[b])
    return int(table[len(column) - 1])


def loop_sample_grids(pmf, table, seed, epoch, alpha_dyn, G, first_sample=0):
    bins, rows, cols = pmf.shape
    groups = (cols + 3) // 4
    key = [seed & 0xFFFFFFFF, seed >> 32]
    out = np.zeros((G, rows, cols), dtype=np.int8)
    for g in range(G):
        for r in range(rows):
            for c in range(cols):
                cg, k = divmod(c, 4)
                if bins <= 64:
                    index = ((first_sample + g) >> 1) * rows * groups + r * groups + cg
                else:
                    index = (first_sample + g) * rows * groups + r * groups + cg
                word = philox_scalar([epoch & 0xFFFFFFFF, epoch >> 32, index & 0xFFFFFFFF, index >> 32], key)[k]
                if bins <= 64:
                    h = (word >> 16) if (g & 1) else (word & 0xFFFF)
                    target = int8(math.ceil((h + 1) / 65536 * 100 * alpha_dyn))
                else:
                    target = int8(math.ceil(f32_uniform_scalar(word) * 100 * alpha_dyn))
                assert target >= 1  # (alpha_dyn in (0, 1]: "0 <= cum" of the model's rule is then implied by target <= cum)
                out[g, r, c] = draw_bin(pmf[:, r, c], table, target)
    return out


def random_pmf(rng, bins, rows, cols, total=100):
    """every cell its own PMF of sum `total`, with empty bins"""
    raw = rng.dirichlet(np.full(bins, 0.4), size=(rows, cols))
    p = np.floor(raw * total).astype(np.int64)
    p[..., int(rng.integers(bins))] += total - p.sum(axis=-1)
    return np.ascontiguousarray(np.moveaxis(p, -1, 0)).astype(np.uint8).astype(np.int8)


LOOP_CASES = [
    # bins, rows, cols, G, first_sample, column sum, alpha_dyn
    (5, 3, 7, 5, 0, 100, 1.0),
    (8, 2, 5, 3, 4, 100, 0.5),
    (12, 2, 4, 2, 0, 200, 1.0),   # wrapped: the running sum passes 127
    (7, 2, 6, 4, 2, 300, 1.0),    # ... and 255
    (6, 3, 3, 3, 0, 60, 1.0),     # short: targets above the sum take the last bin's value
    (1, 2, 5, 2, 0, 100, 1.0),
    (65, 2, 7, 3, 0, 100, 1.0),   # the generic sampler's counters and float32 uniforms
    (70, 2, 5, 2, 2, 180, 0.07),
]


@pytest.mark.parametrize("bins,rows,cols,G,first,total,alpha", LOOP_CASES)
def test_model_equals_a_per_cell_loop(bins, rows, cols, G, first, total, alpha):
    rng = np.random.default_rng(bins * 1000 + cols)
    pmf = random_pmf(rng, bins, rows, cols, total)
    pmf[0, 0, 0] = np.int8(-3)  # a negative entry
    table = rng.integers(-128, 128, size=bins).astype(np.int8)
    for seed, epoch in ((1, 0), (0xFEDCBA9876543210, 3), (7, 0x1_0000_0002)):
        want = loop_sample_grids(pmf, table, seed, epoch, alpha, G, first)
        got = M.sample_grids(pmf, table, seed, epoch, alpha, G, first_sample=first)
        assert got.dtype == np.int8 and np.array_equal(got, want)


def test_a_shard_is_a_slice_of_the_unsharded_draws():
    rng = np.random.default_rng(11)
    for bins in (8, 65):
        pmf, table = random_pmf(rng, bins, 3, 6), np.arange(bins, dtype=np.int8)
        full = M.sample_grids(pmf, table, 1, 2, 1.0, 12)
        for first, G in ((2, 5), (6, 6)):
            assert np.array_equal(M.sample_grids(pmf, table, 1, 2, 1.0, G, first_sample=first), full[first:first + G])


# ---- the byte-parallel arithmetic of the columns kernel, emulated word for word ---------------------------------------
def packed_group(pmf, table, r, cg, targets0, targets1, maxb):
    """load_packed_thresholds + draw_packed_pair (csrc/rng_kernels.h) for one group of 4 cells and one pair of target words;
    32-bit unsigned arithmetic on Python integers"""
    bins, rows, cols = pmf.shape
    u32 = 0xFFFFFFFF
    mass = [0] * maxb
    for b in range(bins):
        for k in range(4):
            mass[b] |= (int(pmf[b, r, min(cg * 4 + k, cols - 1)]) & 0xFF) << (8 * k)
    run, cum, val = 0, [0] * maxb, [0] * maxb
    for b in range(maxb):
        run = (((run & 0x7f7f7f7f) + (mass[b] & 0x7f7f7f7f)) ^ ((run ^ mass[b]) & 0x80808080)) & u32
        negative = ((run & 0x80808080) >> 7) * 255
        cum[b] = ((run & ~negative & u32) if b < bins else 0) | 0x80808080
        val[b] = ((int(table[b]) & 0xFF) * 0x01010101) if b < bins else 0
    last = (int(table[bins - 1]) & 0xFF) * 0x01010101
    picked = []
    for targets in (targets0, targets1):
        word = 0
        for k in range(4):
            word |= min(max(int(targets[k]), 0), 127) << (8 * k)
        p = last
        for b in range(maxb - 1, -1, -1):
            if b < bins:
                hit = ((((cum[b] - word) & u32) & 0x80808080) >> 7) * 255
                p = (val[b] & hit) | (p & ~hit & u32)
        picked.append([int8((p >> (8 * k)) & 0xFF) for k in range(4)])
    return picked


@pytest.mark.parametrize("bins,total", [(1, 100), (5, 100), (8, 127), (9, 200), (16, 300), (17, 60), (33, 255), (64, 100)])
def test_packed_arithmetic_follows_draw_bins_rule(bins, total):
    """Every target 1..100 against neighbouring cells whose columns differ: a carry or a borrow that crossed from one
    packed byte into the next would move a neighbour's bin."""
    rng = np.random.default_rng(bins)
    rows, cols = 2, 7
    pmf = random_pmf(rng, bins, rows, cols, total)
    if bins > 1:
        pmf[:, 0, 0], pmf[:, 0, 1] = 0, 0
        pmf[-1, 0, 0], pmf[0, 0, 1] = 100, 100  # all mass in the last bin next to all mass in bin 0
        pmf[1, 1, 2] = np.int8(-5)
    table = rng.integers(-128, 128, size=bins).astype(np.int8)
    maxb = 8 if bins <= 8 else 16 if bins <= 16 else 32 if bins <= 32 else 64
    for r in range(rows):
        for cg in range(2):
            for t in range(1, 101):
                t0 = [t, 101 - t, (t * 7) % 100 + 1, (t * 13) % 100 + 1]
                t1 = t0[::-1]
                got = packed_group(pmf, table, r, cg, t0, t1, maxb)
                for targets, have in zip((t0, t1), got):
                    for k in range(4):
                        c = cg * 4 + k
                        if c < cols:
                            assert have[k] == draw_bin(pmf[:, r, c], table, targets[k]), (r, c, targets[k])


# ---- distributions ---------------------------------------------------------------------------------------------------
def test_model_frequencies_follow_the_pmf():
    """the same PMF in every cell, as tests/test_gpu_scale.py test_tdm_philox_sampling_follows_the_pmf draws it, and its
    5 sigma bound (worst-case variance 0.25 per draw)"""
    mass = np.array([10, 20, 40, 25, 5], dtype=np.int8)
    rows, cols, G = 30, 41, 4
    pmf = np.broadcast_to(mass.reshape(-1, 1, 1), (5, rows, cols)).copy()
    table = np.array([0, 25, 50, 75, 100], dtype=np.int8)
    for bins_pad in (0, 60):  # the generic sampler: the same PMF padded with empty bins
        p = np.concatenate([pmf, np.zeros((bins_pad, rows, cols), dtype=np.int8)])
        t = np.concatenate([table, np.full(bins_pad, -1, dtype=np.int8)])
        got = M.sample_grids(p, t, 1, 0, 1.0, G)
        freq = np.array([(got == v).mean() for v in table])
        assert np.abs(freq - mass / 100.0).max() < 5 * np.sqrt(0.25 / got.size)
        low = M.sample_grids(p, t, 1, 1, 0.3, G)
        assert set(np.unique(low)) <= {0, 25}
        assert abs((low == 0).mean() - 10.0 / 30.0) < 5 * np.sqrt(0.25 / low.size)


def test_model_noise_statistics():
    n, T = 4096, 8
    z, u, turn = M.noise(1, 0, 0, n, T, (1.0, 1.0))
    assert z.shape == (n, T, 2) and u.dtype == np.float32 and turn.shape == (n, T)
    assert (u > 0).all() and (u <= 1).all() and (turn > 0).all() and (turn <= 1).all()
    count = n * T
    for c in range(2):
        v = z[..., c]
        assert abs(v.mean()) < 5.0 / np.sqrt(count)
        assert abs(v.std() - 1.0) < 5.0 / np.sqrt(2 * count)
        lag1 = np.corrcoef(v[:, :-1].ravel(), v[:, 1:].ravel())[0, 1]  # steps 2k and 2k + 1 share a block
        assert abs(lag1) < 5.0 / np.sqrt(n * (T - 1))
    assert abs(np.corrcoef(z[..., 0].ravel(), z[..., 1].ravel())[0, 1]) < 5.0 / np.sqrt(count)
    # an odd horizon drops the last step of the last block; a shard is a slice; the scale is per channel
    odd, _, _ = M.noise(1, 0, 0, 70, 7, (1.0, 1.0))
    assert np.array_equal(odd, z[:70, :7])  # ceil(7 / 2) = 8 / 2 step pairs: the same counters
    part, _, _ = M.noise(1, 0, 100, 50, T, (2.0, 4.0))  # (powers of two: the scaling is exact)
    assert np.array_equal(part, z[100:150] * np.array([2.0, 4.0]))
    other, _, _ = M.noise(1, 1, 0, n, T, (1.0, 1.0))
    assert abs(np.corrcoef(z.ravel(), other.ravel())[0, 1]) < 5.0 / np.sqrt(2 * count)
