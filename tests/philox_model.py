"""Host model of the Philox samplers (csrc/rng_kernels.h): which counter block every drawn byte and every noise value
comes from, in plain NumPy.  No project import, no GPU.

The map samplers are integer code behind the Philox block, so `sample_grids` is what k_sample_grids_philox_cols,
k_sample_cellsM_philox (64 bins and fewer) and k_sample_grids_philox (more) must write, byte for byte.  `noise` pins the
counters of noise_row and evaluates Box-Muller in float64: the kernel's hardware log2 / sqrt / sin / cos are compared
to it with a tolerance (tests/test_gpu_philox_exact.py), its uniforms are the model's.

Counter layout (DESIGN.md section 4 has the same table):

    draws                   counter {x, y, z, w}                       key              block serves
    maps, <= 64 bins        {epoch lo, epoch hi, pair lo, pair hi}     {seed lo, hi}    4 columns x samples (2p, 2p + 1)
        pair = (first_sample / 2 + p) * rows * groups + r * groups + cg
    maps, > 64 bins         {epoch lo, epoch hi, sub lo, sub hi}       {seed lo, hi}    4 columns of one sample
        sub = first_sample * rows * groups + (g * rows + r) * groups + cg
    control noise           {epoch lo, epoch hi, sub lo, sub hi}       {seed lo, hi}    steps 2 * (t / 2) and the next
        sub = (n_offset + n) * ceil(T / 2) + t / 2

with groups = ceil(cols / 4): word k of a map block is column 4 * cg + k.
"""
import numpy as np

MASK32 = np.uint64(0xFFFFFFFF)
SHIFT32 = np.uint64(32)


def philox4x32_10(counter_words, key_words):
    """Philox4x32-10 (Salmon et al. 2011).  counter_words: four uint64 arrays (or scalars) holding 32-bit words, key_words:
    two.  Returns the four output words as uint64 arrays, in the order {x, y, z, w} of the kernel's uint4."""
    c = [np.asarray(w, dtype=np.uint64) & MASK32 for w in counter_words]
    k = [np.asarray(w, dtype=np.uint64) & MASK32 for w in key_words]
    c = list(np.broadcast_arrays(*c))
    m0, m1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
    w0, w1 = np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)
    for _ in range(10):
        p0 = m0 * c[0]  # 32 x 32 -> 64 bits: no overflow in uint64
        p1 = m1 * c[2]
        c = [(p1 >> SHIFT32) ^ c[1] ^ k[0], p1 & MASK32, (p0 >> SHIFT32) ^ c[3] ^ k[1], p0 & MASK32]
        k = [(k[0] + w0) & MASK32, (k[1] + w1) & MASK32]
    return c


def _split64(v):
    v = np.asarray(v, dtype=np.uint64)
    return v & MASK32, v >> SHIFT32


def _wrap_int8(v):
    """int64 -> the value an int8 holds after the cast (two's complement wrap)"""
    return ((np.asarray(v, dtype=np.int64) + 128) % 256) - 128


def uniform_f32(words):
    """float32(float32(x) * 2^-32 + 2^-32) with a single rounding, as fmaf does: in float64 the product and the sum of a
    float32 and a power of two are exact (at most 25 significant bits), so the cast to float32 is the only rounding."""
    x = np.asarray(words, dtype=np.uint64).astype(np.float32).astype(np.float64)
    return ((x + 1.0) * 2.0 ** -32).astype(np.float32)


def pick_bins(pmf, table, targets):
    """draw_bin's rule for every cell of `targets` (G, rows, cols): the int8 accumulator over the bins wraps, the result is
    table[b] for the lowest b with 0 <= cum[b] and target <= cum[b], and table[bins - 1] where no bin matches."""
    pmf = np.asarray(pmf, dtype=np.int8)
    table = np.asarray(table, dtype=np.int8)
    bins = pmf.shape[0]
    cum = _wrap_int8(np.cumsum(pmf.astype(np.int64), axis=0))  # (bins, rows, cols)
    out = np.full(targets.shape, table[bins - 1], dtype=np.int8)
    open_ = np.ones(targets.shape, dtype=bool)
    for b in range(bins):
        hit = open_ & (cum[b][None] >= 0) & (targets <= cum[b][None])
        out[hit] = table[b]
        open_ &= ~hit
    return out


def map_targets(shape, seed, epoch, alpha_dyn, G, first_sample=0, bins=1):
    """int64 targets (G, rows, cols) of the sampler that serves `bins` bins"""
    rows, cols = shape
    groups = (cols + 3) // 4
    seed_lo, seed_hi = _split64(np.uint64(seed))
    epoch_lo, epoch_hi = _split64(np.uint64(epoch))
    r = np.arange(rows, dtype=np.uint64)[:, None]
    cg = np.arange(groups, dtype=np.uint64)[None, :]
    cgid = r * np.uint64(groups) + cg  # (rows, groups)
    per_sample = np.uint64(rows * groups)
    targets = np.zeros((G, rows, groups * 4), dtype=np.int64)
    if bins <= 64:
        assert first_sample % 2 == 0
        pairs = (G + 1) // 2
        p = np.arange(pairs, dtype=np.uint64)[:, None, None]
        index = (np.uint64(first_sample >> 1) + p) * per_sample + cgid[None]  # (pairs, rows, groups)
        lo, hi = _split64(index)
        words = philox4x32_10([epoch_lo, epoch_hi, lo, hi], [seed_lo, seed_hi])
        for k, word in enumerate(words):
            for half in range(2):
                h = (word >> np.uint64(16 * half)) & np.uint64(0xFFFF)
                t = _wrap_int8(np.ceil((h.astype(np.float64) + 1.0) / 65536.0 * 100.0 * alpha_dyn).astype(np.int64))
                take = t[:(G - half + 1) // 2]  # an odd G: the last pair's second sample does not exist
                targets[half::2, :, k::4] = take
    else:
        g = np.arange(G, dtype=np.uint64)[:, None, None]
        sub = np.uint64(first_sample) * per_sample + g * per_sample + cgid[None]  # (G, rows, groups)
        lo, hi = _split64(sub)
        words = philox4x32_10([epoch_lo, epoch_hi, lo, hi], [seed_lo, seed_hi])
        for k, word in enumerate(words):
            u = uniform_f32(word).astype(np.float64)
            targets[:, :, k::4] = _wrap_int8(np.ceil(u * 100.0 * alpha_dyn).astype(np.int64))
    return targets[:, :, :cols]


def sample_grids(pmf, table, seed, epoch, alpha_dyn, G, first_sample=0):
    """The (G, rows, cols) int8 grids the Philox map samplers draw from the int8 PMF (bins, rows, cols) at call `epoch`."""
    pmf = np.asarray(pmf, dtype=np.int8)
    assert pmf.ndim == 3 and len(table) == pmf.shape[0]
    targets = map_targets(pmf.shape[1:], seed, epoch, alpha_dyn, G, first_sample, bins=pmf.shape[0])
    return pick_bins(pmf, table, targets)


def noise(seed, epoch, n_offset, n_local, T, std):
    """Control noise of call `epoch` for rollouts [n_offset, n_offset + n_local): (n_local, T, 2) float64, and the float32
    uniforms `u` (radius) and `turn` (angle, in turns) it was formed from, each (n_local, T)."""
    pairs = (T + 1) // 2
    seed_lo, seed_hi = _split64(np.uint64(seed))
    epoch_lo, epoch_hi = _split64(np.uint64(epoch))
    n = np.arange(n_local, dtype=np.uint64)[:, None]
    tp = np.arange(pairs, dtype=np.uint64)[None, :]
    sub = (np.uint64(n_offset) + n) * np.uint64(pairs) + tp  # (n_local, pairs)
    lo, hi = _split64(sub)
    x, y, z, w = philox4x32_10([epoch_lo, epoch_hi, lo, hi], [seed_lo, seed_hi])
    u = np.empty((n_local, 2 * pairs), dtype=np.float32)
    turn = np.empty((n_local, 2 * pairs), dtype=np.float32)
    u[:, 0::2], turn[:, 0::2] = uniform_f32(x), uniform_f32(y)
    u[:, 1::2], turn[:, 1::2] = uniform_f32(z), uniform_f32(w)
    u, turn = u[:, :T], turn[:, :T]
    radius = np.sqrt(-2.0 * np.log(u.astype(np.float64)))
    angle = 2.0 * np.pi * turn.astype(np.float64)
    out = np.stack([float(std[0]) * radius * np.sin(angle), float(std[1]) * radius * np.cos(angle)], axis=-1)
    return out, u, turn
