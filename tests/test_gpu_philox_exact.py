"""The Philox samplers of csrc/rng_kernels.h against tests/philox_model.py.

Maps: k_sample_grids_philox_cols (all four bins forms, both loads, both stores, chunks, shards), k_sample_grids_philox
(beyond 64 bins) and k_sample_cellsM_philox (through the costs of a CVaR solve) are integer code behind the Philox block:
every drawn byte must EQUAL the model's, and no byte outside the map may change.

Noise: noise_row's counters are pinned, its hardware log2 / sqrt / sin / cos are not.  The kernel's value over u_std is
held within 1e-3 of the model's float64 Box-Muller on the same uniforms.  The bound is derived, not measured: a wrong,
duplicated or shifted counter gives an independent normal, whose difference from the right one has standard deviation
sqrt(2), so a single element lies within 1e-3 with probability 6e-4 -- every case below has at least one element that
would have to, the larger ones thousands; the transcendentals act on a radius of at most 6.66 and are nowhere near the
bound.  Measured on an MI355X: at most 5.6e-7 over all noise cases of this file (profiles/HISTORY.md; each test prints
its own figure).
"""
import ctypes as C
import gc

import numpy as np
import pytest

import bench
import philox_model as M
from mppi_numba_amd import _lib

pytestmark = pytest.mark.gpu

BIG_SEED = 0xFEDCBA9876543210
NOISE_BOUND = 1e-3


@pytest.fixture(autouse=True)
def release_the_handles():
    """A planner and its device-array views refer to each other, so a handle lives until the cycle collector runs.  Collect
    when a test ends: the streams of this module's planners do not outlive it."""
    yield
    gc.collect()


# ---- TDM handles, made directly (as terrain.py does) so that every dimension is free --------------------------------
class Tdm(object):
    def __init__(self, G, max_rows, max_cols, seed=1):
        self.G, self.max_rows, self.max_cols = G, max_rows, max_cols
        cfg = _lib.TdmCfg(device=0, num_grids=G, max_rows=max_rows, max_cols=max_cols, thread_dim_x=16, thread_dim_y=16,
                          rng=_lib.RNG_PHILOX, seed=seed)
        self.handle = C.c_void_p()
        _lib.call("mppi_tdm_create", C.byref(cfg), C.byref(self.handle))

    def close(self):
        handle, self.handle = self.handle, None
        if handle:
            _lib.call("mppi_tdm_destroy", handle)

    __del__ = close

    def set_maps(self, pmf, table):
        pmf = np.ascontiguousarray(pmf, dtype=np.int8)
        table = np.ascontiguousarray(table, dtype=np.int8)
        bins, rows, cols = pmf.shape
        masks = np.zeros((rows, cols), dtype=np.int8)
        _lib.call("mppi_tdm_set_maps", self.handle, _lib.ptr(pmf, C.c_int8), bins, rows, cols, _lib.ptr(table, C.c_int8), 0.0, 0.01,
                  _lib.ptr(masks, C.c_int8), _lib.ptr(masks, C.c_int8), None)

    def fill(self, byte):
        full = np.full((self.G, self.max_rows, self.max_cols), byte, dtype=np.int8)
        _lib.call("mppi_tdm_set_sampled_grids", self.handle, _lib.ptr(full, C.c_int8), self.max_rows, self.max_cols)

    def sample(self, alpha_dyn):
        _lib.call("mppi_tdm_sample_grids", self.handle, float(alpha_dyn))

    def grids(self):
        out = np.empty((self.G, self.max_rows, self.max_cols), dtype=np.int8)
        _lib.call("mppi_tdm_get_sampled_grids", self.handle, _lib.ptr(out, C.c_int8))
        return out


def assert_drawn(buffer, want, sentinel):
    """buffer[:, :rows, :cols] is `want` byte for byte, and every other byte of the buffer is still the sentinel"""
    G, rows, cols = want.shape
    assert buffer.dtype == np.int8 and want.dtype == np.int8 and buffer.shape[0] == G
    inner = buffer[:, :rows, :cols]
    if not np.array_equal(inner, want):
        bad = np.argwhere(inner != want)
        g, r, c = bad[0]
        raise AssertionError("%d of %d drawn bytes differ; first at sample %d row %d column %d: %d, the model says %d"
                             % (len(bad), want.size, g, r, c, inner[g, r, c], want[g, r, c]))
    outside = np.ones(buffer.shape, dtype=bool)
    outside[:, :rows, :cols] = False
    if not (buffer[outside] == sentinel).all():
        g, r, c = np.argwhere(outside & (buffer != sentinel))[0]
        raise AssertionError("a byte outside the map changed: sample %d row %d column %d holds %d" % (g, r, c, buffer[g, r, c]))


def unused_byte(table):
    return np.int8(next(v for v in range(-128, 128) if v not in set(int(t) for t in table)))


def not_one_hot(pmf):
    """a PMF whose every cell is one-hot is sampled once and then skipped (tdm_sample_on)"""
    hundred = (pmf == 100).sum(axis=0)
    other = ((pmf != 100) & (pmf != 0)).sum(axis=0)
    return bool(((hundred != 1) | (other != 0)).any())


def draw_and_check(pmf, table, G, alpha_dyn=1.0, seed=1, max_rows=None, max_cols=None, first_sample=0, calls=1):
    """`calls` successive sample_grids of a fresh handle against the model at epochs 0, 1, ...; returns the last buffer
    and the model's grids"""
    bins, rows, cols = pmf.shape
    assert not_one_hot(pmf)
    max_rows = rows + 1 if max_rows is None else max_rows
    max_cols = cols if max_cols is None else max_cols
    sentinel = unused_byte(table)
    tdm = Tdm(G, max_rows, max_cols, seed)
    try:
        tdm.set_maps(pmf, table)
        if first_sample:
            _lib.call("mppi_tdm_set_sample_shard", tdm.handle, first_sample)
        for epoch in range(calls):
            tdm.fill(sentinel)
            tdm.sample(alpha_dyn)
            got = tdm.grids()
            want = M.sample_grids(pmf, table, seed, epoch, alpha_dyn, first_sample + G)[first_sample:]
            assert_drawn(got, want, sentinel)
    finally:
        tdm.close()
    return got, want, sentinel


# ---- PMF contents ------------------------------------------------------------------------------------------------------
def random_pmf(rng, bins, rows, cols, total=100, lead_empty=0):
    """every cell its own PMF of column sum `total` (an int or a (rows, cols) array), with empty bins"""
    total = np.broadcast_to(np.asarray(total, dtype=np.int64), (rows, cols))
    live = bins - lead_empty
    raw = rng.dirichlet(np.full(live, 0.5), size=(rows, cols))
    p = np.minimum(np.floor(raw * total[..., None]).astype(np.int64), 127)
    # the remainder goes to bins that still have room below int8's 127
    for r in range(rows):
        for c in range(cols):
            rest = int(total[r, c] - p[r, c].sum())
            for b in rng.permutation(live):
                add = min(rest, 127 - int(p[r, c, b]))
                p[r, c, b] += add
                rest -= add
            assert rest == 0, "column sum %d does not fit %d int8 bins" % (total[r, c], live)
    p = np.concatenate([np.zeros((rows, cols, lead_empty), dtype=np.int64), p], axis=-1)
    return np.ascontiguousarray(np.moveaxis(p, -1, 0)).astype(np.int8)


def wide_table(rng, bins):
    """values over the whole int8 range, -128, -1, 0 and 127 among them where there is room"""
    table = rng.integers(-128, 128, size=bins).astype(np.int8)
    for i, v in enumerate((-128, -1, 127, 0)[:bins]):
        table[(i * 3) % bins] = v
    return table


ROWS, COLS, G_SMALL = 5, 7, 5
# a defect that moves a cumulative mass by one shows only in a draw whose target is that mass: 200 draws a cell, so that nearly
# every target 1..100 occurs in every cell
G_CONTENTS = 200


def contents(kind, bins=8, rows=ROWS, cols=COLS):
    rng = np.random.default_rng(sum(map(ord, kind)) + bins)
    if kind == "empty_bins":
        pmf = random_pmf(rng, bins, rows, cols, lead_empty=min(2, bins - 1))
        pmf[min(4, bins - 1)] = 0  # (an empty bin in the middle; the columns that lose mass are short)
    elif kind == "extremes":
        # all mass in the last bin next to all mass in bin 0 inside every group of four: a carry or a borrow that crossed a
        # byte border would move the neighbour
        pmf = random_pmf(rng, bins, rows, cols)
        for c in range(cols):
            if c % 4 != 3:  # last bin | bin 0 | last bin | a random column
                pmf[:, :, c] = 0
                pmf[0 if c % 4 == 1 else bins - 1, :, c] = 100
    elif kind == "sum127":
        pmf = random_pmf(rng, bins, rows, cols, 127)
    elif kind == "wrap_to_255":
        pmf = random_pmf(rng, bins, rows, cols, rng.integers(128, 256, size=(rows, cols)))
    elif kind == "wrap_beyond_255":
        pmf = random_pmf(rng, bins, rows, cols, rng.integers(256, min(127 * bins, 700), size=(rows, cols)))
    elif kind == "short":
        pmf = random_pmf(rng, bins, rows, cols, rng.integers(1, 100, size=(rows, cols)))
    elif kind == "negative":
        pmf = random_pmf(rng, bins, rows, cols)
        pmf[1, ::2, 1::3] = -7
        pmf[0, 1, 0] = -128
    else:
        assert kind == "plain"
        pmf = random_pmf(rng, bins, rows, cols)
    return pmf, wide_table(rng, bins)


def padded(pmf, table, bins=65):
    """the same PMF with empty bins behind it: the generic kernel's input"""
    rng = np.random.default_rng(bins)
    extra = bins - pmf.shape[0]
    return (np.concatenate([pmf, np.zeros((extra,) + pmf.shape[1:], dtype=np.int8)]),
            np.concatenate([table, rng.integers(-128, 128, size=extra).astype(np.int8)]))


def short_for_one_bin(bins, pmf):
    if bins == 1:  # one bin of 100 everywhere would be one-hot: some cells hold less, the last bin's value all the same
        pmf[0, ::2, ::2] = 60
    return pmf


# ---- the comparison itself ---------------------------------------------------------------------------------------------
def test_one_wrong_bit_of_one_drawn_byte_fails():
    pmf, table = contents("plain")
    got, want, sentinel = draw_and_check(pmf, table, G_SMALL, max_cols=COLS + 2)
    flipped = want.copy()
    flipped[3, 2, 5] ^= 1
    with pytest.raises(AssertionError, match="1 of %d drawn bytes differ; first at sample 3 row 2 column 5" % want.size):
        assert_drawn(got, flipped, sentinel)
    stray = got.copy()
    stray[4, 1, COLS] ^= np.int8(0x40)
    with pytest.raises(AssertionError, match="outside the map"):
        assert_drawn(stray, want, sentinel)
    below = got.copy()
    below[0, ROWS, 0] = table[0]
    with pytest.raises(AssertionError, match="outside the map"):
        assert_drawn(below, want, sentinel)


@pytest.mark.parametrize("bins", [1, 2, 8, 9, 16, 17, 32, 33, 64, 65])
def test_every_bins_form(bins):
    """the borders of bins_form (8 | 16 | 32 | 64 bins in registers) and the generic kernel behind them"""
    pmf, table = contents("plain", bins)
    draw_and_check(short_for_one_bin(bins, pmf), table, G_SMALL, max_cols=COLS + 1)


@pytest.mark.parametrize("cols", [1, 3, 4, 5, 8])
@pytest.mark.parametrize("pitch", ["tight", "next_multiple_of_4", "odd_above"])
def test_row_widths_and_pitches(cols, pitch):
    """cols & 3: the aligned and the unaligned PMF load; max_cols & 3 and the last group of a row: word and byte stores"""
    next4 = (cols // 4 + 1) * 4
    max_cols = dict(tight=cols, next_multiple_of_4=next4, odd_above=next4 + 1)[pitch]
    pmf, table = contents("plain", 8, ROWS, cols)
    draw_and_check(pmf, table, G_SMALL, max_cols=max_cols)


def columns_geometry(rows, cols, G):
    """cvar_plan.h sample_choose for the columns kernel (tests/test_cvar_plan.py holds the header to the same rule)"""
    groups = rows * ((cols + 3) // 4)
    chunks = min(max(-(-256 * 1024 // groups), 1), G)
    g_chunk = (-(-G // chunks) + 1) // 2 * 2
    return dict(chunks=chunks, g_chunk=g_chunk, grid_y=-(-G // g_chunk))


@pytest.mark.parametrize("G", [1, 2, 3, 64, 65])
def test_sample_counts(G):
    pmf, table = contents("plain")
    assert columns_geometry(ROWS, COLS, G) == dict(chunks=G, g_chunk=2, grid_y=(G + 1) // 2)
    draw_and_check(pmf, table, G, max_cols=COLS + 1)


def test_chunks_of_six_with_half_a_pair_in_the_last():
    """65 samples of a 128 x 512 map: 16 chunks are asked for, a chunk is then 6 samples and 11 workgroups cover the 65 --
    the last one holds samples 60..64, the first half of pair 32 at its end"""
    rows, cols, G = 128, 512, 65
    geometry = columns_geometry(rows, cols, G)
    assert geometry == dict(chunks=16, g_chunk=6, grid_y=11) and geometry["g_chunk"] > 2 and G % geometry["g_chunk"] == 5
    rng = np.random.default_rng(65)
    # every cell its own PMF (vectorised: floor of a Dirichlet draw, the remainder of at most 7 into one bin)
    p = np.floor(rng.dirichlet(np.full(8, 0.5), size=(rows, cols)) * 100).astype(np.int64)
    np.put_along_axis(p, rng.integers(8, size=(rows, cols, 1)), 0, axis=-1)
    p[..., 7] += 100 - p.sum(axis=-1)
    assert p.min() >= 0 and p.max() <= 127 and (p.sum(axis=-1) == 100).all()
    pmf = np.ascontiguousarray(np.moveaxis(p, -1, 0)).astype(np.int8)
    # a spare row and a pitch above cols (a multiple of 4: the word store), so that a stray store has sentinels to hit
    draw_and_check(pmf, wide_table(rng, 8), G, max_rows=rows + 1, max_cols=cols + 4)


def test_750_chunks_of_two():
    rows, cols, G = 16, 48, 1500
    assert columns_geometry(rows, cols, G) == dict(chunks=1366, g_chunk=2, grid_y=750)
    rng = np.random.default_rng(1500)
    draw_and_check(random_pmf(rng, 8, rows, cols), wide_table(rng, 8), G)


CONTENTS = ["empty_bins", "extremes", "sum127", "wrap_to_255", "wrap_beyond_255", "short", "negative"]


@pytest.mark.parametrize("kind", CONTENTS)
@pytest.mark.parametrize("kernel", ["columns", "generic"])
def test_pmf_contents(kind, kernel):
    """malformed columns included: both kernels follow draw_bin's rule -- int8 accumulator, the first non-negative
    cumulative mass that reaches the target, the last bin's value where none does"""
    pmf, table = contents(kind)
    if kernel == "generic":
        pmf, table = padded(pmf, table)
    draw_and_check(pmf, table, G_CONTENTS, alpha_dyn=1.0, max_cols=COLS + 1)


@pytest.mark.parametrize("alpha_dyn", [1.0, 0.5, 0.07, 1e-6])
@pytest.mark.parametrize("kernel", ["columns", "generic"])
def test_alpha_dyn(alpha_dyn, kernel):
    pmf, table = contents("plain")
    if kernel == "generic":
        pmf, table = padded(pmf, table)
    draw_and_check(pmf, table, G_SMALL, alpha_dyn=alpha_dyn, max_cols=COLS + 1)


@pytest.mark.parametrize("seed", [1, BIG_SEED])
@pytest.mark.parametrize("kernel", ["columns", "generic"])
def test_epochs_and_key(seed, kernel):
    """three calls on a fresh handle: counter words x, y = 0, 1, 2; the key's high word from the seed's high half"""
    pmf, table = contents("plain")
    if kernel == "generic":
        pmf, table = padded(pmf, table)
    draw_and_check(pmf, table, G_SMALL, seed=seed, max_cols=COLS + 1, calls=3)


@pytest.mark.parametrize("first_sample", [2, 6])
@pytest.mark.parametrize("kernel", ["columns", "generic"])
def test_sample_shards(first_sample, kernel):
    """a shard draws samples [first_sample, first_sample + G) of the unsharded set (pair_base | item_base)"""
    pmf, table = contents("plain")
    if kernel == "generic":
        pmf, table = padded(pmf, table)
    draw_and_check(pmf, table, G_SMALL, max_cols=COLS + 1, first_sample=first_sample, calls=2)


# ---- the cell-word sampler, through the costs of a CVaR solve ----------------------------------------------------------
CELL_ROWS, CELL_COLS, CELL_RES = 30, 41, 0.25


def cvar_planner(m, world):
    from mppi_numba_amd.config import Config
    from mppi_numba_amd.mppi import MPPI_Numba
    from mppi_numba_amd.terrain import TDM_Numba
    lin_pmf, ang_pmf, obstacle, unknown = world
    n, t_steps = 96, 20
    cfg = Config(T=t_steps * 0.1, dt=0.1, num_grid_samples=m, num_control_rollouts=n, max_speed_padding=4.0,
                 num_vis_state_rollouts=1, max_map_dim=(40, 50), seed=9, enforce_recommended_limits=False, use_tdm=True)
    assert cfg.num_steps == t_steps
    tdms = []
    for pmf in (lin_pmf, ang_pmf):
        td = dict(xlimits=(0.0, CELL_COLS * CELL_RES), ylimits=(0.0, CELL_ROWS * CELL_RES), res=CELL_RES,
                  bin_values=np.linspace(0.0, 1.0, pmf.shape[0]), bin_values_bounds=(0.0, 1.0), det_dynamics_cvar_alpha=0.2)
        tdm = TDM_Numba(cfg)
        tdm.set_TDM_from_PMF_grid(pmf, td, obstacle, unknown)
        tdms.append(tdm)
    planner = MPPI_Numba(cfg)
    params = bench.make_params("c3")
    params.update(x0=np.array([2.0, 2.0, 0.4]), xgoal=np.array([8.0, 6.0]), alpha_dyn=0.8)
    planner.setup(params, tdms[0], tdms[1])
    planner.record_sample_costs()
    return tdms[0], tdms[1], planner, params


@pytest.mark.parametrize("m", [192, 193, 256])
def test_cell_word_sampler(m):
    """solve() of a CVaR planner with M >= 192 draws both TDMs straight into the cell words (k_sample_cellsM_philox).
    5 and 12 bins share the 16-bin form, the padded map is 34 x 45 (cols & 3 = 1), M = 193 takes the unpaired store.

    What is shown: a second planner that is GIVEN the model's grids and runs the staged iteration has the same costs,
    per-sample costs and controls to the bit -- the only assertions that see the cell words; and the int8 grids read back
    afterwards are the model's (they come from k_sample_grids_philox_cols at the remembered epoch: tdm_materialize).

    What is NOT shown at run time: that the straight-into-cells route was the one taken.  The library has no text that names
    it (last_rollout_kernel() covers the rollout only), and on the sample + pack route every assertion here would pass as
    well, the counters being the same.  tests/test_cvar_plan.py holds cells_choose to this route for exactly these states
    (its rows for 5 and 12 bins, 34 x 45 cells, M = 192, 193, 256); how cells_held reads the handles is not covered."""
    rng = np.random.default_rng(192)
    world = (random_pmf(rng, 5, CELL_ROWS, CELL_COLS), random_pmf(rng, 12, CELL_ROWS, CELL_COLS),
             (rng.random((CELL_ROWS, CELL_COLS)) < 0.02).astype(np.int8), (rng.random((CELL_ROWS, CELL_COLS)) < 0.02).astype(np.int8))
    for mask in world[2:]:
        mask[4:12, 4:12] = 0
    lin_a, ang_a, fused, params = cvar_planner(m, world)
    lin_b, ang_b, staged, _ = cvar_planner(m, world)
    rows, cols = lin_a.get_padded_grid_xy_dim()
    assert cols % 4 != 0 and (lin_a.num_pmf_bins, ang_a.num_pmf_bins) == (5, 12)
    for epoch in range(2):  # two solves: the epochs advance
        u_fused = fused.solve()
        # (the CVaR rollout ran; this text covers the rollout alone and is the same on the sample + pack route)
        assert fused.last_rollout_kernel().startswith("k_rollout_tdm"), fused.last_rollout_kernel()
        models = []
        for tdm in (lin_a, ang_a):
            want = M.sample_grids(tdm.pmf_grid_d.copy_to_host(), tdm.bin_to_int8, 9, epoch, params["alpha_dyn"], m)
            assert_drawn(tdm.sample_grid_batch_d.copy_to_host(), want, 0)  # (the batch starts zeroed)
            models.append(want)
        lin_b.set_sampled_grids(models[0])
        ang_b.set_sampled_grids(models[1])
        staged.sample_noise()
        staged.rollout()
        staged.update()
        assert np.array_equal(fused.costs_d.copy_to_host(), staged.costs_d.copy_to_host())
        assert np.array_equal(fused.sample_costs(), staged.sample_costs())
        assert np.array_equal(u_fused, staged.u_cur_d.copy_to_host())


# ---- control noise -----------------------------------------------------------------------------------------------------
def det_planner(n, t_steps, seed=1, rank=0, world=1, world_map=None):
    """a deterministic-dynamics planner of n local rollouts and t_steps steps over a small nominal map (or bench.py's)"""
    from mppi_numba_amd.config import Config
    from mppi_numba_amd.mppi import MPPI_Numba
    from mppi_numba_amd.terrain import TDM_Numba
    if world_map is None:
        rows = cols = 16
        pmf = np.zeros((2, rows, cols), dtype=np.int8)
        pmf[-1] = 100
        td = dict(xlimits=(0.0, cols * 0.5), ylimits=(0.0, rows * 0.5), res=0.5, bin_values=np.array([0.0, 1.0]),
                  bin_values_bounds=(0.0, 1.0), det_dynamics_cvar_alpha=1.0)
        obstacle = unknown = None
        max_map_dim, padding, x0, goal = (24, 24), 1.0, np.array([2.0, 2.0, 0.3]), np.array([6.0, 6.0])
    else:
        pmf, obstacle, unknown, td = world_map
        max_map_dim, padding, x0, goal = (260, 260), 5.0, np.array([4.0, 4.0, np.pi / 4]), np.array([60.0, 60.0])
    cfg = Config(T=(t_steps + 0.5) * 0.1, dt=0.1, num_grid_samples=1, num_control_rollouts=n * world, max_speed_padding=padding,
                 num_vis_state_rollouts=1, max_map_dim=max_map_dim, seed=seed, enforce_recommended_limits=False,
                 use_det_dynamics=True)
    assert cfg.num_steps == t_steps and cfg.num_control_rollouts == n * world
    lin, ang = TDM_Numba(cfg), TDM_Numba(cfg)
    lin.set_TDM_from_PMF_grid(pmf, td, obstacle, unknown)
    ang.set_TDM_from_PMF_grid(pmf, td, obstacle, unknown)
    planner = MPPI_Numba(cfg, rank=rank, world_size=world)
    params = bench.make_params("c2")
    params.update(x0=x0, xgoal=goal)
    planner.setup(params, lin, ang)
    return lin, ang, planner, params


def noise_deviation(planner, params, seed, epoch, n_offset=0):
    """max |kernel / u_std - model| of the noise the planner holds"""
    got = planner.noise_samples_d.copy_to_host()
    n, t_steps, _ = got.shape
    want, u, turn = M.noise(seed, epoch, n_offset, n, t_steps, (1.0, 1.0))
    assert np.isfinite(got).all()
    std = np.asarray(params["u_std"], dtype=np.float64)
    return float(np.abs(got.astype(np.float64) / std - want).max())


@pytest.mark.parametrize("n,t_steps", [(1, 1), (1, 2), (63, 7), (64, 8), (65, 17), (130, 1), (200, 33)])
def test_noise_counters_at_ragged_sizes(n, t_steps):
    """N below, at and above a tile of 64, odd horizons (the last block's second step is not stored), three calls
    (epochs 0, 1, 2).  Measured on an MI355X, max |kernel / std - model| over the three calls: 4.4e-8 (1, 1), 4.8e-8 (1, 2),
    4.5e-7 (63, 7), 4.5e-7 (64, 8), 4.9e-7 (65, 17), 2.7e-7 (130, 1), 5.6e-7 (200, 33) -- float32 rounding of a value of
    a few units, three orders of magnitude inside the bound and below the 1e-4 at which box_muller_fast would be reported."""
    _, _, planner, params = det_planner(n, t_steps)
    worst = 0.0
    for epoch in range(3):
        planner.sample_noise()
        worst = max(worst, noise_deviation(planner, params, 1, epoch))
    print("\nnoise N=%d T=%d: max |kernel / std - model| = %.3e (bound %.0e)" % (n, t_steps, worst, NOISE_BOUND))
    assert worst <= NOISE_BOUND


def test_noise_key_high_word():
    _, _, planner, params = det_planner(65, 17, seed=BIG_SEED)
    worst = 0.0
    for epoch in range(2):
        planner.sample_noise()
        worst = max(worst, noise_deviation(planner, params, BIG_SEED, epoch))
    print("\nnoise seed 0x%X: max deviation %.3e" % (BIG_SEED, worst))
    assert worst <= NOISE_BOUND


@pytest.mark.parametrize("rank,world,n_local,t_steps", [(1, 2, 100, 17), (2, 3, 70, 8)])
def test_noise_shard_offsets(rank, world, n_local, t_steps):
    """shard `rank` draws rollouts [rank * n_local, (rank + 1) * n_local) of the unsharded noise; n_local is no multiple
    of 64, so the shard's tiles do not line up with the unsharded run's"""
    assert n_local % 64 != 0
    _, _, planner, params = det_planner(n_local, t_steps, rank=rank, world=world)
    worst = 0.0
    for epoch in range(2):
        planner.sample_noise()
        worst = max(worst, noise_deviation(planner, params, 1, epoch, n_offset=rank * n_local))
    print("\nnoise rank %d of %d: max deviation %.3e" % (rank, world, worst))
    assert worst <= NOISE_BOUND


@pytest.mark.parametrize("n,t_steps", [(256, 10), (70, 7), (65, 17)])
def test_noise_a_launch_generates_for_itself(n, t_steps):
    """bench.py's C2 set-up cut down: iterate_async(1) three times on k_rollout_scan_exact, which draws its noise inside the
    launch (scan_noise_pair, rollout_scan_kernel.h: its own rollout / step-pair arithmetic) and stores nothing.

    What noise_samples_d hands out afterwards is NOT that noise: get_noise regenerates the block with the standalone k_noise
    at the epoch the host remembers.  So the read-back only shows the host's epoch bookkeeping: it is the model's noise of
    some epoch in 0..8, and the three epochs follow one another.

    The in-launch generator itself is held through its effect: a twin planner with the same seed runs the same iteration
    stage by stage -- sample_noise (k_noise, stored; held to the model at that epoch here), rollout over the stored noise,
    update -- and must have the costs and the controls of the loop to the bit.  A wrong, shifted or duplicated counter in
    scan_noise_pair gives other noise, hence other costs.  N = 70 and 65 are no multiple of the 32-rollout tile, T = 7 and
    17 leave the last block's second step unused."""
    world_map = bench.synthetic_world("c2", np.random.default_rng(0))
    lin, ang, loop, params = det_planner(n, t_steps, world_map=world_map)
    lin_b, ang_b, staged, _ = det_planner(n, t_steps, world_map=world_map)
    for tdm in (lin, ang, lin_b, ang_b):
        tdm.sample_grids(1.0)
    loop.move_mppi_task_vars_to_device()
    epochs = []
    for _ in range(3):
        loop.iterate_async(1)
        loop.synchronize()
        text = loop.last_rollout_kernel()
        assert text.startswith("k_rollout_scan_exact") and "noise=in-kernel" in text, text
        deviations = [noise_deviation(loop, params, 1, e) for e in range(9)]
        best = int(np.argmin(deviations))
        print("\n%s: read back as epoch %d, max deviation %.3e" % (text, best, deviations[best]))
        assert deviations[best] <= NOISE_BOUND, deviations
        epochs.append(best)
        # the twin: stored noise of the same epoch, pinned to the model, then the same rollout and update
        staged.sample_noise()
        assert noise_deviation(staged, params, 1, best) <= NOISE_BOUND
        staged.rollout()
        assert "noise=in-kernel" not in staged.last_rollout_kernel(), staged.last_rollout_kernel()
        staged.update()
        assert np.array_equal(loop.noise_samples_d.copy_to_host(), staged.noise_samples_d.copy_to_host())
        assert np.array_equal(loop.costs_d.copy_to_host(), staged.costs_d.copy_to_host())
        assert np.array_equal(loop.u_cur_d.copy_to_host(), staged.u_cur_d.copy_to_host())
    assert epochs[1] == epochs[0] + 1 and epochs[2] == epochs[1] + 1, epochs
    assert np.abs(loop.u_cur_d.copy_to_host()).max() > 0  # (the update moved the controls: the costs were not all alike)
