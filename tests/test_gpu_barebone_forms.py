"""The lattice of forms of k_rollout_barebone_crowd: the per-feature tests compare each feature with its model; this one walks
the COMBINATIONS, which are what the launcher (launch_barebone_crowd, from crowd_form of csrc/barebone_plan.h) answers for.

Every row of the sweep -- wall kind x goal track x discs x {samples, rings, footprint, and the pairs with a footprint} x
{single, batch} -- holds each of its features in the degenerate shape that the documentation of mppi_numba_amd/barebone.py
declares identical to doing without: tracks of one row, wall tracks of one row, a goal track of equal rows, S copies of one
track set, rings of penalty 0, a footprint of the one disc (0, 0, 0), B equal problems.  Per row: (a) the launch names
exactly the pieces asked for, (b) its costs equal, bit for bit, those of the neighbouring row with one feature less, which
another path of the dispatch launches -- so every row reaches a plain form.  No model, no second library.

Shapes: N = 100 (two tiles, 36 live lanes in the second), T = 18 (chunk 14: a second, partial chunk), 70 discs and 65 walls
(a second, partial tile of each).  A batch needs a multiple of 64 rollouts per problem: 128, the first 100 given the single
handle's noise and compared with it.  Disc samples: the documented identity is per sample -- sample s costs what the launch
with samples[s] as its tracks costs -- so the (N, S) sample costs are compared column by column, and the launch's cost with
the CVaR tail formed here on those columns (cvar_alpha = 1: the float32 tree (c + c) + c, divided by 3 in double; the mean of
three equal float32 values is not always that value).

The same lattice at the tile and chunk edges (test_tile_and_chunk_edges): 0, 64 and 128 discs, 0, 1, 64 and 65 walls, T = 18
and T = 5 -- one partial chunk --, one row per kind of count walk."""
import gc
import itertools

import numpy as np
import pytest

from test_gpu_barebone_batch import assert_bits, make_params
from test_gpu_barebone_crowd import cfg_of, inputs, shape_of
from test_gpu_barebone_fleet import fleet_ending, ring
from test_gpu_barebone_walls import DIAG, GOAL, building, discs_of

pytestmark = pytest.mark.gpu

N, NB, T, K, W, B, S, R = 100, 128, 18, 70, 65, 3, 3, 2
T_SHORT = 5  # a horizon of one partial chunk (test_tile_and_chunk_edges)
OBS_PENALTY = 1000.0  # (the default; a cost of a few hits keeps the distance terms in its low bits)
WALLS, DISCS = ("none", "static", "tracks"), ("static", "tracks")
EXTRAS = ((), ("samples",), ("rings",), ("footprint",), ("samples", "footprint"), ("rings", "footprint"))
ROWS = [row for row in itertools.product(WALLS, (False, True), DISCS, EXTRAS, (False, True))
        if not ("samples" in row[3] and row[2] == "static")]  # (samples take the discs' place: S copies of the one-row tracks)
FAST_ROWS = [(walls, True, "tracks", extra, batch) for walls in ("none", "tracks") for extra in EXTRAS[4:] for batch in (False, True)]


@pytest.fixture(autouse=True)
def release_the_handles():
    """A planner and its device-array views refer to each other, so a handle lives until the cycle collector runs."""
    yield
    gc.collect()


def scene(K=K, W=W, T=T):
    """K discs, W walls, T steps.  The horizon of T_SHORT steps starts 0.45 m down the diagonal, the discs and walls where they
    are: the first discs and the first wall are then within its reach."""
    rng = np.random.default_rng(1818)
    params = make_params(0.1, 1.0)
    params["xgoal"], params["vrange"], params["obs_penalty"] = GOAL.copy(), np.array([0.0, 1.8]), OBS_PENALTY
    u_in, noise = inputs(rng, NB, T)
    pos, rad = discs_of(K, "static", T, params)
    seg, hw = building(W)
    if T == T_SHORT:
        params["x0"] = np.array([0.45 * DIAG[0], 0.45 * DIAG[1], np.pi / 4])
    return params, u_in, noise, pos, rad * np.float32(0.5), seg, hw  # (half the radii: a rollout meets some discs, not most)


def row_params(sc, row):
    params, u_in, _, pos, rad, seg, hw = sc
    K, T = len(pos), len(u_in)
    walls, goal, discs, extra, _ = row
    p = dict(params)
    p["obstacle_radius"] = rad
    if "samples" in extra:
        p["obstacle_track_samples"], p["cvar_alpha"] = np.broadcast_to(pos[None, :, None, :], (S, K, 1, 2)).copy(), 1.0
    elif discs == "tracks":
        p["obstacle_tracks"] = pos[:, None, :].copy()
    else:
        p["obstacle_positions"] = pos
    if walls == "static":
        p["wall_segments"], p["wall_halfwidth"] = seg, hw
    elif walls == "tracks":
        p["wall_tracks"], p["wall_halfwidth"] = seg[:, None].copy(), hw
    if goal:
        del p["xgoal"]
        p["goal_track"] = np.tile(np.float32(GOAL), (T + 1, 1))
    if "rings" in extra:
        p["clearance_rings"] = np.float32([[0.25, 0.0], [0.5, 0.0]])[:R]
    if "footprint" in extra:
        p["footprint"] = np.zeros((1, 3), np.float32)
    return p


def tail_of(row, W=W, T=T):
    """What last_rollout_kernel() says behind the chunk."""
    walls, goal, discs, extra, batch = row
    return ((" tracks=1" if "samples" in extra or discs == "tracks" else "") + (" problems=%d" % B if batch else "") +
            {"none": "", "static": " walls=%d" % W, "tracks": " walls=%d wall_rows=1" % W}[walls] +
            (" goal_rows=%d" % (T + 1) if goal else "") + (" samples=%d numel=%d" % (S, S) if "samples" in extra else "") +
            (" footprint=1" if "footprint" in extra else "") + (" rings=%d" % R if "rings" in extra else ""))


def neighbour(row):
    """The row with one feature less, or None: a plain form (static discs; no walls, or static ones)."""
    walls, goal, discs, extra, batch = row
    if batch:
        return (walls, goal, discs, extra, False)
    if "footprint" in extra:
        return (walls, goal, discs, extra[:-1], False)
    if extra:
        return (walls, goal, discs, (), False)
    if discs == "tracks":
        return (walls, goal, "static", (), False)
    if goal:
        return (walls, False, discs, (), False)
    if walls == "tracks":
        return ("static", goal, discs, (), False)
    return None


def cvar_tail(columns):
    """cvar_alpha = 1 over three samples: the strided float32 tree over all of them, the division in double."""
    assert columns.shape[1] == 3
    total = (columns[:, 0] + columns[:, 1]).astype(np.float32) + columns[:, 2]
    return (total.astype(np.float32).astype(np.float64) / 3.0).astype(np.float32)


class Lattice:
    """One handle per (single / batch); a row's launch is made once and kept."""

    def __init__(self, math, K=K, W=W, T=T):
        from mppi_numba_amd.barebone import MPPI_Batch, MPPI_Numba
        self.math, self.sc, self.shape = math, scene(K, W, T), (K, W, T)
        self.single, self.batch = MPPI_Numba(cfg_of(N, T, True, math)), MPPI_Batch(cfg_of(NB, T, True, math), B)
        self.kept, self.chunks = {}, set()

    def costs(self, row):
        """(N,) costs of a single row, (B, N) of a batch row -- and (N, S) sample costs of a single row with samples."""
        if row in self.kept:
            return self.kept[row]
        _, u_in, noise = self.sc[:3]
        p, batch = row_params(self.sc, row), row[4]
        planner = self.batch if batch else self.single
        if batch:
            planner.setup(p)
            planner.set_u(np.tile(u_in, (B, 1, 1)))
            planner.set_noise(np.tile(noise, (B, 1, 1, 1)))
        else:
            planner.set_params(p)
            planner.set_u(u_in)
            planner.set_noise(noise[:N])
        columns = None
        if "samples" in row[3] and not batch:
            planner.record_sample_costs()
        planner.rollout()
        kernel = planner.last_rollout_kernel()
        costs = planner.costs_d.copy_to_host()
        if "samples" in row[3] and not batch:
            columns = planner.sample_costs()
        # (a) the launch names exactly the pieces the row asked for
        K, W, T = self.shape
        if not K and row[0] == "none":  # (nothing to count: not a crowd launch; the scene's cost without obstacles)
            assert kernel.startswith("k_rollout_barebone ") and not row[3] and not batch, "%s: %s" % (row, kernel)
            self.kept[row] = (costs, None)
            return self.kept[row]
        chunk = shape_of(kernel)[1]
        self.chunks.add(chunk)
        assert T > chunk or T == T_SHORT, kernel  # (T_SHORT: one partial chunk, asked for as such)
        head = "k_rollout_barebone_crowd exact=%d rotation=%d waves=" % (self.math == "exact", self.math == "exact")
        assert kernel.startswith(head) and kernel.endswith(" chunk=%d" % chunk + tail_of(row, W, T)), "%s: %s" % (row, kernel)
        self.kept[row] = (costs[:, :N] if batch else costs, columns)
        return self.kept[row]

    def check(self, row):
        """(b) bit for bit the neighbouring form's costs."""
        costs, columns = self.costs(row)
        if neighbour(row) is None:
            return
        want = self.costs(neighbour(row))[0]
        what = "%s math, %s vs %s" % (self.math, row, neighbour(row))
        if columns is not None and "footprint" not in row[3]:  # S copies of the track set against the track set
            for s in range(S):
                assert_bits(columns[:, s], want, what + ", sample %d" % s)
            want = cvar_tail(columns)
        for b in range(B if row[4] else 1):
            assert_bits(costs[b] if row[4] else costs, want, what + (", problem %d" % b if row[4] else ""))

    def the_input_means_something(self):
        """(Of a scene without discs, or without walls, the half that it has.)"""
        K, W, _ = self.shape
        free = self.costs(("none", False, "static", (), False))[0]
        assert len(np.unique(free)) > N // 2, "bad input: the costs are alike"
        if K:
            assert (free >= OBS_PENALTY).any(), "bad input: no disc is hit"
        if W:
            walled = self.costs(("static", False, "static", (), False))[0]
            assert (walled >= free + OBS_PENALTY).any(), "bad input: the walls cost nothing"


@pytest.mark.parametrize("math", ["exact", "fast"])
def test_every_form_equals_its_neighbour(math):
    lattice = Lattice(math)
    for row in (ROWS if math == "exact" else FAST_ROWS):
        lattice.check(row)  # (and, through the neighbours, every row below it)
    lattice.the_input_means_something()
    assert len(ROWS) == 120 and all(neighbour(row) is None or neighbour(row) in ROWS for row in ROWS)


EDGE_EXTRAS = ((), ("samples",), ("rings",), ("samples", "footprint"), ("rings", "footprint"))


@pytest.mark.parametrize("T", [T, T_SHORT])
@pytest.mark.parametrize("K,W", [(0, 64), (64, 0), (64, 65), (128, 1)])
def test_tile_and_chunk_edges(K, W, T):
    """Disc and wall counts at the tile's edges -- none, exactly one tile, exactly two, one past a tile -- under every kind of
    count walk, over a horizon with a second, partial chunk (T = 18) and one that is a single partial chunk (T = 5).  The
    plain row has static discs and static walls; the others hold one-row tracks of both and reach it through their
    neighbours."""
    lattice = Lattice("exact", K, W, T)
    for extra in EDGE_EXTRAS:
        lattice.check(("tracks" if extra and W else "static" if W else "none", False, "tracks" if extra else "static", extra, False))
    lattice.the_input_means_something()
    if T == T_SHORT:
        assert min(lattice.chunks) >= T, lattice.chunks  # (one chunk, and a partial one)


def test_the_fleet_rows():
    """The fleet's form against per-problem wall tracks that hold the walls of its refresh; a fleet of bodies whose body is
    three times the disc (0, 0, r) -- padded to four slots a robot -- against the disc fleet of radius r (dyadic: the
    half-widths r + r and (r + 0) + r are the same double)."""
    from mppi_numba_amd.barebone import MPPI_Batch
    x0s, goals, us, noise = ring(B, NB, T, 7 * B + T, radius=0.5)
    params = make_params(0.1, 1.0)
    batch = MPPI_Batch(cfg_of(NB, T, True), B)
    batch.setup(params, x0s, goals)

    def launch():
        batch.set_u(us)
        batch.set_noise(noise)
        batch.rollout()
        return batch.costs_d.copy_to_host(), batch.last_rollout_kernel()

    free, kernel = launch()
    assert "walls" not in kernel, kernel
    batch.set_fleet(0.25)
    fleet, kernel = launch()
    assert kernel.endswith(" problems=%d" % B + fleet_ending(B, 0, T)), kernel
    assert (fleet != free).any(), "bad input: no rollout meets another robot's plan"
    seg, hw, _ = batch.fleet_walls()
    batch.set_fleet(None)
    batch.set_wall_sets([(seg[b], hw[b]) for b in range(B)])
    walled, kernel = launch()
    assert kernel.endswith(" problems=%d walls=%d wall_rows=%d" % (B, B - 1, T)), kernel
    assert_bits(walled, fleet, "the fleet vs wall sets that hold its walls")
    batch.set_wall_sets(None)
    batch.set_fleet_bodies(np.float32([[0.0, 0.0, 0.25]] * 3))
    bodies, kernel = launch()
    assert kernel.endswith(" problems=%d walls=%d wall_rows=%d fleet=%d footprint=3" % (B, (B - 1) * 4, T, B)), kernel
    assert_bits(bodies, fleet, "a fleet of bodies of three equal centred discs vs the disc fleet")
