"""Every form of k_rollout_barebone_crowd against the host model, at partial obstacle tiles.

The per-feature modules compare one feature at a time with its model; the lattice (test_gpu_barebone_forms.py) walks the
combinations with every feature in its degenerate shape.  Here every row of the table of forms (crowd_form_legal of
csrc/barebone_plan.h) runs with features that count -- tracks of T + 1 rows, a goal track whose rows differ, three distinct
samples under a sorting tail, two rings with penalties that show in the bits, a body of three discs off the axis -- on
obstacle counts that leave idle lanes in a tile and idle waves in a chunk: (K, W) = (7, 10), one partial tile of each kind,
and (70, 74), a full tile and a partial one; N = 64 a problem, so that every lane from W % 64 on holds a rollout and no
wall; T = 18 against a chunk of 14.  The inputs are those of tests/form_cases.py, the model tests/form_model.py, and
tests/test_form_model.py shows on the CPU that the inputs allow the comparison and mean something.

1. Exact math: every launch gives the model's bits -- rotation on and off, single and batch, both obstacle shapes, 32 forms
   each, single handles at track offsets 0 and 3.  A case names, from last_rollout_kernel(), exactly the 32 forms of its
   (rotation, batch) pair; the four pairs name 128.
2. Fast math has no model of its states, but a step's hits are integers in every math mode and the chain adds obs_penalty
   once per hit: so a launch must give the same bits (a) with its discs and walls in reverse order -- other lanes hold them --
   and (b) with its sets padded to (64, 64) by obstacles about 1e3 m away that nothing can touch -- a full tile has no idle
   lane in the guarded loads.  Both follow from the counting alone; no device's output went into them.  All 32 forms, single
   and batch, at (7, 10): 64 forms with exact=0.  The 32 single exact forms without rotation run them as well, a second
   witness beside the model.
3. A batch of three problems with disc sets of 70, 7 and 0 and wall sets of 10, 74 and 0: a partial tile that begins in the
   middle of the shared arrays; every problem against the model of its own sets."""
import gc
import re

import numpy as np
import pytest

import form_cases as fc
from form_cases import ALPHA, B, N, S, T
from disc_samples_model import cvar_numel
from test_gpu_barebone_batch import assert_bits
from test_gpu_barebone_crowd import cfg_of, shape_of

pytestmark = pytest.mark.gpu

R, F = len(fc.RING_ROWS), len(fc.BODY)


@pytest.fixture(autouse=True)
def release_the_handles():
    """A planner and its device-array views refer to each other, so a handle lives until the cycle collector runs."""
    yield
    gc.collect()


def key_of(kernel):
    """The instantiation a launch's description names: (exact, rotation, batched) + form_cases.form_of's fields.  The
    description says what the handle holds; samples, rings and a footprint run TRACKS forms and take static walls as wall
    tracks of one row (crowd_form), which is the one thing added here."""
    found = re.match(r"k_rollout_barebone_crowd exact=([01]) rotation=([01]) waves=\d+ chunk=\d+((?: \w+=\d+)*)$", kernel)
    assert found, kernel
    said = dict(re.findall(r" (\w+)=(\d+)", found.group(3)))
    assert set(said) <= {"tracks", "problems", "walls", "wall_rows", "goal_rows", "samples", "numel", "footprint", "rings"}, kernel
    extra = bool({"samples", "rings", "footprint"} & set(said))
    walls = "none" if "walls" not in said else ("tracks" if "wall_rows" in said or extra else "static")
    return (found.group(1) == "1", found.group(2) == "1", "problems" in said, "tracks" in said or extra, walls, "goal_rows" in said,
            "samples" in said, "rings" in said, "footprint" in said)


def tail_of(row, K, W, problems=0):
    """What last_rollout_kernel() says behind the chunk: what the row asked for."""
    discs, walls, goal, extra, one_row = row
    return ((" tracks=%d" % (1 if one_row else T + 1) if "samples" in extra or discs == "tracks" else "") +
            (" problems=%d" % problems if problems else "") +
            ("" if walls == "none" else " walls=%d" % W + (" wall_rows=%d" % (T + 1) if walls == "tracks" and not one_row else "")) +
            (" goal_rows=%d" % (T + 1) if goal else "") + (" samples=%d numel=%d" % (S, cvar_numel(S, ALPHA)) if "samples" in extra else "") +
            (" footprint=%d" % F if "footprint" in extra else "") + (" rings=%d" % R if "rings" in extra else ""))


class Sweep:
    """One handle for every row; what its launches named."""

    def __init__(self, math, wscale, problems=0):
        from mppi_numba_amd.barebone import MPPI_Batch, MPPI_Numba
        self.exact, self.rotation, self.problems = math == "exact", math == "exact" and wscale == 1.0, problems
        self.planner = MPPI_Batch(cfg_of(N, T, True, math), problems) if problems else MPPI_Numba(cfg_of(N, T, True, math))
        self.keys = set()

    def launch(self, params, row, u, noise, K, W, offset=0, **sets):
        """((N,) costs -- (problems, N) of a batch --, (N, S) sample columns of a single handle's sample row or None)."""
        planner, columns = self.planner, "samples" in row[3] and not self.problems
        if self.problems:
            planner.setup(params, **sets)
        else:
            planner.set_params(params)
        planner.move_mppi_task_vars_to_device()  # (hands tracks over: "now" is row 0 again)
        if columns:
            planner.record_sample_costs()
        planner.set_track_offset(offset)
        planner.set_u(u)
        planner.set_noise(noise)
        planner.rollout()
        kernel = planner.last_rollout_kernel()
        costs = planner.costs_d.copy_to_host()
        chunk = shape_of(kernel)[1]
        assert T > chunk, kernel  # (a second, partial chunk: waves with wj >= cl)
        head = "k_rollout_barebone_crowd exact=%d rotation=%d waves=" % (self.exact, self.rotation)
        assert kernel.startswith(head) and kernel.endswith(" chunk=%d" % chunk + tail_of(row, K, W, self.problems)), "%s: %s" % (row, kernel)
        assert key_of(kernel) == (self.exact, self.rotation, bool(self.problems)) + fc.form_of(row), "%s: %s" % (row, kernel)
        self.keys.add(key_of(kernel))
        return costs, (planner.sample_costs() if columns else None)

    def launch_row(self, sc, row, offset=0, params=None, K=None, W=None):
        u, noise = (sc["u"], sc["noise"]) if self.problems else (sc["u"][0], sc["noise"][0])
        return self.launch(fc.row_params(sc, row) if params is None else params, row, u, noise,
                           sc["K"] if K is None else K, sc["W"] if W is None else W, offset)

    def named_the_table(self):
        """Exactly the 32 forms of this (math, rotation, batch): a dispatch change cannot empty the sweep unnoticed."""
        want = {(self.exact, self.rotation, bool(self.problems)) + fc.form_of(row) for row in fc.ROWS}
        assert len(want) == 32 and self.keys == want, sorted(want ^ self.keys)


# ---- 1. every exact form against the model -----------------------------------------------------------------------------------
@pytest.mark.parametrize("K,W", fc.SHAPES)
@pytest.mark.parametrize("batch", [False, True])
@pytest.mark.parametrize("wscale", fc.WSCALES)
def test_every_exact_form_equals_the_model(wscale, batch, K, W):
    sc = fc.scene(K, W, wscale)
    sweep = Sweep("exact", wscale, B if batch else 0)
    for row in fc.ROWS:
        for offset in (fc.OFFSETS if fc.moves(row) and not batch else fc.OFFSETS[:1]):
            got, columns = sweep.launch_row(sc, row, offset)
            what = "%s, %d discs, %d walls, rotation %d, offset %d" % (row, K, W, wscale == 1.0, offset)
            for b in range(B if batch else 1):
                want, want_columns = fc.model(K, W, wscale, row, b, offset)
                assert_bits(got[b] if batch else got, want, what + (", problem %d" % b if batch else "") + " vs the model")
            assert (columns is not None) == ("samples" in row[3] and not batch)
            if columns is not None:
                assert_bits(columns, want_columns, what + ": the sample columns vs the model")
    sweep.named_the_table()


def test_the_exact_cases_name_128_forms():
    """Each case above ends by asserting that it named exactly the forms of its (rotation, batch) pair; together those are
    the 128 exact instantiations."""
    keys = {(True, rotation, batch) + fc.form_of(row) for rotation in (False, True) for batch in (False, True) for row in fc.ROWS}
    assert len(keys) == 128
    fast = {(False, False, batch) + fc.form_of(row) for batch in (False, True) for row in fc.ROWS}
    assert len(fast) == 64 and not (fast & keys)


# ---- 2. two identities per form: the order of the obstacles, and tiles without idle lanes ------------------------------------
ALONG = {"obstacle_positions": 0, "obstacle_tracks": 0, "obstacle_radius": 0, "obstacle_track_samples": 1, "wall_segments": 0,
         "wall_tracks": 0, "wall_halfwidth": 0}  # the axis the obstacles lie along
FAR = 1e3  # metres: the scene lies within 10 m of the origin, the widest ring margin is 0.3 m, the body reaches 0.7 m


def reversed_order(params):
    return {k: (np.ascontiguousarray(np.flip(v, axis=ALONG[k])) if k in ALONG else v) for k, v in params.items()}


def padded(params, count=64):
    """The discs and the walls filled up to `count` each with obstacles nobody can touch: discs and walls 0.4 m long about
    FAR away, a metre apart, with radii and half-widths of the set's own (repeated)."""
    out = dict(params)

    def fill(key, far):  # far: (pads, 2) or (pads, 2, 2), broadcast over samples and rows
        have = np.asarray(params[key], np.float32)
        axis = ALONG[key]
        shape = list(have.shape)
        shape[axis] = len(far)
        lead = (None,) * axis + (slice(None),) + (None,) * (have.ndim - axis - far.ndim)
        out[key] = np.concatenate([have, np.broadcast_to(far[lead], shape).astype(np.float32)], axis=axis)

    for key in ("obstacle_positions", "obstacle_tracks", "obstacle_track_samples"):
        if key in params:
            pads = count - np.shape(params[key])[ALONG[key]]
            fill(key, np.stack([FAR + np.arange(pads), np.full(pads, FAR)], axis=1))
            out["obstacle_radius"] = np.resize(np.asarray(params["obstacle_radius"], np.float32), count)
    for key in ("wall_segments", "wall_tracks"):
        if key in params:
            pads = count - len(params[key])
            a = np.stack([FAR + np.arange(pads), np.full(pads, -FAR)], axis=1)
            fill(key, np.stack([a, a + np.array([0.3, 0.25])], axis=1))
            out["wall_halfwidth"] = np.resize(np.asarray(params["wall_halfwidth"], np.float32), count)
    return out


@pytest.mark.parametrize("math,wscale,batch", [("fast", 1.0, False), ("fast", 1.0, True), ("exact", 1.5, False)])
def test_order_and_padding_change_no_bit(math, wscale, batch):
    K, W = fc.SHAPES[0]
    sc = fc.scene(K, W, wscale)
    sweep = Sweep(math, wscale, B if batch else 0)
    kept = {}
    for row in fc.ROWS:
        params = fc.row_params(sc, row)
        want, want_columns = kept[row] = sweep.launch_row(sc, row)
        for what, other, counts in (("in reverse order", reversed_order(params), (K, W)), ("padded to full tiles", padded(params), (64, 64))):
            got, columns = sweep.launch_row(sc, row, params=other, K=counts[0], W=counts[1])
            assert_bits(got, want, "%s math, %s: the obstacles %s" % (math, row, what))
            if want_columns is not None:
                assert_bits(columns, want_columns, "%s math, %s: the sample columns, the obstacles %s" % (math, row, what))
    sweep.named_the_table()
    # the input means something in this math mode too: the walls cost the rollouts of the idle lanes, the discs cost some
    walled, bare = kept[("static", "static", False, (), False)][0], kept[("static", "none", False, (), False)][0]
    assert (walled != bare)[..., W:].any(), "bad input: the walls cost the rollouts in lanes >= %d nothing" % W
    assert (bare >= sc["params"]["obs_penalty"]).any(), "bad input: no disc is hit"  # (the distance terms stay below 1e4)


# ---- 3. mixed counts in one batch -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("wscale", fc.WSCALES)
def test_a_batch_of_mixed_counts_equals_the_model(wscale):
    """Three problems, 70, 7 and 0 discs and 10, 74 and 0 walls, their own track offsets: wall0, wcount and disc_pitch with a
    partial tile that begins in the middle of the shared arrays.  Disc samples are shared by the problems of a batch."""
    problems = len(fc.MIXED_DISCS)
    sc = fc.scene(70, 74, wscale)
    u, noise = fc.mixed_inputs(wscale)
    sweep = Sweep("exact", wscale, problems)
    for row in fc.MIXED_ROWS:
        sets = dict(wall_sets=[(sc["wtracks"][sc["W"] - w:], sc["hw"][sc["W"] - w:]) for w in fc.MIXED_WALLS])
        if "samples" not in row[3]:
            sets["obstacle_sets"] = [(sc["tracks"][:k], sc["rad"][:k]) for k in fc.MIXED_DISCS]
        got, _ = sweep.launch(fc.row_params(sc, row, discs=False, walls=False), row, u, noise, max(fc.MIXED_DISCS), max(fc.MIXED_WALLS),
                              np.array(fc.MIXED_OFFSETS, dtype=np.int32), **sets)
        for b in range(problems):
            assert_bits(got[b], fc.mixed_model(wscale, row, b), "%s, rotation %d, problem %d (%d discs, %d walls) vs the model" % (
                row, wscale == 1.0, b, fc.MIXED_DISCS[b], fc.MIXED_WALLS[b]))
    assert len(sweep.keys) == len(fc.MIXED_ROWS)
