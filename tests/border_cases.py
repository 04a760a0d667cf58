"""Worlds and starts for the map border: rollouts that leave the map, starts on its edge and outside it.

TEST INFRASTRUCTURE (tests/test_border_cases.py checks it on the CPU, tests/test_gpu_border.py runs it on the device).

The kernels CLAMP a cell index that is off the map to the border cell (deliberate deviations).  The
oracle (oracle/mppi_oracle.c: wrap_index) clamps on the HIGH side too, but on the LOW side it wraps as Python's negative
indices do.  So that the oracle can serve as the reference on both sides, every layer of these worlds (linear and angular
traction, obstacle, unknown, risk) has the COPY PROPERTY: its last R columns are copies of column 0, and then its last R
rows copies of row 0 (in that order: the corner comes out consistent).  A negative index down to -R then reads, wrapped,
the bytes the clamp reads.  R bounds the most negative index a rollout can form (negative_index_bound); the grids handed
to the oracle have the map's own dims, so its stride is the map's columns.

No world has a ring of zero-traction cells: a ring would stop the rollouts before any index leaves the map.  Of the two
ways to have none, this module uses Config(max_speed_padding=0.0): pad_cells = ceil(0 * dt / res) = 0, which Config,
TDM_Numba and the library's map preprocessing all accept, so the TDM's own PMF path builds the maps and the padded limits
are the map's limits.  (The other way -- nonzero bytes put over a ring with set_sampled_grids -- is not used.)

The traction bytes come from one-hot PMFs over bin values linspace(0, 1, 8): bytes 0, 14, 28, 42, 57, 71, 85, 100.
"""
import numpy as np

from mppi_numba_amd import tdm_host

ROWS, COLS, R = 96, 104, 40
T_STEPS, DT = 20, 0.1
VMAX = 3.0
BIN_VALUES = np.linspace(0.0, 1.0, 8)
BOUNDS = (0.0, 1.0)
KINDS = {
    # kind: (res, (x origin, y origin)); origins are exact in float32 and not zero, so that pos - lo is a real subtraction
    "nominal": (0.25, (-1.0, 0.5)),
    "cellwise": (0.25, (-1.0, 0.5)),
    "res03": (0.3, (-0.9, 0.6)),
}


def copy_property(layer, r=R):
    """The last r columns <- column 0, then the last r rows <- row 0 (a (..., rows, cols) array, in place)."""
    layer[..., :, -r:] = layer[..., :, :1]
    layer[..., -r:, :] = layer[..., :1, :]
    return layer


def has_copy_property(layer, r=R):
    return bool((layer[..., :, -r:] == layer[..., :, :1]).all() and (layer[..., -r:, :] == layer[..., :1, :]).all())


def one_hot(bins_of_cell):
    pmf = np.zeros((len(BIN_VALUES),) + bins_of_cell.shape, dtype=np.int8)
    np.put_along_axis(pmf, bins_of_cell[None], 100, axis=0)
    return pmf


def world(kind, copies=True, density=0.15, rows=ROWS, cols=COLS, seed=7):
    """The layers and limits of a world.  `copies=False`: the same world without the copy property (the control that shows
    that a low-border case discriminates).  Returns a dict:
      res, xlimits, ylimits, td (what set_TDM_from_PMF_grid takes), lin_pmf, ang_pmf (int8 one-hot (8, rows, cols)),
      obstacle, unknown (int8 (rows, cols)), and the layers the device must arrive at and the oracle reads:
      lin, ang (int8 (1, rows, cols) traction bytes), risk (int8 (1, rows, cols): the speed-map mode's risk layer of lin_pmf
      at alpha = 1; its dynamics are nominal whatever the kind)."""
    res, (ox, oy) = KINDS[kind]
    rng = np.random.default_rng(seed)
    if kind == "nominal":
        lin_bins = np.full((rows, cols), 6)
        ang_bins = np.full((rows, cols), 5)
    else:  # bytes 42 .. 100 per cell, linear and angular different
        lin_bins = rng.integers(3, 8, size=(rows, cols))
        ang_bins = rng.integers(3, 8, size=(rows, cols))
    obstacle = (rng.random((rows, cols)) < density).astype(np.int8)
    unknown = (rng.random((rows, cols)) < density).astype(np.int8)
    # the speed-map mode's risk comes from its own PMF (the dynamics are nominal): cell-wise for every kind
    risk_bins = rng.integers(2, 8, size=(rows, cols))
    if copies:
        for layer in (lin_bins, ang_bins, obstacle, unknown, risk_bins):
            copy_property(layer)
    table = tdm_host.bin_table(BIN_VALUES.astype(np.float32), np.asarray(BOUNDS, dtype=np.float32))
    risk_pmf = one_hot(risk_bins)
    risk = tdm_host.risk_traction_map(risk_pmf, BIN_VALUES.astype(np.float32), np.asarray(BOUNDS, dtype=np.float32), 1.0)
    xlimits, ylimits = (ox, ox + cols * res), (oy, oy + rows * res)
    td = dict(xlimits=xlimits, ylimits=ylimits, res=res, bin_values=BIN_VALUES, bin_values_bounds=BOUNDS,
              det_dynamics_cvar_alpha=1.0)
    return dict(kind=kind, res=res, rows=rows, cols=cols, xlimits=xlimits, ylimits=ylimits, td=td,
                lin_pmf=one_hot(lin_bins), ang_pmf=one_hot(ang_bins), risk_pmf=risk_pmf, obstacle=obstacle, unknown=unknown,
                lin=table[lin_bins][None].astype(np.int8), ang=table[ang_bins][None].astype(np.int8), risk=risk,
                nominal_byte=int(table[-1]))


def flip_outermost_obstacles(obstacle):
    """The obstacle layer with the bit of every outermost cell (the ring of width 1 at the border) flipped -- and, the
    copy property kept, the bits of the copies of column 0 and row 0, which is where the oracle's wrapped index reads the
    low border cells from."""
    out = obstacle.copy()
    ring = np.zeros(out.shape, dtype=bool)
    ring[0, :] = ring[-1, :] = ring[:, 0] = ring[:, -1] = True
    out[ring] ^= 1
    return copy_property(out)


# ---- the starts ------------------------------------------------------------------------------------------------------
# name: (column, row of the start cell; heading).  Cells below 0 or from cols / rows on are outside.  Each heads outwards.
def start_cells(rows=ROWS, cols=COLS):
    mx, my = cols // 2, rows // 2
    q = np.pi / 4
    return {
        # the four edges: the third cell from the border
        "edge_xlo": (2, my, np.pi), "edge_xhi": (cols - 3, my, 0.0), "edge_ylo": (mx, 2, -2 * q), "edge_yhi": (mx, rows - 3, 2 * q),
        # the four corners
        "corner_lolo": (2, 2, -3 * q), "corner_hilo": (cols - 3, 2, -q), "corner_lohi": (2, rows - 3, 3 * q),
        "corner_hihi": (cols - 3, rows - 3, q),
        # the outermost cell of each side
        "cell_xlo": (0, my + 7, np.pi), "cell_xhi": (cols - 1, my - 9, 0.0), "cell_ylo": (mx - 11, 0, -2 * q),
        "cell_yhi": (mx + 5, rows - 1, 2 * q),
        # 1 to 5 cells outside each side
        "out_xlo": (-2, my - 4, np.pi), "out_xhi": (cols, my + 3, 0.0), "out_ylo": (mx + 8, -5, -2 * q), "out_yhi": (mx - 6, rows + 2, 2 * q),
        # far outside: more than `rows` cells beyond both high sides (map_window: no overlap, the whole map)
        "far_hi": (cols + rows + 30, 2 * rows + 30, q),
        # mid-map: the control of the cases with exits (the reach square of T_STEPS steps lies strictly inside the map)
        "mid": (mx, my, q),
    }


LOW_STARTS = ("edge_xlo", "edge_ylo", "corner_lolo", "corner_hilo", "corner_lohi", "cell_xlo", "cell_ylo", "out_xlo", "out_ylo")


def start(w, name):
    """(x0 [x, y, theta], xgoal): inside the named cell (0.4 of a cell from its low corner), the goal 6 m ahead -- as far
    as T_STEPS steps at full speed and full traction get."""
    cx, cy, th = start_cells(w["rows"], w["cols"])[name]
    x = w["xlimits"][0] + (cx + 0.4) * w["res"]
    y = w["ylimits"][0] + (cy + 0.4) * w["res"]
    return np.array([x, y, th]), np.array([x + 6.0 * np.cos(th), y + 6.0 * np.sin(th)])


def params(w, name, **over):
    """The task of a case: C2's cost weights and control ranges, the named start and its goal."""
    x0, xgoal = start(w, name)
    p = dict(x0=x0, xgoal=xgoal, dt=DT, goal_tolerance=0.5, v_post_rollout=0.01, lambda_weight=1.0, cvar_alpha=1.0,
             alpha_dyn=1.0, num_opt=1, u_std=np.array([2.0, 3.0]), vrange=np.array([0.0, VMAX]),
             wrange=np.array([-np.pi, np.pi]), dist_weight=1.0, obs_penalty=1e5, unknown_penalty=1e2)
    p.update(over)
    return p


def cells_outside_low(w, name):
    """How many cells the named start lies outside a low border (0: on the map or beyond a high border)."""
    cx, cy, _ = start_cells(w["rows"], w["cols"])[name]
    return max(0, -cx, -cy)


def negative_index_bound(w, name, t_steps=T_STEPS, vmax=VMAX, trmax=1.0):
    """The most negative cell index a rollout from the named start can form, as a count of cells: the distance travelled
    at the most, T * dt * max|v| * max traction / res, the start's own distance outside, and 2 for the roundings."""
    return int(np.ceil(t_steps * DT * vmax * trmax / w["res"])) + cells_outside_low(w, name) + 2


# ---- the (family, kind, start) triples tests/test_gpu_border.py runs; tests/test_border_cases.py holds each to the
#      conditions on the inputs ----------------------------------------------------------------------------------------
GPU_CASES = {
    "scan_exact": ("nominal", ["edge_xlo", "corner_hihi", "cell_yhi", "out_xhi", "out_ylo", "far_hi"]),
    "scan_exact_reexecuted": ("cellwise", ["edge_yhi", "corner_lolo", "cell_xlo", "out_yhi", "out_xlo"]),
    "scan_exact_direct": ("cellwise", ["edge_ylo", "corner_hilo", "cell_xhi", "far_hi", "out_ylo"]),
    "speed_map": ("cellwise", ["edge_xhi", "corner_lohi", "out_yhi", "out_xlo"]),
    "pipe": ("cellwise", ["edge_xlo", "corner_hihi", "out_xhi", "out_ylo"]),
    "pipe_res03": ("res03", ["edge_yhi", "corner_lolo", "out_yhi"]),
    "fused": ("cellwise", ["edge_ylo", "corner_lohi", "out_xhi"]),
    "general": ("cellwise", ["edge_xhi", "corner_hilo", "out_yhi", "out_xlo"]),
    "tdm": ("cellwise", ["edge_yhi", "corner_hihi", "out_xhi", "cell_ylo"]),
    "batch": ("cellwise", ["corner_lolo", "corner_hilo", "corner_lohi", "corner_hihi", "mid", "far_hi"]),
    "state_rollout": ("cellwise", ["edge_xlo"]),
}
# the long horizon of the pipelined kernel (beyond the time-parallel kernel's 104 steps): v in [0, 0.8] keeps the bound
PIPE_T105 = dict(kind="cellwise", start="out_yhi", t_steps=105, vmax=0.8)
