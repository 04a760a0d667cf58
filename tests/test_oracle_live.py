"""The oracle against the REFERENCE ITSELF on worlds that are not among the main fixtures: the
reference's kernels were run under the CUDA simulator with other random maps (oracle/gen_golden.py
with GOLDEN_SEED_OFFSET=303, `--only` each of NAMES, `--out tests/golden/seed303`), and the C
restatement has to reproduce what they recorded bit for bit, like the main fixtures."""
import os

import numpy as np
import pytest

from helpers import GOLDEN_DIR, iterations, params_from_golden, ulp_diff_f32
from oracle import oracle as O
from test_oracle_golden import map_params, solve_of_iteration

NAMES = ["det_odd_units", "speedmap_odd_units", "tdm_odd_units"]


@pytest.fixture(scope="module", params=[303])
def live_fixtures(request):
    loaded = {}
    for name in NAMES:
        with np.load(os.path.join(GOLDEN_DIR, "seed%d" % request.param, name + ".npz")) as z:
            loaded[name] = {k: z[k] for k in z.files}
    return loaded


@pytest.mark.parametrize("name", NAMES)
def test_oracle_reproduces_the_reference_on_other_worlds(live_fixtures, name):
    g = live_fixtures[name]
    P = params_from_golden(g)
    n_iter = 0
    for k, it in enumerate(iterations(g)):
        s = solve_of_iteration(g, k)
        P["x0"] = g["solve%d_x0" % s]
        p = map_params(g, P)
        lin, ang = g["solve%d_lin_sample_grid" % s], g["solve%d_ang_sample_grid" % s]
        obs, unk = g["lin_obstacle_map_padded"], g["lin_unknown_map_padded"]
        if name.startswith("tdm"):
            c = O.rollout_tdm(p, lin, ang, obs, unk, it["noise"], it["u_in"])
        else:
            c = O.rollout_det(p, lin, ang, obs, unk, it["noise"], it["u_in"],
                              risk=g.get("lin_risk_traction_map_padded"))
        assert ulp_diff_f32(c, it["costs"]).max() == 0, (name, k)
        w, u, _ = O.update_useq(P["lambda_weight"], it["costs"], it["noise"], P["vrange"], P["wrange"],
                                it["u_in"], num_threads=1)
        assert ulp_diff_f32(w, g["it%d_serial_weights" % k]).max() == 0
        assert ulp_diff_f32(u, g["it%d_serial_u_out" % k]).max() == 0
        n_iter += 1
    assert n_iter >= 1
