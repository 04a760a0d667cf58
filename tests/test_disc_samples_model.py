"""tests/disc_samples_model.py: its CVaR tail against the pinned oracle's, its per-sample costs against the crowd model."""
import numpy as np
import pytest

from crowd_model import crowd_costs, crowd_discs
from disc_samples_model import cvar_numel, cvar_tail, sample_costs
from helpers import golden, iterations, params_from_golden
from oracle import oracle as O


@pytest.mark.parametrize("name", ["tdm_cvar", "tdm_cvar_odd", "tdm_mean_alpha_dyn"])  # alpha 0.5 (M 8), 0.3 (M 10), 1.0 (M 6)
def test_cvar_tail_is_the_oracles(name):
    g = golden(name)
    P = params_from_golden(g)
    assert (P["cvar_alpha"] < 1) == (name != "tdm_mean_alpha_dyn")
    p = O.make_params(dict(P, x0=g["solve0_x0"]), g["lin_res"], g["lin_padded_xlimits"], g["lin_padded_ylimits"],
                      g["lin_bin_values_bounds"], g["ang_bin_values_bounds"])
    it = iterations(g)[0]
    want, per = O.rollout_tdm(p, g["solve0_lin_sample_grid"], g["solve0_ang_sample_grid"], g["lin_obstacle_map_padded"],
                              g["lin_unknown_map_padded"], it["noise"], it["u_in"], want_per_sample=True)
    assert (np.ptp(per, axis=1) > 0).any(), "bad input: every rollout costs the same under every sample"
    got = cvar_tail(per, P["cvar_alpha"])
    assert (got.view(np.int32) == want.view(np.int32)).all()


def test_numel():
    assert [cvar_numel(16, a) for a in (1.0, 0.99, 0.5, 0.34, 1 / 16, 1e-3)] == [16, 16, 8, 6, 1, 1]
    assert [cvar_numel(3, a) for a in (1.0, 0.99, 0.5, 0.34, 1 / 16)] == [3, 3, 2, 2, 1]
    assert cvar_numel(5, 0.5) == 3 and cvar_numel(2, 0.5) == 1


def _task(n=70, t=20, K=9):
    from track_model import oracle_params
    rng = np.random.default_rng(4)
    params = dict(dt=0.1, x0=np.array([0.0, 0.0, np.pi / 4]), xgoal=np.array([2.2, 2.2]), goal_tolerance=0.5, dist_weight=10,
                  lambda_weight=1.0, num_opt=1, u_std=np.array([1.0, 1.0]), vrange=np.array([0.0, 2.0]),
                  wrange=np.array([-np.pi, np.pi]), obs_penalty=1e6)
    pos, rad = crowd_discs(rng, K, params["x0"], params["xgoal"])
    vel = rng.normal(0, 0.5, (K, 2))
    rows = (np.arange(t + 1) * 0.1)[None, :, None]
    tracks = (pos[:, None].astype(np.float64) + vel[:, None] * rows).astype(np.float32)
    u = np.stack([rng.uniform(0.8, 1.8, t), rng.uniform(-0.2, 0.2, t)], 1).astype(np.float32)
    noise = rng.normal(0, 0.5, (n, t, 2)).astype(np.float32)
    return oracle_params(params), tracks, rad, noise, u


def test_one_sample_is_the_plain_track_set():
    p, tracks, rad, noise, u = _task()
    want = crowd_costs(p, tracks, rad, noise, u, offset=2)
    assert (want > 1e6).any(), "bad input: no rollout is inside a disc"
    per = sample_costs(p, tracks[None], rad, noise, u, offset=2)
    assert per.shape == (len(noise), 1) and (per[:, 0].view(np.int32) == want.view(np.int32)).all()
    for alpha in (1.0, 0.5):
        assert (cvar_tail(per, alpha).view(np.int32) == want.view(np.int32)).all()


@pytest.mark.parametrize("alpha", [1.0, 0.5])  # numel 4 and 2: powers of two, the tree of equal values is exact
def test_four_equal_samples_are_the_plain_track_set(alpha):
    p, tracks, rad, noise, u = _task()
    want = crowd_costs(p, tracks, rad, noise, u)
    got = cvar_tail(sample_costs(p, np.repeat(tracks[None], 4, axis=0), rad, noise, u), alpha)
    assert (got.view(np.int32) == want.view(np.int32)).all()
