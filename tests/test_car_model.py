"""tests/car_model.py on the host: with car=False it is oracle.state_rollout_barebone to the bit, and with car=True it has
the properties of a car -- no turning at rest, the heading a float32 running sum of fl(dt * fl(v * kappa)) -- and differs
from the unicycle in most words."""
import numpy as np

import car_model
from oracle import oracle as O
from track_model import oracle_params

N, T = 513, 100


def params_of(vrange=(-1.0, 3.0), wrange=(-2.0, 2.0)):
    return dict(dt=0.1, x0=np.array([0.3, -0.2, 0.7]), xgoal=np.array([7.0, 5.0]), goal_tolerance=0.5, dist_weight=10,
                lambda_weight=1.0, num_opt=1, u_std=np.array([1.0, 1.0]), vrange=np.array(vrange), wrange=np.array(wrange))


def draw(rng):
    noise = rng.normal(0, 1.0, (N, T, 2)).astype(np.float32)
    u_prev = np.stack([rng.uniform(-1.5, 3.5, T), rng.uniform(-2.5, 2.5, T)], 1).astype(np.float32)
    u_cur = np.stack([rng.uniform(-1.5, 3.5, T), rng.uniform(-2.5, 2.5, T)], 1).astype(np.float32)  # (past the ranges: row 0 is unclipped)
    return noise, u_prev, u_cur


def test_the_unicycle_form_is_the_oracle_bit_for_bit():
    p = oracle_params(params_of())
    differ = words = 0
    for seed in range(20):
        noise, u_prev, u_cur = draw(np.random.default_rng(seed))
        want = O.state_rollout_barebone(p, noise, u_prev, u_cur, N)
        got = car_model.state_rollout(p, noise, u_prev, u_cur, N, car=False)
        assert got.shape == want.shape == (N, T + 1, 3)
        differ += int((got.view(np.int32) != want.view(np.int32)).sum())
        words += got.size
    print("%d of %d words differ" % (differ, words))
    assert differ == 0, "%d of %d words differ" % (differ, words)


def test_a_car_at_rest_does_not_turn():
    p = oracle_params(params_of(vrange=(0.0, 0.0)))
    noise, u_prev, u_cur = draw(np.random.default_rng(1))
    u_cur[:, 0] = 0.0  # (row 0 is not clipped)
    st = car_model.state_rollout(p, noise, u_prev, u_cur, N)
    assert (st[:, :, 2].view(np.int32) == st[:, :1, 2].view(np.int32)).all(), "the heading changed at v = 0"
    assert (st[:, :, :2] == st[:, :1, :2]).all()
    unicycle = car_model.state_rollout(p, noise, u_prev, u_cur, N, car=False)
    assert (unicycle[:, -1, 2] != unicycle[:, 0, 2]).mean() > 0.9, "bad input: the unicycle does not turn either"


def test_the_heading_is_the_running_sum_of_the_rounded_products():
    P = params_of()
    p = oracle_params(P)
    noise, u_prev, u_cur = draw(np.random.default_rng(2))
    st = car_model.state_rollout(p, noise, u_prev, u_cur, N)
    v = np.clip(u_prev[None, :, 0] + noise[:, :, 0], np.float32(P["vrange"][0]), np.float32(P["vrange"][1]))
    k = np.clip(u_prev[None, :, 1] + noise[:, :, 1], np.float32(P["wrange"][0]), np.float32(P["wrange"][1]))
    v[0], k[0] = u_cur[:, 0], u_cur[:, 1]
    assert v.dtype == np.float32 and k.dtype == np.float32
    want = car_model.heading_sum(p, v, k)
    assert (st[:, -1, 2].view(np.int32) == want.view(np.int32)).all()
    # reversing with the wheel turned left swings the heading the other way
    back = (v[:, 0] < 0) & (k[:, 0] > 0)
    assert back.any() and (st[back, 1, 2] < st[back, 0, 2]).all()


def test_car_and_unicycle_differ_in_most_words():
    """Equal by construction: the start row and the position after step 0 (5 of 303 words a rollout); v * kappa == kappa
    needs v == 1 or kappa == 0, which a continuous draw does not give, so nearly every other word differs: 0.9 is far below."""
    p = oracle_params(params_of())
    noise, u_prev, u_cur = draw(np.random.default_rng(3))
    car = car_model.state_rollout(p, noise, u_prev, u_cur, N)
    unicycle = car_model.state_rollout(p, noise, u_prev, u_cur, N, car=False)
    share = (car.view(np.int32) != unicycle.view(np.int32)).mean()
    print("%.1f %% of the words differ" % (100 * share))
    assert share > 0.9


def test_the_steering_helpers_are_inverse_to_each_other():
    from mppi_numba_amd.barebone import curvature_of_steering, steering_of_curvature
    steer = np.linspace(-0.6, 0.6, 13)
    kappa = curvature_of_steering(steer, 1.2)
    np.testing.assert_array_equal(kappa, np.tan(steer) / 1.2)
    np.testing.assert_array_equal(steering_of_curvature(kappa, 1.2), np.arctan(1.2 * kappa))
    np.testing.assert_allclose(steering_of_curvature(kappa, 1.2), steer, atol=1e-15)
    assert float(curvature_of_steering(0.0, 2.0)) == 0.0
