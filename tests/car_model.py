"""State model of the barebone rollout with car-like steering (params['drive'] = 'car'; numpy, CPU): the reference planner
has no car, so the reference for it is the oracle's own state step with one more float32 product.

state_rollout has the signature and the row convention of oracle.state_rollout_barebone -- row 0 is u_cur without noise or
clip, row b >= 1 is clip(u_prev + noise[b]) -- and, with car=False, its bits (tests/test_car_model.py).  A step, every
operation rounded once, float32 unless widened:
  v = clip(u[t][0] + e[0], vrange)      k = clip(u[t][1] + e[1], wrange)
  w = v * k                             (car=False: w = k)
  x' = float32(float64(x) + float64(dt * v) * cos(float64(th)))     y' likewise with sin: the heading BEFORE the step
  th' = th + dt * w
Every cost model of the suite takes its states from oracle.state_rollout_barebone, looked up on the module when it is
called, so monkeypatch.setattr(O, "state_rollout_barebone", car_model.state_rollout) gives the car's costs, hit counts, fleet
plans and walls from the models as they stand."""
import numpy as np


def _clip(lo, hi, x):
    """oracle/mppi_oracle.c: max(lo, min(hi, x))"""
    return np.maximum(lo, np.minimum(hi, x))


def state_rollout(p, noise, u_prev, u_cur, n_vis, car=True):
    """p: oracle parameters; noise (>= n_vis, T, 2), u_prev, u_cur (T, 2) -> (n_vis, T + 1, 3) float32."""
    noise = np.ascontiguousarray(noise, np.float32)
    u_prev, u_cur = np.ascontiguousarray(u_prev, np.float32), np.ascontiguousarray(u_cur, np.float32)
    T = u_cur.shape[0]
    dt = np.float32(p.dt)
    v_lo, v_hi = np.float32(p.vrange[0]), np.float32(p.vrange[1])
    w_lo, w_hi = np.float32(p.wrange[0]), np.float32(p.wrange[1])
    out = np.zeros((n_vis, T + 1, 3), np.float32)
    x = np.full(n_vis, np.float32(p.x0[0]), np.float32)
    y = np.full(n_vis, np.float32(p.x0[1]), np.float32)
    th = np.full(n_vis, np.float32(p.x0[2]), np.float32)
    out[:, 0, 0], out[:, 0, 1], out[:, 0, 2] = x, y, th
    for t in range(T):
        v = _clip(v_lo, v_hi, u_prev[t, 0] + noise[:n_vis, t, 0])
        k = _clip(w_lo, w_hi, u_prev[t, 1] + noise[:n_vis, t, 1])
        if n_vis:
            v[0], k[0] = u_cur[t, 0], u_cur[t, 1]  # row 0: u_cur, no noise, no clip
        w = (v * k).astype(np.float32) if car else k
        th64 = th.astype(np.float64)
        dtv = (dt * v).astype(np.float32).astype(np.float64)
        nx = (x.astype(np.float64) + dtv * np.cos(th64)).astype(np.float32)
        ny = (y.astype(np.float64) + dtv * np.sin(th64)).astype(np.float32)
        th = (th + (dt * w).astype(np.float32)).astype(np.float32)
        x, y = nx, ny
        out[:, t + 1, 0], out[:, t + 1, 1], out[:, t + 1, 2] = x, y, th
    return out


def heading_sum(p, v, k):
    """The float32 running sum th0 + sum_t fl(dt * fl(v_t * k_t)) for clipped controls v, k (n, T): (n,) float32."""
    dt = np.float32(p.dt)
    th = np.full(v.shape[0], np.float32(p.x0[2]), np.float32)
    for t in range(v.shape[1]):
        th = (th + (dt * (v[:, t] * k[:, t]).astype(np.float32)).astype(np.float32)).astype(np.float32)
    return th
