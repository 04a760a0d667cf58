"""numpy restatement of the oracle's deterministic rollout (oracle/mppi_oracle.c: oracle_rollout_det) that keeps
what the stage-cost walk of k_rollout_scan_exact consumes: per (rollout, step) the stage cost and the two penalties.

TEST INFRASTRUCTURE for tests/test_gpu_stage_walk.py: the tests prove it on every input they use (walking its
addends in the oracle's order gives the oracle's bits) and then ask it what the oracle does not tell: in which steps
a rollout pays both penalties, where it stands still, and what the costs would be if the two penalties of a step
were added as one float32 sum.
"""
import numpy as np

from scan_model import _cell_index

f32, f64 = np.float32, np.float64


def stage_records(p, lin_grid, ang_grid, obs, unk, noise, u, risk=None):
    """p: oracle.OracleParams.  Returns a dict of [N, T] arrays -- sg float64 (stage cost), po / pu float32 (obstacle /
    unknown penalty), active (the step is executed: no goal hit before it), still (the step starts in a cell of zero
    linear traction) -- and term float64 [N], the terminal cost."""
    noise, u = np.asarray(noise, dtype=f32), np.asarray(u, dtype=f32)
    N, T = noise.shape[:2]
    lin, ang = np.asarray(lin_grid)[0], np.asarray(ang_grid)[0]
    rp, cp = obs.shape
    dt = f64(f32(p.dt))
    res, xlo, ylo = f32(p.res), f32(p.xlo), f32(p.ylo)
    xg, yg = (f32(v) for v in p.xgoal)
    gt2 = f64(f32(p.goal_tolerance) * f32(p.goal_tolerance))
    x, y, th = (np.full(N, f32(v), dtype=f32) for v in p.x0)
    out = dict(sg=np.zeros((N, T), f64), po=np.zeros((N, T), f32), pu=np.zeros((N, T), f32),
               active=np.zeros((N, T), bool), still=np.zeros((N, T), bool))
    done = np.zeros(N, bool)
    d2 = np.full(N, 1e9)
    for t in range(T):
        gx, gy = _cell_index(x, xlo, res, lin.shape[1]), _cell_index(y, ylo, res, lin.shape[0])
        mx, my = _cell_index(x, xlo, res, cp), _cell_index(y, ylo, res, rp)
        vtr = p.lin_lo + p.lin_ratio * lin[gy, gx].astype(f64)
        wtr = p.ang_lo + p.ang_ratio * ang[gy, gx].astype(f64)
        v = np.clip((u[t, 0] + noise[:, t, 0]).astype(f32), f32(p.vrange[0]), f32(p.vrange[1])).astype(f64)
        w = np.clip((u[t, 1] + noise[:, t, 1]).astype(f32), f32(p.wrange[0]), f32(p.wrange[1])).astype(f64)
        th64 = th.astype(f64)
        nx = (x.astype(f64) + dt * vtr * v * np.cos(th64)).astype(f32)
        ny = (y.astype(f64) + dt * vtr * v * np.sin(th64)).astype(f32)
        nth = (th64 + dt * wtr * w).astype(f32)
        x, y, th = np.where(done, x, nx), np.where(done, y, ny), np.where(done, th, nth)
        dx, dy = (xg - x).astype(f32).astype(f64), (yg - y).astype(f32).astype(f64)
        d2 = np.where(done, d2, dx * dx + dy * dy)
        step_time = dt if risk is None else dt / (p.lin_lo + p.lin_ratio * risk[my, mx].astype(f64) + 1e-6)
        out["active"][:, t] = ~done
        out["still"][:, t] = ~done & (vtr == 0.0)
        out["sg"][:, t] = np.where(done, 0.0, step_time + f64(p.dist_weight) * np.sqrt(d2))
        out["po"][:, t] = np.where(done, f32(0), obs[my, mx].astype(f32) * f32(p.obs_cost))
        out["pu"][:, t] = np.where(done, f32(0), unk[my, mx].astype(f32) * f32(p.unknown_cost))
        done = done | (d2 <= gt2)
    out["term"] = np.where(done, 0.0, 1.0) * np.sqrt(d2) / (f64(f32(p.v_post_rollout)) + 1e-6)
    return out


def control_terms(p, noise, u):
    """[N, T] float64: control_cost_term of the oracle"""
    s = np.array([f64(f32(p.u_std[0])) ** 2, f64(f32(p.u_std[1])) ** 2])
    uo = np.asarray(u, f32).astype(f64) / s[None, :]
    e = np.asarray(noise, f32).astype(f64)
    return f64(f32(p.lambda_weight)) * (uo[None, :, 0] * e[:, :, 0] + uo[None, :, 1] * e[:, :, 1])


def walk(rec, terms, merged=False):
    """The oracle's additions in the oracle's order (mppi.py:994-998, 1005-1009); merged: the two penalties of a step
    as one float32 sum -- what the stage-cost walk may only do where one of them is +0.0f."""
    sg, po, pu, active = rec["sg"], rec["po"], rec["pu"], rec["active"]
    cost = np.zeros(sg.shape[0], dtype=f32)
    for t in range(sg.shape[1]):
        c = (cost.astype(f64) + sg[:, t]).astype(f32)
        if merged:
            c = (c + (po[:, t] + pu[:, t]).astype(f32)).astype(f32)
        else:
            c = ((c + po[:, t]).astype(f32) + pu[:, t]).astype(f32)
        cost = np.where(active[:, t], c, cost)
    cost = (cost.astype(f64) + rec["term"]).astype(f32)
    for t in range(terms.shape[1]):
        cost = (cost.astype(f64) + terms[:, t]).astype(f32)
    return cost
