"""Acceleration limits on the sampled controls, in numpy float32: the recurrence of csrc/control_limits.h, the feasibility
tolerance the issue derives, and the feasibility measure the tests share.  Every operation is one float32 operation; the
loop runs over t and is vectorised over the rollouts."""
import numpy as np

F = np.float32


def step_size(accel, dt):
    """d = float32(float32(accel) * float32(dt)), per component: (2,) float32."""
    acc = np.broadcast_to(np.asarray(accel, dtype=np.float64).astype(F), (2,))
    with np.errstate(over="ignore"):
        return np.multiply(acc, F(dt), dtype=F)


def valid(accel):
    """control_limit_valid: not NaN and > 0 (+inf is one)."""
    with np.errstate(invalid="ignore"):
        return np.asarray(accel, dtype=F) > F(0)


def clip(v, lo, hi):
    """max(lo, min(hi, v)), as the rollouts write it."""
    return np.maximum(F(lo), np.minimum(F(hi), v))


def chain(e, u, lo, hi, anchor, d):
    """One component: e (N, T) float32, u (T,) float32 -> (e' (N, T), p (N, T)).  d = +inf: e itself."""
    e = np.ascontiguousarray(e, dtype=F)
    u = np.asarray(u, dtype=F)
    d = F(d)
    out, path = e.copy(), np.empty_like(e)
    if np.isinf(d):
        return out, clip(np.add(u[None, :], e, dtype=F), lo, hi)
    p = np.full(e.shape[0], clip(F(anchor), lo, hi), dtype=F)
    for t in range(e.shape[1]):
        c = clip(np.add(u[t], e[:, t], dtype=F), lo, hi)
        p = np.minimum(np.maximum(c, np.subtract(p, d, dtype=F)), np.add(p, d, dtype=F))
        path[:, t] = p
        out[:, t] = np.subtract(p, u[t], dtype=F)
    return out, path


def limit(block, u, anchor, vrange, wrange, accel, dt):
    """block (N, T, 2), u (T, 2), anchor (2,) -> e' (N, T, 2) float32; the input is left as it is."""
    block = np.asarray(block, dtype=F)
    u = np.asarray(u, dtype=F)
    d = step_size(accel, dt)
    out = np.empty_like(block)
    for c, (lo, hi) in enumerate((vrange, wrange)):
        out[..., c] = chain(block[..., c], u[:, c], lo, hi, np.asarray(anchor, dtype=F)[c], d[c])[0]
    return out


def applied(noise, u, vrange, wrange):
    """What the rollouts re-form from a block: clip(float32(u + e)), (N, T, 2) float32."""
    noise, u = np.asarray(noise, dtype=F), np.asarray(u, dtype=F)
    out = np.empty_like(noise)
    for c, (lo, hi) in enumerate((vrange, wrange)):
        out[..., c] = clip(np.add(u[None, :, c], noise[..., c], dtype=F), lo, hi)
    return out


def tolerance(vrange, wrange, accel, dt):
    """tol = 2^-20 * (M + d) per component, M = max(|lo|, |hi|): (2,) float64 (inf where the component has no limit)."""
    d = step_size(accel, dt).astype(np.float64)
    m = np.array([np.abs(np.asarray(r, dtype=F).astype(np.float64)).max() for r in (vrange, wrange)])
    return 2.0 ** -20 * (m + d)


def excess(q, anchor, vrange, wrange, accel, dt):
    """q (..., T, 2) sequences: per component, how far the worst of them is outside the feasible set -- the largest of
    (step - d) over the steps, the one from the clipped anchor included, and of the distance outside the box; in float64.
    Feasible within tol: excess <= tol.  A component without a limit has no step to exceed."""
    q = np.asarray(q, dtype=np.float64)
    d = step_size(accel, dt).astype(np.float64)
    worst = np.zeros(2)
    for c, (lo, hi) in enumerate((vrange, wrange)):
        lo, hi = float(F(lo)), float(F(hi))
        a = min(max(float(F(np.asarray(anchor, dtype=F)[c])), lo), hi)
        seq = np.concatenate([np.full(q.shape[:-2] + (1,), a), q[..., c]], axis=-1)
        box = max((lo - q[..., c]).max(), (q[..., c] - hi).max(), 0.0)
        step = np.abs(np.diff(seq, axis=-1)).max() - d[c] if np.isfinite(d[c]) else 0.0
        worst[c] = max(box, step)
    return worst


def largest_step(q, anchor):
    """(2,): the largest |q[t] - q[t-1]| per component, the step from the anchor included."""
    q = np.asarray(q, dtype=np.float64)
    seq = np.concatenate([np.broadcast_to(np.asarray(anchor, dtype=np.float64), q.shape[:-2] + (1, 2)), q], axis=-2)
    return np.abs(np.diff(seq, axis=-2)).reshape(-1, 2).max(axis=0)
