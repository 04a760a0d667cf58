"""The recurrence of time-correlated control noise (csrc/noise_smooth.h, k_noise_smooth) in numpy float32, over host-layout
noise (N, T, 2):

    g_c        = float32(sqrt(1 - float64(beta_c) * float64(beta_c)))
    e[n, 0, c] = w[n, 0, c]
    e[n, t, c] = float32(float32(beta_c * e[n, t-1, c]) + float32(g_c * w[n, t, c]))        t = 1 .. T-1

np.float32 products and sums are rounded one by one: numpy has no fused operation to contract them into.
"""
import numpy as np


def gain(beta):
    """float32(sqrt(1 - beta^2)), the square and the root in float64."""
    b = np.asarray(beta, dtype=np.float32).astype(np.float64)
    return np.sqrt(1.0 - b * b).astype(np.float32)


def step(beta, g, e_prev, w):
    """One step, elementwise on float32 arrays: two rounded products, one rounded sum."""
    beta, g, e_prev, w = (np.asarray(v, dtype=np.float32) for v in (beta, g, e_prev, w))
    with np.errstate(under="ignore", over="ignore", invalid="ignore"):
        carried = np.multiply(beta, e_prev, dtype=np.float32)
        fresh = np.multiply(g, w, dtype=np.float32)
        return np.add(carried, fresh, dtype=np.float32)


def smooth(noise, beta):
    """noise (..., T, 2) float32, beta a scalar or (2,): the filtered block, float32, the input left as it is."""
    w = np.asarray(noise)
    assert w.dtype == np.float32 and w.shape[-1] == 2 and w.ndim >= 2
    b = np.ascontiguousarray(np.broadcast_to(np.asarray(beta, dtype=np.float64).astype(np.float32), (2,)))
    g = gain(b)
    e = np.empty_like(w)
    e[..., 0, :] = w[..., 0, :]
    for t in range(1, w.shape[-2]):
        e[..., t, :] = step(b, g, e[..., t - 1, :], w[..., t, :])
    return e


def roughness(u):
    """sum_t |u[t+1] - u[t]|^2 of a control sequence (T, 2), in float64."""
    d = np.diff(np.asarray(u, dtype=np.float64), axis=0)
    return float((d * d).sum())
