"""Model of the barebone planner's wall tracks (numpy, CPU): walls that move, built on wall_model.hit and wall_model.chain.

Every wall has Lw segments, row j the segment it occupies during control interval j (from j*dt to (j+1)*dt after "now").
Step t of a rollout moves the robot from P to Q during interval offset + t, so it is tested -- wall_model.hit, unchanged --
against row min(offset + t, Lw - 1) of every wall.  (A disc row is an instant: crowd_model.hit_counts tests the post-step
position against row min(offset + t + 1, L - 1).  Each kind clamps against its own row count.)  The half-widths are
static per wall.  The cost chain is wall_model.chain on `disc hits + wall hits`: nothing but the integer per step knows
that the walls move."""
import numpy as np

import crowd_model
from wall_model import chain, hit


def wall_track_hits_of_states(st, tracks, halfwidths, offset=0):
    """(n, T) int64: how many walls step t hits, for states (n, T+1, >=2), wall tracks (W, Lw, 2, 2) and half-widths: a
    scalar or (W,)."""
    tr = np.asarray(tracks, np.float32)
    assert tr.ndim == 4 and tr.shape[1] >= 1 and tr.shape[2:] == (2, 2), tr.shape
    W, Lw = tr.shape[:2]
    hw = np.ascontiguousarray(np.broadcast_to(np.asarray(halfwidths, np.float32), (W,)))
    n, T = st.shape[0], st.shape[1] - 1
    counts = np.zeros((n, T), np.int64)
    for t in range(T):
        row = min(offset + t, Lw - 1)
        P, Q = st[:, t, None, :2], st[:, t + 1, None, :2]
        for k0 in range(0, W, 64):  # (integers: the order does not matter)
            counts[:, t] += hit(P, Q, tr[None, k0:k0 + 64, row, 0], tr[None, k0:k0 + 64, row, 1], hw[None, k0:k0 + 64]).sum(axis=1)
    return counts


def wall_track_costs(p, disc_tracks, radii, wall_tracks, halfwidths, noise, u, offset=0):
    """Costs (n,) float32 with discs (tracks (K, L, 2), radii (K,); K = 0: none) and wall tracks (W, Lw, 2, 2): the cost
    chain of crowd_model.crowd_costs on disc hits + wall hits, both at the one offset."""
    disc_counts, st = crowd_model.hit_counts(p, disc_tracks, radii, noise, u, offset)
    return chain(p, disc_counts + wall_track_hits_of_states(st, wall_tracks, halfwidths, offset), st, noise, u)
