"""One host model for any form of k_rollout_barebone_crowd (numpy, CPU): a composition of the existing models, with no
arithmetic of its own.

    hits and ring counts   clearance_model.hit_counts / ring_counts -- a footprint or None, no walls, static walls (W, 2, 2) or
                           wall tracks (W, Lw, 2, 2), the track offset
    the chain              wall_model.chain, goal_track_model.chain with a goal track, clearance_model.chain with rings
    disc samples           every sample's discs through the same hit count, the walls counted once (they do not depend on the
                           sample: disc_samples_model.sample_costs), the tail disc_samples_model.cvar_tail

tests/test_form_model.py shows on the CPU that this gives, bit for bit, what each feature's own model gives on that feature."""
import numpy as np

import clearance_model
import disc_samples_model
import goal_track_model
import wall_model


def _chain(p, hits, near, rings, st, noise, u, goals):
    if rings is not None:
        return clearance_model.chain(p, hits, near, rings, st, noise, u, goals)
    if goals is not None:
        return goal_track_model.chain(p, hits, st, noise, u, goals)
    return wall_model.chain(p, hits, st, noise, u)


def sample_costs(p, tracks_or_samples, radii, seg, hw, noise, u, footprint=None, rings=None, goal_track=None, offset=0):
    """(n, S) float32: the cost of every rollout under every disc sample.  p: oracle parameters (with a goal track: xgoal its
    first row, which rests); tracks_or_samples (S, K, L, 2) -- a plain track set (K, L, 2), static discs as tracks of one row,
    counts as one sample --; radii (K,); seg None, (W, 2, 2) or (W, Lw, 2, 2) with hw; footprint (F, 3) or None; rings (R, 2)
    or None (never beside more than one sample: the planner keeps them apart); goal_track (Lg, 2) or None; all at one offset."""
    samples = np.asarray(tracks_or_samples, np.float32)
    if samples.ndim == 3:
        samples = samples[None]
    assert samples.ndim == 4 and samples.shape[3] == 2, samples.shape
    assert rings is None or len(samples) == 1, "clearance rings beside disc samples"
    st = wall_model.states(p, noise, u)
    goals = None if goal_track is None else goal_track_model.goal_rows(goal_track, st.shape[1] - 1, offset)
    none = samples[0][:0], np.asarray(radii, np.float32)[:0]
    wall_hits = clearance_model.hit_counts(st, *none, seg, hw, footprint, offset)  # (zeros without walls)
    wall_near = None if rings is None else clearance_model.ring_counts(st, rings, *none, seg, hw, footprint, offset)
    out = []
    for tracks in samples:
        hits = clearance_model.hit_counts(st, tracks, radii, None, None, footprint, offset) + wall_hits
        near = None if rings is None else clearance_model.ring_counts(st, rings, tracks, radii, None, None, footprint, offset) + wall_near
        out.append(_chain(p, hits, near, rings, st, noise, u, goals))
    return np.stack(out, axis=1)


def costs(p, tracks_or_samples, radii, seg, hw, noise, u, footprint=None, rings=None, goal_track=None, alpha=None, offset=0):
    """(n,) float32: the costs of the form.  A track set (K, L, 2): the chain's; samples (S, K, L, 2) with alpha: the CVaR
    tail over the sample columns."""
    per = sample_costs(p, tracks_or_samples, radii, seg, hw, noise, u, footprint, rings, goal_track, offset)
    if np.ndim(tracks_or_samples) == 3:
        assert alpha is None, "cvar_alpha without disc samples"
        return per[:, 0]
    assert alpha is not None, "disc samples take their cvar_alpha"
    return disc_samples_model.cvar_tail(per, alpha)
