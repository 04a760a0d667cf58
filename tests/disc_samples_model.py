"""Cost model of the barebone rollout over disc samples (numpy, CPU): params['obstacle_track_samples'].

S sampled futures of the moving discs give a rollout S costs, each the cost the crowd launch gives it with that sample as
its disc tracks; walls, wall tracks and a goal track do not depend on the sample and are counted once.  The rollout's cost is
the reference's CVaR tail over the S values (mppi.py:716-755 with block_width = S): sorted descending iff alpha < 1, the
strided float32 tree over the first numel = ceil(S * alpha) entries, the division in double.

Built from the existing models only: crowd_model.hit_counts per sample, wall_model.wall_hits_of_states or
wall_track_model.wall_track_hits_of_states once, wall_model.chain or goal_track_model.chain per sample."""
import numpy as np

import crowd_model
import goal_track_model
import wall_model
import wall_track_model


def cvar_numel(S, alpha):
    """cvar_numel of csrc/cvar_plan.h: ceil(S * float32(alpha)) in double, clamped to [1, S]."""
    return min(int(S), max(1, int(np.ceil(np.float64(S) * np.float64(np.float32(alpha))))))


def cvar_tail(per_sample, alpha):
    """(n, S) float32 per-sample costs -> (n,) float32."""
    sc = np.array(per_sample, dtype=np.float32)
    assert sc.ndim == 2 and sc.shape[1] >= 1, sc.shape
    S = sc.shape[1]
    numel = cvar_numel(S, alpha)
    if np.float32(alpha) < np.float32(1.0):  # (even when numel == S)
        sc = -np.sort(-sc, axis=1)
    st = 1
    while st < numel:
        for i in range(0, S, 2 * st):
            if i + st < numel:
                sc[:, i] = sc[:, i] + sc[:, i + st]  # float32
        st *= 2
    return (sc[:, 0].astype(np.float64) / np.float64(numel)).astype(np.float32)


def sample_costs(p, samples, radii, noise, u, offset=0, wall_segments=None, wall_tracks=None, halfwidths=None,
                 goal_track=None, wall_offset=None):
    """(n, S) float32: the cost of every rollout under every sample.  p: oracle parameters (track_model.oracle_params);
    samples (S, K, L, 2), radii (K,); static walls (W, 2, 2) or wall tracks (W, Lw, 2, 2) with their half-widths; a goal
    track (Lg, 2); all at the one offset (wall_offset: the wall tracks' own -- 0 for a fleet's rows)."""
    samples = np.asarray(samples, np.float32)
    assert samples.ndim == 4 and samples.shape[3] == 2, samples.shape
    assert wall_segments is None or wall_tracks is None
    out, walls, st = [], None, None
    for s in range(len(samples)):
        counts, st = crowd_model.hit_counts(p, samples[s], radii, noise, u, offset)
        if walls is None:  # (the states do not depend on the sample: once)
            walls = np.zeros_like(counts)
            if wall_segments is not None:
                walls = wall_model.wall_hits_of_states(st, wall_segments, halfwidths)
            if wall_tracks is not None:
                walls = wall_track_model.wall_track_hits_of_states(st, wall_tracks, halfwidths,
                                                                   offset if wall_offset is None else wall_offset)
        if goal_track is None:
            out.append(wall_model.chain(p, counts + walls, st, noise, u))
        else:
            goals = goal_track_model.goal_rows(goal_track, st.shape[1] - 1, offset)
            out.append(goal_track_model.chain(p, counts + walls, st, noise, u, goals))
    return np.stack(out, axis=1)


def costs(p, samples, radii, noise, u, alpha, **kw):
    return cvar_tail(sample_costs(p, samples, radii, noise, u, **kw), alpha)
