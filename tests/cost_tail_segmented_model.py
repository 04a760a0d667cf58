"""The T control-cost additions behind the terminal cost (mppi.py:1005-1009) in SEGMENTED integer form.

test_cost_tail_model.py states the integer form for a cost that stays strictly inside one float32 binade and meets no
tie, and measures why that alone buys nothing: 0.9 % of C2's rollouts leave it, i.e. a quarter of the tiles, i.e. every
launch.  This file states the missing piece -- the rollouts that leave it are ALSO done in integer form, piece by piece
-- in numpy, with the reference's two roundings, for every rollout (not only the safe ones):

  1. c (float32; at first the cost after the terminal cost) lies in a binade B = [2^k, 2^(k+1)): q = 2^(k-23) is its
     ulp, fine = q * 2^-29 the ulp of the float64 sum.
  2. For the steps not yet added: m_t = rn(rn(a_t / fine) * 2^-29) ulps (independent of c), their prefix sums, and per
     PIECE of 4 steps (steps 4 j .. 4 j + 3 of the horizon: the steps one lane of a chunk wave holds) the minimum and the
     maximum of the prefix sums and whether one of the piece's increments is a tie of either rounding.
  3. The first piece whose bounds are not one ulp clear of both binade edges (c / q + prefix within
     [2^23 + 1, 2^24 - 2]: the margin test_cost_tail_model.py found) or that holds a tie ends the round.  Without such
     a piece the result is c + (sum of m) * q.
  4. The cost at that piece's start is exact -- c + prefix * q, all earlier pieces were clear -- and the piece's 4
     steps are walked in float arithmetic (the three-instruction form: add, round to float32, widen).
  5. The next round starts behind the piece, in whatever binade the cost is in now.
  6. At most MAX_ROUNDS rounds; what is left after them is walked.

THE WALK RULE.  A round is only started from a cost that is a positive, normal, finite float32.  Zero, subnormal,
negative and non-finite costs have no binade whose ulp grid the increments could be rounded to (below 2^-126 the
float32 grid stops getting finer; at zero there is no grid at all), so from such a cost the remainder is walked.  Costs
below 1 that are normal (2^-126 <= c) are scale-free and take the integer form like any other.

Negative costs: the oracle (oracle/mppi_oracle.c, rollout_det: dt + dist_weight * distance, the obstacle and unknown
penalties, the terminal cost) only adds non-negative terms before the control-cost terms as long as dist_weight and the
penalties are non-negative, as every configuration of the project has them: c0 >= +0.  The control-cost terms have
either sign, so the RUNNING cost can turn negative when the stage costs are small (a problem whose costs stay below 1):
the walk rule covers it.

A round count of r means r integer evaluations: 1 = safe, 2 = one piece walked (one crossing or one tie), ...
MAX_ROUNDS = 17: the smallest value that C2-like inputs never exceed in 10^6 rollouts (print_round_shares below, recorded
in profiles/HISTORY.md).  It is that large because a cost next to a binade edge does not cross it once: with terms of
+-1 (thousands of ulps) it is a random walk around the edge and crosses it ~sqrt(T) times, one round each.  99.1 % of the
rollouts and 76 % of the tiles need one round, 19 % of the tiles two -- but 5 % need three or more, and a launch of 256
tiles ends with its slowest tile: the median launch holds a tile of 10 rounds, none fewer than 5 (print_round_shares, 122 launches), which at the
~0.6k cycles a round was estimated at is MORE than the 3.3k cycles of the walk it replaces.  The form is exact; what it
does not do is shorten a launch, and that is why the kernel does not carry it (profiles/HISTORY.md)."""
import numpy as np

from test_cost_tail_model import c2_like, walk  # noqa: F401  (walk: the statement this form must equal bit for bit)

f32, f64 = np.float32, np.float64
PIECE = 4
MAX_ROUNDS = 17
TINY = np.float32(2.0 ** -126)


def walk_steps(c, a):
    """the three-instruction form over the columns of a"""
    c = c.astype(f32)
    for t in range(a.shape[1]):
        c = (c.astype(f64) + a[:, t]).astype(f32)
    return c


def can_start_round(c):
    """the walk rule: positive, normal, finite"""
    return np.isfinite(c) & (c >= TINY)


def segmented(c0, a, max_rounds=MAX_ROUNDS):
    """(cost after the T additions, rounds[n]).  rounds = integer evaluations the rollout took part in with work left;
    0 = walked from the start (the walk rule)."""
    n, T = a.shape
    c = c0.astype(f32).copy()
    pos = np.zeros(n, np.int64)      # next step to add: a multiple of PIECE, or T
    rounds = np.zeros(n, np.int64)
    n_pieces = (T + PIECE - 1) // PIECE
    Tp = n_pieces * PIECE
    ap = np.zeros((n, Tp), f64)
    ap[:, :T] = a                    # (steps past the horizon add +0.0: m = 0, no tie)
    step = np.arange(Tp)
    for _ in range(max_rounds):
        act = np.flatnonzero((pos < T) & can_start_round(c))
        if len(act) == 0:
            break
        rounds[act] += 1
        ca, aa, pa = c[act], ap[act], pos[act]
        k = np.frexp(ca.astype(f64))[1].astype(np.int64) - 1            # ca in [2^k, 2^(k+1))
        q = np.ldexp(1.0, k - 23)
        fine = np.ldexp(1.0, k - 52)
        with np.errstate(over="ignore", invalid="ignore"):
            a1 = aa / fine[:, None]
            a1r = np.rint(a1)                                            # first rounding: the float64 sum's grid
            tie = np.abs(a1 - np.trunc(a1)) == 0.5
            m_exact = a1r * 2.0 ** -29
            m = np.rint(m_exact)                                         # second rounding: the float32 store
            tie |= np.abs(m_exact - np.trunc(m_exact)) == 0.5
            todo = step[None, :] >= pa[:, None]
            m = np.where(todo, m, 0.0)
            prefix = np.cumsum(m, axis=1)                                # (integers far below 2^53: exact)
            base = ca.astype(f64) / q
            level = base[:, None] + prefix
            clear = (level >= 2.0 ** 23 + 1) & (level <= 2.0 ** 24 - 2) & ~tie   # (a NaN level is not clear)
        clear |= ~todo
        piece_clear = clear.reshape(len(act), n_pieces, PIECE).all(axis=2)
        first = np.where(piece_clear.all(axis=1), n_pieces, np.argmin(piece_clear, axis=1))
        start = first * PIECE                                            # first step of the piece to walk (Tp: none)
        before = np.where(start > 0, prefix[np.arange(len(act)), np.maximum(start, 1) - 1], 0.0)
        with np.errstate(invalid="ignore"):
            c_at = ((base + before) * q).astype(f32)               # exact: all pieces before `first` were clear
        walked = c_at.copy()
        idx = np.minimum(start[:, None] + np.arange(PIECE)[None, :], Tp - 1)
        piece = np.take_along_axis(aa, idx, axis=1)
        piece = np.where((start < Tp)[:, None], piece, 0.0)
        walked = np.where(start < Tp, walk_steps(walked, piece), c_at)
        c[act] = walked
        pos[act] = np.minimum(start + PIECE, Tp)
    rest = np.flatnonzero(pos < T)
    for i in rest:                                                       # beyond the rounds, or the walk rule
        c[i] = walk_steps(c[i:i + 1], a[i:i + 1, pos[i]:])[0]
    return c, rounds


def round_shares(rounds, tile=32):
    """share of the tiles of `tile` rollouts whose slowest rollout needs 1, 2, ... rounds"""
    per_tile = rounds[:len(rounds) // tile * tile].reshape(-1, tile).max(axis=1)
    top = int(per_tile.max())
    return {r: float((per_tile == r).mean()) for r in range(1, top + 1)}, top


def print_round_shares(n=1_000_000, t=100, seed=11, max_rounds=64):
    rng = np.random.default_rng(seed)
    rounds = []
    for _ in range(10):
        c0, a = c2_like(n // 10, t, rng)
        rounds.append(segmented(c0, a, max_rounds=max_rounds)[1])
    rounds = np.concatenate(rounds)
    shares, top = round_shares(rounds)
    print("\nC2-like, %d rollouts, T = %d: rounds per rollout: %s" % (
        len(rounds), t, ", ".join("%d: %.4f %%" % (r, 100 * (rounds == r).mean()) for r in range(1, top + 1))))
    print("tiles of 32 by the rounds of their slowest rollout: %s; most rounds of any rollout: %d" % (
        ", ".join("%d: %.2f %%" % (r, 100 * s) for r, s in shares.items()), int(rounds.max())))
    per_launch = rounds[:len(rounds) // 8192 * 8192].reshape(-1, 8192).max(axis=1)
    if len(per_launch):
        print("launches of 256 tiles by the rounds of their slowest tile: median %d, min %d, max %d (%d launches)" % (
            int(np.median(per_launch)), int(per_launch.min()), int(per_launch.max()), len(per_launch)))
    return rounds


if __name__ == "__main__":
    print_round_shares()
