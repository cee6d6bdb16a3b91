"""Cases the diverse-selection tests share (tests/test_diverse_host.py, tests/test_gpu_diverse.py)."""
import numpy as np


def integer_rows():
    """Mixing rows of small integers: entries in [-2, 2], Mx = 5, a (17,130) grid, the reference being two pairs of the
    grid.  Every sum, difference, square and partial sum is a small integer, exact in float32 and float64 alike, and
    the square root of an integer is rounded once either way: the two arithmetics see the same order and the same ties
    -> (mix_cat, mix_an, ref) float32."""
    rng = np.random.default_rng(1)
    mc = rng.integers(-2, 3, (17, 5)).astype(np.float32)
    ma = rng.integers(-2, 3, (130, 5)).astype(np.float32)
    ref = np.stack([mc[3] + ma[7], mc[11] + ma[100]])
    return mc, ma, ref


INTEGER_K = 40


def greedy(state, z, k, dtype):
    """The definition, step by step, in ``dtype`` arithmetic on a (C,A) start state (NaN: no candidate) -> (picks as
    flat indices, distances when chosen, steps whose maximum was shared by several candidates)."""
    state, z = state.astype(dtype), z.astype(dtype)
    A = state.shape[1]
    picks, distance, tied = [], [], 0
    with np.errstate(invalid="ignore"):
        for _ in range(k):
            cand = state > 0
            if not cand.any():
                break
            top = state[cand].max()
            at = np.flatnonzero(cand.reshape(-1) & (state.reshape(-1) == top))
            tied += len(at) > 1
            picks.append(int(at[0]))
            distance.append(top)
            diff = z - z[at[0] // A, at[0] % A]
            d2 = np.zeros(state.shape, dtype)
            for kk in range(z.shape[2]):                    # k ascending
                d2 = d2 + diff[:, :, kk] * diff[:, :, kk]
            state = np.minimum(state, np.sqrt(d2))
    return picks, distance, tied
