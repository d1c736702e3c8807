"""What the band-route StreamDecoder tests share: a numpy float32 restatement of the prefix / band / suffix rule of
csrc/stream_band.hpp (`band_arrays`, to be compared with `stream_cases.reference_arrays`, the full-row rule), generators of
band matrices at given reaches and background, and the tie and non-finite inputs of both test files."""
import math

import numpy as np

NONE = np.iinfo(np.int64).max            # the index of a range without a non-NaN candidate
TINY = np.float32(math.log(np.finfo(np.float32).tiny))          # log(tiny): what the reference's evaluation holds outside its band
BACKGROUNDS = {'minus_inf': np.float32(-np.inf), 'log_tiny': TINY, 'minus_20': np.float32(-20.)}
REACHES = [(2, 2), (0, 0), (0, 3), (3, 0), (2, 5), (5, 2), (31, 31)]


def band_matrix(S, reach_left, reach_right, background, seed=0, grid=None):
    """(S, S) float32 [next, prev]: `background` outside j - reach_left <= i <= j + reach_right; inside, continuous scores in
    (-4, 0) or, with `grid` levels, multiples of -0.25 (0 .. -0.25 * (grid - 1))."""
    rng = np.random.default_rng(seed)
    inside = (-0.25 * rng.integers(0, grid, size=(S, S)) if grid else rng.uniform(-4, 0, size=(S, S))).astype(np.float32)
    j, i = np.meshgrid(np.arange(S), np.arange(S), indexing='ij')
    return np.where((i >= j - reach_left) & (i <= j + reach_right), inside, np.float32(background)).astype(np.float32)


def diagonals(trans, reach_left, reach_right):
    """diag[k][j] = trans[j][j - reach_left + k], (W, S); 0 where that column does not exist."""
    S = trans.shape[0]
    W = reach_left + reach_right + 1
    diag = np.zeros((W, S), np.float32)
    for k in range(W):
        i = np.arange(S) - reach_left + k
        ok = (i >= 0) & (i < S)
        diag[k, ok] = trans[np.arange(S)[ok], i[ok]]
    return diag


def _scan(d, order):
    """Running best non-NaN (value, index) of d along `order`: larger value, then lower index; (-inf, NONE) for none yet."""
    value, index = np.empty(len(d), np.float32), np.empty(len(d), np.int64)
    v, a = np.float32(-np.inf), NONE
    for i in order:
        if not np.isnan(d[i]) and (a == NONE or d[i] > v or (d[i] == v and i < a)):
            v, a = d[i], i
        value[i], index[i] = v, a
    return value, index


def band_arrays(seq, diag, reach_left, reach_right, background, init):
    """Posterior rows and backpointers by the band rule, numpy float32: per frame the two scans of d_i = prev[i] + background,
    then per state the prefix's best, the in-band candidates in ascending i and the suffix's best, each taken on a strict
    '>' (NaN candidates skipped; the first non-NaN candidate starts the maximum); the NaN test of c_0 uses the in-band
    entry when j <= reach_left and d_0 otherwise."""
    T, S = seq.shape
    W = reach_left + reach_right + 1
    background = np.float32(background)
    states = np.arange(S)
    post = np.empty((T, S), np.float32)
    bp = np.zeros((T, S), np.int64)
    post[0] = seq[0] + init
    with np.errstate(invalid='ignore'):
        for t in range(1, T):
            prev = post[t - 1]
            d = prev + background
            pre_v, pre_i = _scan(d, range(S))
            suf_v, suf_i = _scan(d, range(S - 1, -1, -1))
            e = states - reach_left - 1
            best = np.where(e >= 0, pre_v[np.maximum(e, 0)], np.float32(-np.inf)).astype(np.float32)
            arg = np.where(e >= 0, pre_i[np.maximum(e, 0)], NONE)
            for k in range(W):
                i = states - reach_left + k
                ok = (i >= 0) & (i < S)
                c = np.full(S, np.nan, np.float32)
                c[ok] = prev[i[ok]] + diag[k][ok]
                take = ~np.isnan(c) & ((arg == NONE) | (c > best))
                best[take], arg[take] = c[take], i[take]
            e = states + reach_right + 1
            ov = np.where(e < S, suf_v[np.minimum(e, S - 1)], np.float32(-np.inf)).astype(np.float32)
            oi = np.where(e < S, suf_i[np.minimum(e, S - 1)], NONE)
            take = (oi != NONE) & ((arg == NONE) | (ov > best))
            best[take], arg[take] = ov[take], oi[take]
            first = np.where(states <= reach_left, diag[np.maximum(reach_left - states, 0), states], background).astype(np.float32)
            nan0 = np.isnan(prev[0] + first)
            assert (nan0 | (arg != NONE)).all()
            bp[t] = np.where(nan0, 0, arg)
            post[t] = seq[t] + np.where(nan0, np.float32(np.nan), best)
    return post, bp


# ------------------------------------------------------------------------------------------------------------ inputs
def continuous(B, T, S, seed):
    """(B, T, S) float32 log scores without ties worth the name."""
    return np.random.default_rng(seed).uniform(-6, 0, size=(B, T, S)).astype(np.float32)


def grid_scores(B, T, S, levels, seed):
    """(B, T, S) on `levels` multiples of -0.25 -- exact sums, many equal maxima.  (Passed as log inputs they go through
    log(exp(x) + tiny), which returns these values unchanged: tiny is far below half an ulp of exp(-3).)"""
    return (-0.25 * np.random.default_rng(seed).integers(0, levels, size=(B, T, S))).astype(np.float32)


def tie_background(reach_left, reach_right):
    """The grid value outside the band of `tie_problem`: -1 beside a narrow band, whose best in-band score is often that low,
    0 beside a wide one, which nearly always holds a 0."""
    return np.float32(-1. if reach_left + reach_right + 1 < 16 else 0.)


def tie_problem(S, reach_left, reach_right, seed):
    """(obs (T, S), trans, init) on the -0.25 grid with a grid-valued background (`tie_background`) inside the range of the
    in-band scores, so that candidates outside the band tie with the in-band best on both sides (count them with
    `tie_counts`)."""
    T = 24
    obs = grid_scores(1, T, S, 3, seed)[0]
    trans = band_matrix(S, reach_left, reach_right, tie_background(reach_left, reach_right), seed=seed + 1, grid=8)
    return obs, trans, np.zeros(S, np.float32)


def tie_counts(seq, trans, init, reach_left, reach_right, reference_arrays):
    """On the full-row numpy reference: (frames x states where a candidate left of the band equals the in-band best, is the
    overall maximum and therefore must win; ... where the in-band best equals a candidate right of the band, beats the left
    side and therefore must win), each checked against the reference's backpointer."""
    post, bp = reference_arrays(seq, trans, init)
    S = seq.shape[1]
    prefix_wins = band_wins = 0
    for t in range(1, len(seq)):
        cand = post[t - 1][None, :] + trans
        for j in range(S):
            lo, hi = max(j - reach_left, 0), min(j + reach_right, S - 1)
            left = cand[j, :lo].max() if lo > 0 else -np.inf
            mid = cand[j, lo:hi + 1].max()
            right = cand[j, hi + 1:].max() if hi + 1 < S else -np.inf
            if left == mid and left >= right and np.isfinite(left):
                assert bp[t][j] < lo
                prefix_wins += 1
            if mid == right and mid > left and np.isfinite(mid):
                assert lo <= bp[t][j] <= hi
                band_wins += 1
    return prefix_wins, band_wins


def dead_initial(S, plus_inf_at=None):
    """An initial vector of -inf: every row of the stream is -inf (the decoder's epsilon round trip lifts a -inf OBSERVATION
    to log(tiny), so a row of -inf has to come from here), every candidate a tie at -inf.  `plus_inf_at`: 0 there, for a
    first observation of +inf at that state -- a row of -inf with one +inf, which beside a -inf background is a NaN
    candidate of every state outside its band."""
    init = np.full(S, -np.inf, np.float32)
    if plus_inf_at is not None:
        init[plus_inf_at] = 0.
    return init


def nonfinite_sources(T, S, seed):
    """Sequences (T, S) that meet NaN and +/-inf: a NaN at state 0, NaN elsewhere, +inf observations (beside a -inf
    background: NaN candidates that must be skipped), rows of -inf (given to the recurrence as they are: every candidate of
    the next frame -inf, the first non-NaN one wins; behind the decoder's round trip: rows of log(tiny)), with +inf at
    state 0 and elsewhere."""
    base = continuous(6, T, S, seed)
    a, b, c, d, e, f = (base[k].copy() for k in range(6))
    a[T // 3, 0] = np.nan
    b[T // 3, [S // 2, S - 1]] = np.nan
    b[2 * T // 3, 1] = np.nan
    c[T // 4, [3, S // 2]] = np.inf
    c[T // 2, S - 2] = np.inf
    d[T // 3] = -np.inf
    e[T // 3] = -np.inf
    e[T // 3, 0] = np.inf
    f[T // 4, 0] = np.inf                                     # +inf at state 0: c_0 is NaN beside a -inf background
    f[T // 2] = -np.inf
    f[T // 2, [0, 5]] = np.inf
    return [a, b, c, d, e, f]
