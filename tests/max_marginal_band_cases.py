"""What tests/test_max_marginals_band_cpu.py and tests/test_max_marginals_band_gpu.py share: a numpy restatement of the band
rule of max-marginals (MARGINALS.md, "Band route"), written here independently of torbi_amd and of the kernels, the
generators of band problems, and the operand-form rows of the two new entries.

The rule, all sums float32 with one rounding each, A [next j][prev i] with A[j][i] == background outside
j - rl <= i <= j + rr, pre[x] = max(v[0..x]), suf[x] = max(v[x..S-1]), pre[-1] = suf[S] = -inf:

    forward   inner_t[j] = max( max_{i in band} fl(alpha_{t-1}[i] + A[j][i]), fl(max(pre[j-rl-1], suf[j+rr+1]) + background) )
              alpha_t[j] = fl(o_t[j] + inner_t[j])                                     pre / suf over alpha_{t-1}
    backward  w[j] = fl(o_{t+1}[j] + beta_{t+1}[j])
              beta_t[i]  = max( max_{j in band} fl(A[j][i] + w[j]), fl(background + max(pre[i-rr-1], suf[i+rl+1])) )

`restate` is that, and counts the cells each of the two terms strictly decides.  The REFERENCE of every comparison is
`max_marginal_cases.loop` on the full matrix, never this file: the restatement is itself under test
(tests/test_max_marginals_band_cpu.py) and says which inputs exercise the out-of-band term at all.
"""
import functools

import numpy as np

import max_marginal_cases as mmc
import operand_form_cases as ofc
import stream_band_cases as sbc
from torbi_amd import margins

NINF = np.float32(-np.inf)
THREADS = 1024                       # mmb::kThreads: a thread owns states tid, tid + 1024, ...
MAX_GROUP, WORKGROUPS = 4, 256       # mmb::kMaxGroup, mmb::kWorkgroups
MAX_LDS = 159 * 1024                 # mmb::kMaxLdsBytes
BACKGROUNDS = {'minus_inf': NINF, 'log_tiny': sbc.TINY, 'minus_3': np.float32(-3.)}
# (S, reach_left, reach_right): sbc.REACHES at the floor, and two bands wider than half the row: with 40/20 the first 41 rows
# have no out-of-band column on the left and the last 21 none on the right; with 40/30 rows 33 .. 40 have none at all
REACH_CASES = [(64, left, right) for left, right in sbc.REACHES] + [(64, 40, 20), (64, 40, 30)]


def lds_bytes(G, S, left, right):
    """mmb::lds_bytes: two rows with halos of max(left, right) on both sides and two scans per item."""
    return (2 * G * (S + 2 * max(left, right)) + 2 * G * S) * 4


def items_per_workgroup(B, S, left, right):
    """The G of mmb_kernel<G> a call runs (mm_band_items): from 4, halved while the LDS rows do not fit, then while the launch
    has fewer than 256 workgroups."""
    G = MAX_GROUP
    while G > 1 and lds_bytes(G, S, left, right) > MAX_LDS:
        G //= 2
    while G > 1 and -(-B // G) < WORKGROUPS:
        G //= 2
    return G


def _extremes(v):
    """(pre, suf) with one more slot each: pre[x + 1] = max(v[0..x]), pre[0] = -inf; suf[x] = max(v[x..S-1]), suf[S] = -inf."""
    pre = np.concatenate([[NINF], np.maximum.accumulate(v)]).astype(np.float32)
    suf = np.concatenate([np.maximum.accumulate(v[::-1])[::-1], [NINF]]).astype(np.float32)
    return pre, suf


def _step(v, entries, lo, hi, background):
    """One max-plus step by the band rule.  entries[x][k]: the matrix entry that meets v[lo[x] + k] for k < hi[x] - lo[x] + 1
    (the in-band candidates of output x, lo / hi already clipped to the row).  Returns (out (S,), the in-band term, the
    out-of-band term)."""
    S = len(v)
    pre, suf = _extremes(v)
    inside = np.full((S,), NINF, np.float32)
    for x in range(S):
        if hi[x] >= lo[x]:
            inside[x] = (v[lo[x]:hi[x] + 1] + entries[x]).max()
    beyond = np.maximum(pre[np.clip(lo, 0, S)], suf[np.clip(hi + 1, 0, S)]) + np.float32(background)
    return np.maximum(inside, beyond).astype(np.float32), inside, beyond.astype(np.float32)


def restate(obs, frames, A, pi, left, right, background):
    """(m (B, T, S) float32, score (B,) float32, decided): the band rule in numpy float32, item by item.  `decided`:
    {'forward' | 'backward': (cells the out-of-band term strictly decides, cells the in-band term strictly decides, cells)}.
    Where an entry outside the band differs from `background` in any bit, every item is NaN in its rows t < F."""
    obs, pi, A = np.asarray(obs, np.float32), np.asarray(pi, np.float32), np.asarray(A, np.float32)
    background = np.float32(background)
    B, T, S = obs.shape
    F = mmc.clamp(frames, T)
    nxt, prv = np.meshgrid(np.arange(S), np.arange(S), indexing='ij')
    outside = (prv < nxt - left) | (prv > nxt + right)
    broken = bool((A.view(np.int32)[outside] != background.view(np.int32)).any())
    states = np.arange(S)
    f_lo, f_hi = np.maximum(states - left, 0), np.minimum(states + right, S - 1)          # prev i of next j
    b_lo, b_hi = np.maximum(states - right, 0), np.minimum(states + left, S - 1)          # next j of prev i
    f_entries = [A[j, f_lo[j]:f_hi[j] + 1] for j in range(S)]
    b_entries = [A[b_lo[i]:b_hi[i] + 1, i] for i in range(S)]
    m = np.full((B, T, S), NINF, np.float32)
    score = np.empty((B,), np.float32)
    decided = {'forward': [0, 0, 0], 'backward': [0, 0, 0]}

    def tally(which, inside, beyond):
        decided[which][0] += int((beyond > inside).sum())
        decided[which][1] += int((inside > beyond).sum())
        decided[which][2] += len(inside)

    with np.errstate(invalid='ignore', over='ignore'):
        for b in range(B):
            f = int(F[b])
            if broken or mmc.odd(obs[b, :f]).any() or mmc.odd(pi).any() or (f >= 2 and mmc.odd(A).any()):
                m[b, :f] = np.nan
                score[b] = np.nan
                continue
            alpha = np.empty((f, S), np.float32)
            alpha[0] = obs[b, 0] + pi
            for t in range(1, f):
                inner, inside, beyond = _step(alpha[t - 1], f_entries, f_lo, f_hi, background)
                tally('forward', inside, beyond)
                alpha[t] = obs[b, t] + inner
            beta = np.zeros((S,), np.float32)
            m[b, f - 1] = alpha[f - 1] + beta
            for t in range(f - 2, -1, -1):
                beta, inside, beyond = _step(obs[b, t + 1] + beta, b_entries, b_lo, b_hi, background)
                tally('backward', inside, beyond)
                m[b, t] = alpha[t] + beta
            score[b] = alpha[f - 1].max()
    return m, score, {k: tuple(v) for k, v in decided.items()}


@functools.lru_cache(maxsize=None)
def case(B, T, S, left, right, background, seed=0, grid=None):
    """(obs, frames, A, pi, mmc.loop's (m, score) on the full matrix) of a band problem: `sbc.continuous` scores, or with
    `grid` levels `sbc.grid_scores` and a grid matrix (every sum exact); ragged lengths with F = T and F = 1 present.
    `background` is a key of BACKGROUNDS or a number.  Computed once, never written."""
    bg = np.float32(BACKGROUNDS.get(background, background))
    obs = sbc.grid_scores(B, T, S, grid, seed) if grid else sbc.continuous(B, T, S, seed)
    A = sbc.band_matrix(S, left, right, bg, seed=seed + 1, grid=grid)
    rng = np.random.default_rng(seed + 2)
    pi = (-0.25 * rng.integers(0, grid, size=S) if grid else rng.uniform(-3, 0, size=S)).astype(np.float32)
    frames = mmc.ragged(B, T, seed)
    return obs, frames, A, pi, mmc.loop(obs, frames, A, pi)


def decided_shares(decided):
    """{pass: (share of cells the out-of-band term strictly decides, share the in-band term strictly decides)}."""
    return {k: (out / max(cells, 1), inside / max(cells, 1)) for k, (out, inside, cells) in decided.items()}


# the case that exercises both terms: a background inside the range of the in-band sums
BOTH_TERMS = (3, 6, 64, 3, 2, 'minus_3')


# the two new entries as rows of tests/operand_form_cases.py's table (as mmc.ENTRIES: not in torbi_amd.__all__)
ENTRIES = [
    ofc.Entry('forward_backward_max_banded', [], ofc.OFAP, 'band',
              lambda o, gpu: margins.forward_backward_max_banded(o[ofc.O], o[ofc.F], o[ofc.A], o[ofc.PI], *ofc.BAND), band=True),
    ofc.Entry('max_marginals-band', [], ofc.OFAP, 'band',
              lambda o, gpu: margins.max_marginals(o[ofc.O], batch_frames=o[ofc.F], transition=o[ofc.A], initial=o[ofc.PI],
                                                   log_probs=True, gpu=gpu, route='band'), route=True),
]
ENTRY = {e.name: e for e in ENTRIES}


def form_cases(device):
    """(entry name, operand, form) of every non-plain case of the two entries on `device`."""
    return [(e.name, operand, name) for e in ENTRIES for operand in e.operands for name in e.forms(operand, device)
            if name != 'plain']
