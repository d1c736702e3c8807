"""What tests/test_path_entropy_band_cpu.py and tests/test_path_entropy_band_gpu.py share: band problems (the softmax rows of
`path_entropy_cases.softmax_case` under a `stream_band_cases.band_matrix`), a float64 numpy restatement of the band split of
ENTROPY.md "Band route" written independently of the kernels, the instance rule of csrc/path_entropy_band.hpp and the
operand-form rows of the new entries.

The reference of every comparison is `pec.loop` or `entropy._host` on the FULL matrix; the restatement is itself compared
with `pec.loop` and serves nowhere as a reference.
"""
import functools
import math

import numpy as np

import operand_form_cases as ofc
import path_entropy_cases as pec
import stream_band_cases as sbc
from torbi_amd import _lib, entropy

banded = entropy.forward_entropy_banded           # (the entry under test: without it nothing here means anything)

BACKGROUNDS = {'minus_inf': np.float32(-np.inf), 'log_tiny': sbc.TINY, 'minus_3': np.float32(-3.)}
# csrc/path_entropy_band.hpp
THREADS, WAVES, MAX_GROUP, MAX_LDS, MAX_STATES, MAX_WINDOW = 1024, 16, 4, 159 * 1024, 4096, 64


def clamp_reach(reach, S):
    return min(max(int(reach), 0), S - 1)


def lds_bytes(G, S, left, right):
    """peb::lds_bytes: the fp64 sums of L, the pairs (a, v) by parity with their halos, the wave sums of v and of a, H."""
    halo = max(clamp_reach(left, S), clamp_reach(right, S))
    return G * (WAVES * 8 + 8 + 2 * (S + 2 * halo) * 8 + 2 * WAVES * 8 + 2 * WAVES * 4 + 4) + 16


def items_per_workgroup(B, S, left, right, compute_units=None):
    """The G of pe_band_kernel<G> a call runs: from MAX_GROUP, halved while the rows of G items do not fit the LDS budget,
    then while the launch has fewer workgroups than the device has compute units."""
    if compute_units is None:
        compute_units = _lib.load().torbi_hip_compute_units(0)
    G = MAX_GROUP
    while G > 1 and lds_bytes(G, S, left, right) > MAX_LDS:
        G //= 2
    while G > 1 and -(-B // G) < compute_units:
        G //= 2
    return G


def band_matrix(S, left, right, background, seed=0, left_to_right=False):
    """`sbc.band_matrix` (in-band scores in (-4, 0)); with `left_to_right` the in-band cells with prev > next are -inf."""
    A = sbc.band_matrix(S, left, right, np.float32(background), seed=seed)
    if left_to_right:
        j, i = np.meshgrid(np.arange(S), np.arange(S), indexing='ij')
        A = np.where((i > j) & (i >= j - left) & (i <= j + right), np.float32(-np.inf), A).astype(np.float32)
    return A


@functools.lru_cache(maxsize=None)
def case(B, T, S, left, right, background, seed=0, left_to_right=False):
    """(obs, frames, A, pi) of a band problem: softmax rows of scale 3, ragged lengths with F = T first and F = 1 last, a band
    matrix at the given reaches.  `background` is a key of BACKGROUNDS or a number.  Computed once, never written."""
    bg = np.float32(BACKGROUNDS.get(background, background))
    obs, frames, _, pi = pec.softmax_case(B, T, S, seed, matrix=None)
    return obs, frames, band_matrix(S, left, right, bg, seed + 1, left_to_right), pi


@functools.lru_cache(maxsize=None)
def loop_reference(*key):
    """`pec.loop` on the full matrix of `case(*key)`: (H, L, prefix) float64."""
    return pec.loop(*case(*key))


def host64(obs, frames, A, pi):
    """`entropy._host` on the full matrix: (H, L, prefix) float64 arrays."""
    o, f, a, p = pec.tensors(obs, frames, A, pi)
    return tuple(x.numpy() for x in entropy._host(o, f, a, None, p))


def restate(obs, frames, A, pi, left, right, background):
    """(H, L, prefix) float64 by the band split: per state the in-band diagonals of E - ebg and G - gbg against the previous
    rows, plus ebg and gbg times the sums of those rows.  A broken promise gives NaN in H, L and the prefix entries t < F."""
    obs, A, pi = np.asarray(obs, np.float64), np.asarray(A, np.float32), np.asarray(pi, np.float64)
    B, T, S = obs.shape
    F = pec.clamp(frames, T)
    left, right = clamp_reach(left, S), clamp_reach(right, S)
    W = left + right + 1
    bg = np.float32(background)
    ebg = 0. if np.isneginf(bg) else math.exp(float(bg))
    gbg = 0. if np.isneginf(bg) else ebg * float(bg)
    j = np.arange(S)
    Df, Dg, col = np.zeros((W, S)), np.zeros((W, S)), np.zeros((W, S), np.int64)
    inside = np.zeros((S, S), bool)
    for k in range(W):
        i = j - left + k
        ok = (i >= 0) & (i < S)
        a = A[j[ok], i[ok]].astype(np.float64)
        e = np.exp(a)
        Df[k, ok] = e - ebg
        Dg[k, ok] = np.where(np.isneginf(a), 0., e * np.where(np.isneginf(a), 0., a)) - gbg
        col[k] = np.clip(i, 0, S - 1)                                # (clipped positions hold 0 in Df and Dg)
        inside[j[ok], i[ok]] = True
    broken = bool((A[~inside].view(np.int32) != bg.view(np.int32)).any())
    H, L, prefix = np.zeros(B), np.zeros(B), np.zeros((B, T))
    xlogx = lambda p: np.where(p > 0, p * np.log(np.where(p > 0, p, 1.)), 0.)
    for b in range(B):
        f = int(F[b])
        if broken:
            H[b] = L[b] = prefix[b, :f] = np.nan
            continue
        for t in range(f):
            x = obs[b, t] + (pi if t == 0 else 0.)
            m = x.max()
            e = np.exp(x - m)
            if t == 0:
                a, h = e, np.zeros(S)
            else:
                d = (Df * p[col]).sum(axis=0) + ebg * p.sum()
                D2 = (Df * u[col]).sum(axis=0) + ebg * u.sum()
                D3 = (Dg * p[col]).sum(axis=0) + gbg * p.sum()
                reached = d > 0
                h = np.zeros(S)
                h[reached] = np.log(d[reached]) + (D2[reached] - D3[reached]) / d[reached]
                a = e * d
            c = a.sum()
            p = a / c
            u = p * h - xlogx(p)
            prefix[b, t] = u.sum()
            L[b] += math.log(c) + m
        H[b] = prefix[b, f - 1]
    return H, L, prefix


# the new entries as rows of tests/operand_form_cases.py's table (as pec.ENTRIES: not in torbi_amd.__all__)
ENTRIES = [
    ofc.Entry('forward_entropy_banded', [], ofc.OFAP, 'band',
              lambda o, gpu: banded(o[ofc.O], o[ofc.F], o[ofc.A], o[ofc.PI], *ofc.BAND, prefix=True),
              band=True),
    ofc.Entry('path_entropy-band', [], ofc.OFAP, 'band',
              lambda o, gpu: entropy.path_entropy(o[ofc.O], batch_frames=o[ofc.F], transition=o[ofc.A], initial=o[ofc.PI],
                                                  log_probs=True, gpu=gpu, prefix=True, route='band'), route=True),
]
ENTRY = {e.name: e for e in ENTRIES}


def form_cases(device):
    """(entry name, operand, form) of every non-plain case of the two entries on `device`."""
    return [(e.name, operand, name) for e in ENTRIES for operand in e.operands for name in e.forms(operand, device)
            if name != 'plain']
