"""Inputs and float64 references shared by tests/test_sample_band_cpu.py and tests/test_sample_band_gpu.py (SAMPLING.md,
"Band route")."""
import math

import torch

import torbi_amd

import sample_cases as sc

# (B, T, S, (reach_left, reach_right), background, lengths, seeds) of the two frequency cases; the seeds are those at which
# the float64 band rule alone stays below 4 of the 5 the bound allows
# (tests/test_sample_band_cpu.py::test_frequencies_follow_the_posteriors asserts that)
FREQUENCY_CASES = [
    (4, 8, 9, (1, 2), -math.inf, (8, 4, 1, 8), (0, 1, 2)),
    (4, 6, 8, (1, 1), -3., (6, 3, 1, 6), (0, 1, 2)),
]
FREQUENCY_DRAWS = sc.FREQUENCY_DRAWS


def in_band(S, band):
    j, i = torch.arange(S)[:, None], torch.arange(S)[None, :]
    return (i >= j - band[0]) & (i <= j + band[1])


def problem(B, T, S, seed, band, background=-math.inf):
    """`sc.problem` with A [next, prev] equal to `background` outside j - l <= i <= j + r.  With a finite background the
    in-band entries are raised to at least background + 0.05: entries below the background are outside the contract."""
    obs, A, pi = sc.problem(B, T, S, seed, band)
    if background != -math.inf:
        bg = torch.tensor(background, dtype=torch.float32)
        A = torch.where(in_band(S, band), torch.maximum(A, bg + 0.05), bg)
    return obs, A, pi


def host(obs, frames, A, pi, u, band, background):
    """The float64 band rule at the operator level: (indices int64, L float64)."""
    return torbi_amd.sampling._host_banded(obs, frames, A, pi, u, band[0], band[1], background)


def ebg_of(background):
    return float(torch.exp(torch.tensor(background, dtype=torch.float32).to(torch.float64)))


def conditional_weights(a, E, F, indices, band, background):
    """float64: (w (B, N, T, W + S), state (B, N, T, W)).  w is the concatenated weight vector of every draw and frame
    t < F_b conditioned on the draw's OWN j_{t+1} -- the band part, whose slot k is state j - l + k (weight 0 where the
    matrix clips it), then ebg * a_t --; at t = F_b - 1 the band part is 0 and the second part a_t itself.  Rows t >= F_b
    are 0."""
    B, T, S = a.shape
    N = indices.shape[1]
    left, right = min(band[0], S - 1), min(band[1], S - 1)
    W = left + right + 1
    ebg = ebg_of(background)
    V = (E - ebg).clamp_min(0.)
    nxt = torch.cat([indices[:, :, 1:], indices[:, :, -1:]], dim=2).to(torch.int64).clamp(0, S - 1)      # (B, N, T)
    state = nxt[..., None] + (torch.arange(W) - left)                                # (B, N, T, W)
    inside = (state >= 0) & (state < S)
    at = state.clamp(0, S - 1)
    rows = a[:, None].expand(B, N, T, S)
    zero = torch.zeros((), dtype=torch.float64)
    v = torch.where(inside, torch.gather(rows, 3, at) * V[nxt[..., None], at], zero)
    t = torch.arange(T)[None, None, :, None]
    Fb = F[:, None, None, None]
    v = torch.where(t < Fb - 1, v, zero)
    second = torch.where(t < Fb - 1, ebg * rows, torch.where(t == Fb - 1, rows, zero))
    return torch.cat([v, second], dim=3), torch.where(inside, state, torch.full_like(state, -1))


def draw_errors(indices, u, a, E, F, band, background):
    """Draw by draw against float64.  The chosen state has up to two slots in the concatenated vector: its band slot and
    its whole-row slot.  For each of them that has weight > 0,
        d = max(0, P64[before] - u Z64, u Z64 - P64[slot]) / Z64
    and the smaller is kept (inf where neither has weight > 0).  Returns (worst d, share of the draws taken from the
    whole-row part at frames t < F_b - 1)."""
    w, state = conditional_weights(a, E, F, indices, band, background)
    B, N, T, C = w.shape
    S = a.shape[2]
    W = C - S
    j = indices.to(torch.int64)
    assert ((j >= 0) & (j < S)).all()
    P = torch.cumsum(w, dim=-1)
    Z = P[..., -1]
    target = torbi_amd.sampling.read_uniforms(u) * Z

    def error(slot, valid):
        slot = slot.clamp(0, C - 1)
        hi = torch.gather(P, 3, slot[..., None])[..., 0]
        lo = torch.where(slot == 0, torch.zeros_like(hi), torch.gather(P, 3, (slot - 1).clamp(0)[..., None])[..., 0])
        weight = torch.gather(w, 3, slot[..., None])[..., 0]
        d = torch.maximum(torch.zeros_like(Z), torch.maximum(lo - target, target - hi)) / Z
        return torch.where(valid & (weight > 0), d, torch.full_like(d, math.inf))

    hit = state == j[..., None]                                                      # (B, N, T, W): at most one slot
    d_band = error(torch.argmax(hit.to(torch.int8), dim=-1), hit.any(dim=-1))
    d_row = error(W + j, torch.ones_like(j, dtype=torch.bool))
    d = torch.minimum(d_band, d_row)
    live = (torch.arange(T)[None, None, :] < F[:, None, None]).expand_as(d)
    inner = (torch.arange(T)[None, None, :] < F[:, None, None] - 1).expand_as(d)
    behind = float((d_row < d_band)[inner].double().mean()) if bool(inner.any()) else 0.
    return float(d[live].max()), behind


def pairs_in_band(indices, F, band):
    """No drawn pair (j_{t+1}, j_t), t + 1 < F_b, lies outside the band."""
    T = indices.shape[2]
    if T < 2:
        return True
    nxt, prv = indices[:, :, 1:].long(), indices[:, :, :-1].long()
    inner = (torch.arange(T - 1)[None, :] < (F - 1)[:, None])[:, None, :].expand_as(nxt)
    return bool(((prv >= nxt - band[0]) & (prv <= nxt + band[1]))[inner].all())
