"""Inputs and float64 references shared by tests/test_sample_cpu.py and tests/test_sample_gpu.py (SAMPLING.md)."""
import math

import torch

import torbi_amd
from torbi_amd import posterior

# (B, T, S, band, lengths, seeds) of the two frequency cases; the seeds are those at which the float64 host route alone stays
# below 4 of the 5 the bound allows (tests/test_sample_cpu.py::test_frequencies_follow_the_posteriors asserts that)
FREQUENCY_CASES = [
    (4, 6, 5, None, (6, 3, 1, 6), (0, 1, 2, 3, 4, 5)),
    (4, 8, 9, (1, 2), (8, 4, 1, 8), (0, 1, 2)),
]
FREQUENCY_DRAWS = 4096


def problem(B, T, S, seed, band=None):
    """(obs (B, T, S), A (S, S) [next, prev], pi (S,)) float32 log inputs; `band` = (l, r): A = -inf outside
    j - l <= i <= j + r."""
    g = torch.Generator().manual_seed(seed)
    obs = torch.log_softmax(3 * torch.randn(B, T, S, generator=g), 2)
    A = torch.log_softmax(2 * torch.randn(S, S, generator=g), 0)
    pi = torch.log_softmax(torch.randn(S, generator=g), 0)
    if band is not None:
        j, i = torch.arange(S)[:, None], torch.arange(S)[None, :]
        A = torch.where((i >= j - band[0]) & (i <= j + band[1]), A, torch.full_like(A, -math.inf))
    return obs, A, pi


def uniforms(B, N, T, seed):
    """(B, N, T) float32 uniforms drawn ON THE CPU, so that host and device read the same numbers."""
    return torch.rand((B, N, T), generator=torch.Generator().manual_seed(1000 + seed))


def frames_of(lengths, B, T):
    return torch.full((B,), T, dtype=torch.int32) if lengths is None else torch.tensor(lengths, dtype=torch.int32)


def host(obs, frames, A, pi, u):
    """The float64 host route at the operator level (log inputs as they are): (indices int64, L float64)."""
    uniform = None if A is not None else float(torch.tensor(math.log(1. / obs.shape[2]), dtype=torch.float32))
    return torbi_amd.sampling._host(obs, frames, A, uniform, pi, u)


def reference(obs, frames, A, pi):
    """float64: (a (B, T, S) filtered rows, E (S, S) or None, L (B,), F (B,), gamma (B, T, S))."""
    uniform = None if A is not None else float(torch.tensor(math.log(1. / obs.shape[2]), dtype=torch.float32))
    a, E, L, F = torbi_amd.sampling._filter(obs, frames, A, uniform, pi)
    gamma = posterior._host(obs, frames, A, uniform, pi)[0]
    return a, E, L, F, gamma


def conditional_weights(a, E, F, indices):
    """float64 weights w (B, N, T, S) of every draw and frame t < F_b, conditioned on the draw's OWN j_{t+1} (rows t >= F_b
    are 0)."""
    B, T, S = a.shape
    N = indices.shape[1]
    w = a[:, None].expand(B, N, T, S).clone()
    if E is not None and T > 1:
        nxt = indices[:, :, 1:].to(torch.int64).clamp(0, S - 1)                   # (B, N, T - 1)
        inner = (torch.arange(T - 1)[None, :] < (F - 1)[:, None])[:, None, :, None]
        w[:, :, :-1] = torch.where(inner, w[:, :, :-1] * E[nxt], w[:, :, :-1])
    live = (torch.arange(T)[None, :] < F[:, None])[:, None, :, None]
    return torch.where(live, w, torch.zeros_like(w))


def draw_errors(indices, u, a, E, F):
    """Draw by draw against float64: for the chosen i of every draw and frame t < F_b,
        d = max(0, P64[i-1] - u Z64, u Z64 - P64[i]) / Z64
    -- how far u Z lies outside the chosen state's interval of the float64 prefix sums.  Returns (worst d, all chosen weights
    > 0)."""
    w = conditional_weights(a, E, F, indices)
    B, N, T, S = w.shape
    j = indices.to(torch.int64)
    assert ((j >= 0) & (j < S)).all()
    P = torch.cumsum(w, dim=-1)
    Z = P[..., -1]
    target = torbi_amd.sampling.read_uniforms(u) * Z
    hi = torch.gather(P, 3, j[..., None])[..., 0]
    lo = torch.where(j == 0, torch.zeros_like(hi), torch.gather(P, 3, (j - 1).clamp(0)[..., None])[..., 0])
    d = torch.maximum(torch.zeros_like(Z), torch.maximum(lo - target, target - hi)) / Z
    live = torch.arange(T)[None, None, :] < F[:, None, None]
    chosen = torch.gather(w, 3, j[..., None])[..., 0]
    return float(d[live.expand_as(d)].max()), bool((chosen[live.expand_as(chosen)] > 0).all())


def frequency_ratio(indices, a, E, F, gamma):
    """The largest |f - p| / (sqrt(p (1 - p) / N) + 1 / N) over the empirical marginals against gamma and, with a matrix,
    the empirical pairs against xi_t(j, i) = gamma_{t+1}[j] a_t[i] E[j, i] / sum_i a_t[i] E[j, i]; the bound allows 5."""
    B, N, T = indices.shape
    S = a.shape[2]
    j = indices.to(torch.int64)
    worst = 0.
    for b in range(B):
        Fb = int(F[b])
        for t in range(Fb):
            f = torch.bincount(j[b, :, t], minlength=S).to(torch.float64) / N
            p = gamma[b, t]
            worst = max(worst, float((torch.abs(f - p) / (torch.sqrt(p * (1 - p) / N) + 1. / N)).max()))
            if E is None or t + 1 >= Fb:
                continue
            joint = a[b, t][None, :] * E                                         # [j, i]
            xi = gamma[b, t + 1][:, None] * joint / joint.sum(dim=1, keepdim=True).clamp_min(1e-300)
            f2 = torch.bincount(j[b, :, t + 1] * S + j[b, :, t], minlength=S * S).to(torch.float64).view(S, S) / N
            worst = max(worst, float((torch.abs(f2 - xi) / (torch.sqrt(xi * (1 - xi) / N) + 1. / N)).max()))
    return worst


def tails_repeat(indices, F):
    """Columns t >= F_b repeat j_{F-1}."""
    B, N, T = indices.shape
    last = torch.gather(indices, 2, (F.to(torch.int64) - 1)[:, None, None].expand(B, N, 1))
    tail = torch.arange(T)[None, None, :] >= F[:, None, None]
    return bool((indices == last)[tail.expand_as(indices)].all())
