"""Path entropy: the entropy, in nats, of the posterior over whole state paths, on the HMM that `from_probabilities` decodes.

    H_b = - sum over every path q of item b of  P(q | o_b) log P(q | o_b)

`exp(H)` is the effective number of paths that were in play: the sequence-level confidence that per-frame posteriors cannot
give (their frame entropies only bound H from above).  It has a forward-only recursion (Hernando, Crespi and Cybenko 2005;
the entropy semiring).  In log space, A indexed [next, prev], F the item's frames clamped to [1, T], -inf a zero
probability, with E = exp(A), G = E o A (0 where A = -inf), p_t the filtered distribution and xlogx(0) = 0:

    h_0[j] = 0
    u_{t-1}[i] = p_{t-1}[i] h_{t-1}[i] - xlogx(p_{t-1}[i])
    d = E p_{t-1}        D2 = E u_{t-1}        D3 = G p_{t-1}
    h_t[j] = log d[j] + (D2[j] - D3[j]) / d[j]                  (0 where d[j] = 0: no path reaches j)
    p_t    = normalise(exp(o_t - m_t) * d)                      (the scaled forward step; L accumulates log c_t + m_t)
    prefix_t = sum_j u_t[j]                                     (the entropy of q_0 .. q_t given o_0 .. o_t)
    H = prefix_{F-1}

The matrix need not be stochastic.  The value is what the arithmetic gives: it is not clamped at 0.  An item that reads a
NaN or +inf has a NaN log-likelihood, a NaN entropy and NaN prefix entries t < F; an item of total probability 0 has
log-likelihood -inf and the same NaNs.  Prefix entries t >= F are 0.  `transition=None` (the uniform model) makes the frames
independent: prefix_t is the running sum of the entropies of softmax(o_s), with pi + o_0 at s = 0.

The HIP route is csrc/path_entropy.hpp behind torbi_hip_path_entropy / _uniform (include/torbi_hip.h); `gpu=None` and host
tensors run the recursion in float64 with torch CPU ops.  ENTROPY.md has the contract, the kernels and the numbers.

This module is published as the submodule `torbi_amd.entropy`, like `margins` and `paths`; its functions are not in
`torbi_amd.__all__` (every top-level public function that takes an observation has a row in the operand-form table of the
test suite; the rows of these are run from this feature's own tests).
"""
import math
from typing import Optional, Tuple

import torch

from . import _lib, inputs

__all__ = ['path_entropy', 'forward_entropy', 'path_entropy_workspace_bytes']


def path_entropy_workspace_bytes(B: int, T: int, S: int, uniform: bool = False) -> int:
    """Bytes of device scratch `forward_entropy` needs for a (B, T, S) problem: the general route's (two padded copies of
    the matrix, four scalars per item and frame, four operand rows and two rows of partial sums per item), or with `uniform`
    the uniform route's (`transition=None`: two float64 per item and frame).  Neither holds a (B, T, S) region."""
    return int(_lib.load().torbi_hip_path_entropy_workspace_size(B, T, S, 1 if uniform else 0))


def _answer(entropy, log_likelihood, prefix_rows, prefix):
    return (entropy, log_likelihood, prefix_rows) if prefix else (entropy, log_likelihood)


def forward_entropy(observation: torch.Tensor, batch_frames: Optional[torch.Tensor], transition: Optional[torch.Tensor],
                    initial: torch.Tensor, workspace: Optional[torch.Tensor] = None, prefix: bool = False
                    ) -> Tuple[torch.Tensor, ...]:
    """Path entropy on log inputs: the operator level, like `decode`.  Runs on the HIP device of `observation`, or on the
    host (in float64, rounded once) for a host tensor.

    Args:
        observation: (B, T, S) float32 log scores
        batch_frames: (B,) valid frames per item (clamped to [1, T]); None = all T
        transition: (S, S) float32 log transition matrix [next, prev]; None = uniform, fl(log(1/S)) everywhere
        initial: (S,) float32 log initial distribution
        workspace: optional uint8 device tensor of >= `path_entropy_workspace_bytes(B, T, S, uniform=transition is None)`
            bytes, no alignment and no initialisation (a call that owns its workspace allocates nothing but its outputs, so
            it can be captured into a graph); ignored on the host
        prefix: also return prefix_t, the entropy of q_0 .. q_t given o_0 .. o_t, for every frame

    Returns:
        (entropy (B,) float32, log_likelihood (B,) float32) where the observation lives, and with `prefix` also
        (B, T) float32, 0 for t >= F_b.
    """
    if initial is None:
        raise RuntimeError('forward_entropy needs an initial distribution')
    B, T, S = inputs.check_shapes(observation, batch_frames, transition, initial)
    uniform = None if transition is not None else float(torch.tensor(math.log(1. / S), dtype=torch.float32))
    if not observation.is_cuda:
        frames = inputs.frames(batch_frames, B, T, torch.device('cpu'))
        H, L, rows = _host(observation.to(torch.float32), frames, transition, uniform, initial)
        return _answer(H.to(torch.float32), L.to(torch.float32), rows.to(torch.float32), prefix)
    frames = inputs.frames(batch_frames, B, T, observation.device)
    return _run(observation.to(torch.float32).contiguous(), frames, transition, uniform, initial, workspace, prefix)


def path_entropy(observation: torch.Tensor, batch_frames: Optional[torch.Tensor] = None,
                 transition: Optional[torch.Tensor] = None, initial: Optional[torch.Tensor] = None, log_probs: bool = False,
                 gpu: Optional[int] = 0, prefix: bool = False) -> Tuple[torch.Tensor, ...]:
    """The entropy of the posterior over whole state paths of every item, and log P(observations) of every item.

    Arguments mean what they mean to `from_probabilities`, defaults included (uniform initial log(1/S + tiny), uniform
    transition log(1/S)), and the inputs go through the same log() and epsilon round trip (torbi_amd/inputs.py), so the
    model is bit for bit the one `from_probabilities` decodes and `state_posteriors` takes.  `gpu` is a HIP device index;
    None computes in float64 on the CPU.  The caller's tensors are not written.

        H, L = path_entropy(observation, gpu=0)
        effective_paths = H.exp()              # 1: one certain path; 2: an even split between two

    Returns:
        (entropy (batch,) float32, log_likelihood (batch,) float32) on the compute device, and with `prefix` also
        (batch, frames) float32: the entropy of the path up to each frame given the observations up to it, 0 for
        t >= batch_frames[b].  An item of total probability 0 has log-likelihood -inf and a NaN entropy, an item that reads
        a NaN or +inf has NaN for both.
    """
    B, T, S = inputs.check_shapes(observation, batch_frames, transition, initial)
    device = inputs._compute_device(gpu)
    frames = inputs.frames(batch_frames, B, T, device)
    transition, uniform, initial = inputs.model(transition, initial, log_probs, S, device, plain=gpu is not None)
    obs = inputs.observation(observation, log_probs, device)
    if gpu is None:
        H, L, rows = _host(obs, frames, transition, uniform, initial)
        return _answer(H.to(torch.float32), L.to(torch.float32), rows.to(torch.float32), prefix)
    return _run(obs, frames, transition, uniform, initial, None, prefix)


def _run(observation, frames, transition, uniform, initial, workspace=None, prefix=False):
    """One call of the HIP route on the device of `observation` (float32, contiguous, log space)."""
    B, T, S = observation.shape
    device = observation.device
    entropy = torch.empty((B,), dtype=torch.float32, device=device)
    log_likelihood = torch.empty((B,), dtype=torch.float32, device=device)
    rows = torch.empty((B, T), dtype=torch.float32, device=device) if prefix else None
    name, model = (('torbi_hip_path_entropy', transition) if uniform is None else ('torbi_hip_path_entropy_uniform', uniform))
    _lib.run(name, observation, frames, (model, initial), (entropy, rows, log_likelihood),
             ('torbi_hip_path_entropy_workspace_size', (B, T, S, 0 if uniform is None else 1)), (B, T, S), workspace)
    return _answer(entropy, log_likelihood, rows, prefix)


def _xlogx(p):
    return torch.where(p > 0, p * torch.log(p), torch.zeros_like(p))


def _host(obs, frames, transition, uniform, initial):
    """The recursion in float64 with torch CPU ops, on the float32 values of its operands: (H (B,), L (B,), prefix (B, T)),
    float64.  `uniform` (not None) takes the closed form of a uniform transition matrix."""
    B, T, S = obs.shape
    o = obs.detach().to('cpu', torch.float32).to(torch.float64)
    pi = initial.detach().to('cpu', torch.float32).to(torch.float64)
    F = frames.detach().to('cpu', torch.int64).clamp(1, T)
    valid = torch.arange(T)[None, :] < F[:, None]                                   # (B, T)
    x = o.clone()
    x[:, 0] += pi
    m = torch.amax(x, dim=2) if B else x.new_zeros((0, T))                          # NaN propagates
    m = torch.where(m == -math.inf, torch.zeros_like(m), m)
    z = x - m[..., None]
    e = torch.exp(z)                                                                # (B, T, S) in [0, 1] (or NaN)
    zero = torch.zeros((), dtype=torch.float64)
    if uniform is not None:
        c = e.sum(dim=2)
        lse = m + torch.log(c)
        lse[:, 1:] += float(uniform)
        terms = lse
        w = torch.where(e > 0, z * e, zero).sum(dim=2)
        rows = torch.where(valid, torch.log(c) - w / c, zero).cumsum(dim=1)
    else:
        A = transition.detach().to('cpu', torch.float32).to(torch.float64)          # [next, prev]
        E = torch.exp(A)
        G = torch.where(A == -math.inf, zero, E * A)
        Et, Gt = E.t().contiguous(), G.t().contiguous()
        rows = torch.zeros((B, T), dtype=torch.float64)
        c = torch.zeros((B, T), dtype=torch.float64)
        h = torch.zeros((B, S), dtype=torch.float64)
        p = u = None
        for t in range(T):
            a = e[:, t]
            if t > 0:
                d = p @ Et
                h = torch.where(d == 0, zero, torch.log(d) + (u @ Et - p @ Gt) / d)
                a = a * d
            c[:, t] = a.sum(dim=1)
            ct = c[:, t, None]
            p = torch.where(ct == 0, a * 0., a / ct)
            u = p * h - _xlogx(p)
            rows[:, t] = u.sum(dim=1)
        terms = torch.log(c) + m
    L = torch.where(valid, terms, zero).sum(dim=1)
    L = torch.where(torch.isnan(L) | (L == math.inf), torch.full_like(L, math.nan), L)
    bad = ~torch.isfinite(L)
    rows = torch.where(valid, rows, zero)
    rows = torch.where(bad[:, None] & valid, torch.full_like(rows, math.nan), rows)
    H = rows[torch.arange(B), F - 1]
    return H, L, rows
