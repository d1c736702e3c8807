"""Max-marginals: the largest log score of any complete path of an item that is in state j at frame t, on the HMM that
`from_probabilities` decodes.

    m[b, t, j] = max over every path q of item b with q_t = j of its log score

One forward and one backward max-plus pass, all sums in float32 with one rounding each, A indexed [next, prev], F the
item's frames clamped to [1, T]:

    alpha_0[j] = fl(o_0[j] + pi[j])
    alpha_t[j] = fl(o_t[j] + max_i fl(alpha_{t-1}[i] + A[j, i]))          1 <= t < F   (the decoder's posterior rows)
    beta_{F-1}[i] = +0
    beta_t[i]  = max_j fl(A[j, i] + fl(o_{t+1}[j] + beta_{t+1}[j]))       0 <= t < F-1
    m_t[j]     = fl(alpha_t[j] + beta_t[j])   for t < F,   -inf   for F <= t < T
    score      = max_j alpha_{F-1}[j]

A maximum of floats does not depend on the order it is taken in, so the values are defined exactly, whatever the route:
only the sign of a zero is not.  `score` is `best_paths(..., k=1)`'s score, and `max_j m_t[j] == score` for every t < F
wherever the sums are exact.  -inf is an ordinary value: a state that no path reaches or leaves has m = -inf.  An item that
reads a NaN or +inf (its observation rows t < F, the initial vector, the matrix when F >= 2) has NaN in every m_t, t < F,
and a NaN score.  Sums of finite inputs that overflow float32 are outside the contract.

The HIP route is csrc/max_marginals.hpp behind torbi_hip_max_marginals / _uniform (include/torbi_hip.h); `gpu=None` and
host tensors run the same recurrences with torch CPU ops.  MARGINALS.md has the contract, the kernels and the numbers.

This module is published as the submodule `torbi_amd.margins`, like `data`, `synth` and `distributed`; its functions are
not in `torbi_amd.__all__`.  Every top-level public function that takes an observation has a row in the operand-form table
of the test suite; lifting these names to the top level belongs to a later change that adds their rows there (the same
rows are already run from this feature's own tests).
"""
import math
from typing import Optional, Tuple

import torch

from . import _lib, inputs
from .k_best import _HOST_CHUNK_ELEMENTS

__all__ = ['max_marginals', 'forward_backward_max', 'max_marginals_workspace_bytes']


def max_marginals_workspace_bytes(B: int, T: int, S: int, uniform: bool = False) -> int:
    """Bytes of device scratch `forward_backward_max` needs for a (B, T, S) problem: the general route's (the matrix
    transposed, two beta rows per item, the alarm words), or with `uniform` the uniform route's (`transition=None`: three
    scalars per item and frame).  Neither holds a (B, T, S) region."""
    return int(_lib.load().torbi_hip_max_marginals_workspace_size(B, T, S, 1 if uniform else 0))


def forward_backward_max(observation: torch.Tensor, batch_frames: Optional[torch.Tensor], transition: Optional[torch.Tensor],
                         initial: torch.Tensor, workspace: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """Max-marginals on log inputs: the operator level, like `decode`.  Runs on the HIP device of `observation`, or on the
    host for a host tensor.

    Args:
        observation: (B, T, S) float32 log scores
        batch_frames: (B,) valid frames per item (clamped to [1, T]); None = all T
        transition: (S, S) float32 log transition matrix [next, prev]; None = uniform, fl(log(1/S)) everywhere
        initial: (S,) float32 log initial distribution
        workspace: optional uint8 device tensor of >= `max_marginals_workspace_bytes(B, T, S, uniform=transition is None)`
            bytes, no alignment and no initialisation (a call that owns its workspace allocates nothing but its outputs, so
            it can be captured into a graph); ignored on the host

    Returns:
        (marginals (B, T, S) float32, score (B,) float32) where the observation lives.  Rows t >= F_b are -inf; an item that
        reads a NaN or +inf has NaN in its rows t < F_b and a NaN score.
    """
    if initial is None:
        raise RuntimeError('forward_backward_max needs an initial distribution')
    B, T, S = inputs.check_shapes(observation, batch_frames, transition, initial)
    uniform = None if transition is not None else float(torch.tensor(math.log(1. / S), dtype=torch.float32))
    if not observation.is_cuda:
        frames = inputs.frames(batch_frames, B, T, torch.device('cpu'))
        return _host(observation.to(torch.float32), frames, transition, uniform, initial)
    frames = inputs.frames(batch_frames, B, T, observation.device)
    return _run(observation.to(torch.float32).contiguous(), frames, transition, uniform, initial, workspace)


def max_marginals(observation: torch.Tensor, batch_frames: Optional[torch.Tensor] = None,
                  transition: Optional[torch.Tensor] = None, initial: Optional[torch.Tensor] = None, log_probs: bool = False,
                  gpu: Optional[int] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """The best path score through every frame and state, and the best path's score.

    Arguments mean what they mean to `from_probabilities`, defaults included (uniform initial log(1/S + tiny), uniform
    transition log(1/S)), and the inputs go through the same log() and epsilon round trip (torbi_amd/inputs.py), so `score`
    is bit for bit `best_paths(..., k=1)`'s and, where the best path is unique, `argmax_j m_t[j]` is the path
    `from_probabilities` returns.  `gpu` is a HIP device index; None computes on the CPU with the same float32 sums.  The
    caller's tensors are not written.

    The gap between the decoded state and the runner-up at the same frame is a path-consistent confidence:

        m, score = max_marginals(observation, gpu=0)
        path = m.argmax(2, keepdim=True)
        gap = m.gather(2, path) - m.topk(2, dim=2).values[..., 1:]

    Returns:
        (marginals (batch, frames, states) float32, score (batch,) float32) on the compute device, as `forward_backward_max`.
    """
    B, T, S = inputs.check_shapes(observation, batch_frames, transition, initial)
    device = inputs._compute_device(gpu)
    frames = inputs.frames(batch_frames, B, T, device)
    transition, uniform, initial = inputs.model(transition, initial, log_probs, S, device, plain=gpu is not None)
    obs = inputs.observation(observation, log_probs, device)
    if gpu is None:
        return _host(obs, frames, transition, uniform, initial)
    return _run(obs, frames, transition, uniform, initial)


def _run(observation, frames, transition, uniform, initial, workspace=None):
    """One call of the HIP route on the device of `observation` (float32, contiguous, log space)."""
    B, T, S = observation.shape
    device = observation.device
    outputs = (torch.empty((B, T, S), dtype=torch.float32, device=device), torch.empty((B,), dtype=torch.float32, device=device))
    name, model = (('torbi_hip_max_marginals', transition) if uniform is None else ('torbi_hip_max_marginals_uniform', uniform))
    return _lib.run(name, observation, frames, (model, initial), outputs,
                    ('torbi_hip_max_marginals_workspace_size', (B, T, S, 0 if uniform is None else 1)), (B, T, S), workspace)


def _max_plus(M, v):
    """out[b, r] = max_c fl(M[r, c] + v[b, c]), chunked over items and rows so that no temporary holds more than
    _HOST_CHUNK_ELEMENTS values."""
    B, S = v.shape
    out = torch.empty((B, S), dtype=torch.float32)
    rstep = max(1, min(S, _HOST_CHUNK_ELEMENTS // S))
    bstep = max(1, _HOST_CHUNK_ELEMENTS // (S * rstep))
    for b0 in range(0, B, bstep):
        b1 = min(B, b0 + bstep)
        for r0 in range(0, S, rstep):
            r1 = min(S, r0 + rstep)
            out[b0:b1, r0:r1] = (M[None, r0:r1, :] + v[b0:b1, None, :]).amax(dim=2)
    return out


def _host(obs, frames, transition, uniform, initial):
    """The recurrences with torch CPU ops in float32.  `uniform` (not None) stands for the float32 fill matrix of that
    value; there the maxima collapse to one scalar per item and frame (max_i fl(x_i + u) = fl(max_i x_i + u)), which gives
    the same values without the (S, S) temporaries."""
    B, T, S = obs.shape
    if B == 0:
        return torch.empty((0, T, S), dtype=torch.float32), torch.empty((0,), dtype=torch.float32)
    obs = obs.detach().to('cpu', torch.float32)
    F = frames.detach().to('cpu', torch.int64).clamp(1, T)
    pi = initial.detach().to('cpu', torch.float32)
    if uniform is None:
        A = transition.detach().to('cpu', torch.float32)
        At = A.t().contiguous()
        u = None
    else:
        u = torch.tensor(uniform, dtype=torch.float32)
    top = int(F.max())
    m = torch.full((B, T, S), -math.inf, dtype=torch.float32)
    m[:, 0] = obs[:, 0] + pi
    for t in range(1, top):
        prev = m[:, t - 1]
        inner = _max_plus(A, prev) if u is None else (prev.amax(dim=1, keepdim=True) + u).expand(B, S)
        m[:, t] = obs[:, t] + inner
    score = m[torch.arange(B), F - 1].amax(dim=1)
    beta = torch.zeros((B, S), dtype=torch.float32)
    for t in range(top - 2, -1, -1):
        w = obs[:, t + 1] + beta
        step = _max_plus(At, w) if u is None else (u + w.amax(dim=1, keepdim=True)).expand(B, S)
        beta = torch.where((F - 1 == t)[:, None], torch.zeros(()), step)
        m[:, t] = m[:, t] + beta
    beyond = torch.arange(T)[None, :] >= F[:, None]                                    # (B, T)
    m[beyond] = -math.inf
    bad = (~(pi < math.inf)).any().expand(B).clone()
    if T > 1:
        bad |= (F >= 2) & ((~(A < math.inf)).any() if u is None else ~(u < math.inf))
    bad |= ((~(obs < math.inf)) & ~beyond[:, :, None]).flatten(1).any(dim=1)
    m[bad[:, None] & ~beyond] = math.nan
    score[bad] = math.nan
    return m, score
