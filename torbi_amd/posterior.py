"""Per-frame state posteriors and sequence log-likelihoods: the forward-backward algorithm on the HMM that
`from_probabilities` decodes.

For t < F_b (log space, A indexed [next, prev]):

    log alpha_0[j] = initial[j] + o_0[j]          log alpha_t[j] = o_t[j] + logsumexp_i (A[j, i] + log alpha_{t-1}[i])
    log beta_{F-1}[j] = 0                         log beta_t[i]  = logsumexp_j (A[j, i] + o_{t+1}[j] + log beta_{t+1}[j])
    L_b = logsumexp_j log alpha_{F-1}[j]          gamma_t[j]     = exp(log alpha_t[j] + log beta_t[j] - L_b)

The HIP route is csrc/forward_backward.hpp behind torbi_hip_forward_backward / _uniform (include/torbi_hip.h); `gpu=None`
runs the same scaled recurrence in float64 with torch CPU ops.  POSTERIOR.md has the contract, the kernels and the numbers.
"""
import ctypes
import math
from typing import Optional, Tuple

import torch

from . import _lib
from .core import _compute_device, _host_log, _prepared_transition
from .viterbi import epsilon_clamp_, log_epsilon_clamp


def forward_backward_workspace_bytes(B: int, T: int, S: int) -> int:
    """Bytes of device scratch `forward_backward` needs for a (B, T, S) problem (either route)."""
    return int(_lib.load().torbi_hip_forward_backward_workspace_bytes(B, T, S))


def _check_shapes(observation, batch_frames, transition, initial):
    """(B, T, S) of a call; raises before anything is launched or computed unless batch_frames is (B,), transition (S, S)
    and initial (S,) (None: the default of that argument).  The kernels read exactly those extents."""
    if observation.dim() != 3:
        raise RuntimeError(f'observation must have shape (batch, frames, states); got {tuple(observation.shape)}')
    B, T, S = observation.shape
    if T < 1 or S < 1:
        raise RuntimeError('observation needs at least one frame and one state')
    if batch_frames is not None and tuple(batch_frames.shape) != (B,):
        raise RuntimeError(f'batch_frames must have shape ({B},); got {tuple(batch_frames.shape)}')
    if transition is not None and tuple(transition.shape) != (S, S):
        raise RuntimeError(f'transition must have shape ({S}, {S}); got {tuple(transition.shape)}')
    if initial is not None and tuple(initial.shape) != (S,):
        raise RuntimeError(f'initial must have shape ({S},); got {tuple(initial.shape)}')
    return B, T, S


def _frames(batch_frames, B, T, device):
    if batch_frames is None:
        return torch.full((B,), T, dtype=torch.int32, device=device)
    return batch_frames.to(device=device, dtype=torch.int32).contiguous()


def _run(observation, batch_frames, transition, uniform, initial, workspace):
    """One call of the HIP route on the device of `observation` (float32, contiguous, log space)."""
    B, T, S = _check_shapes(observation, batch_frames, transition, initial)
    device = observation.device
    lib = _lib.load()
    posterior = torch.empty((B, T, S), dtype=torch.float32, device=device)
    loglik = torch.empty((B,), dtype=torch.float32, device=device)
    if B == 0:
        return posterior, loglik
    need = lib.torbi_hip_forward_backward_workspace_bytes(B, T, S)
    if workspace is None:
        workspace = torch.empty((need,), dtype=torch.uint8, device=device)
    elif (workspace.device != device or workspace.dtype != torch.uint8 or workspace.numel() < need
          or not workspace.is_contiguous()):
        raise RuntimeError(f'workspace must be a contiguous uint8 tensor of >= {need} bytes on {device}')
    index = device.index if device.index is not None else torch.cuda.current_device()
    stream = ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)
    frames = batch_frames.to(device=device, dtype=torch.int32).contiguous()
    init = initial.to(device=device, dtype=torch.float32).contiguous()
    if uniform is None:
        trans = transition.to(device=device, dtype=torch.float32).contiguous()
        _lib.check(lib.torbi_hip_forward_backward(
            observation.data_ptr(), frames.data_ptr(), trans.data_ptr(), init.data_ptr(), posterior.data_ptr(),
            loglik.data_ptr(), workspace.data_ptr(), workspace.numel(), B, T, S, index, stream), 'torbi_hip_forward_backward')
    else:
        _lib.check(lib.torbi_hip_forward_backward_uniform(
            observation.data_ptr(), frames.data_ptr(), ctypes.c_float(uniform), init.data_ptr(), posterior.data_ptr(),
            loglik.data_ptr(), workspace.data_ptr(), workspace.numel(), B, T, S, index, stream),
            'torbi_hip_forward_backward_uniform')
    return posterior, loglik


def forward_backward(observation: torch.Tensor, batch_frames: Optional[torch.Tensor], transition: torch.Tensor,
                     initial: torch.Tensor, workspace: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """Forward-backward on log inputs, on a HIP device: the operator level, like `decode`.

    Args:
        observation: (B, T, S) float32 log scores
        batch_frames: (B,) valid frames per item (clamped to [1, T]); None = all T
        transition: (S, S) float32 log transition matrix [next, prev]
        initial: (S,) float32 log initial distribution
        workspace: optional uint8 device tensor of >= `forward_backward_workspace_bytes(B, T, S)` bytes (a call that
            owns its workspace allocates nothing else but its outputs, so it can be captured into a graph)

    Returns:
        (posterior (B, T, S) float32, log_likelihood (B,) float32) on the device; rows t >= F_b are 0
    """
    if transition is None or initial is None:
        raise RuntimeError('forward_backward needs a transition matrix and an initial distribution')
    B, T, S = _check_shapes(observation, batch_frames, transition, initial)
    if not torch.cuda.is_available():
        raise RuntimeError('torbi_amd.forward_backward needs a HIP device (state_posteriors(gpu=None) runs on the CPU)')
    device = observation.device if observation.is_cuda else torch.device('cuda', torch.cuda.current_device())
    obs = observation.to(device=device, dtype=torch.float32).contiguous()
    return _run(obs, _frames(batch_frames, B, T, device), transition, None, initial, workspace)


def state_posteriors(observation: torch.Tensor, batch_frames: Optional[torch.Tensor] = None,
                     transition: Optional[torch.Tensor] = None, initial: Optional[torch.Tensor] = None,
                     log_probs: bool = False, gpu: Optional[int] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """P(state_t = j | all frames) of every frame, and log P(observations) of every item.

    Arguments mean what they mean to `from_probabilities`, defaults included (uniform initial log(1/S + tiny), uniform
    transition log(1/S)), and the inputs go through the same log() and epsilon round trip, so the model is bit for bit the
    one `from_probabilities` decodes.  `transition=None` takes the closed form of a uniform matrix (beta is constant over
    states).  `gpu` is a HIP device index; None computes in float64 on the CPU.  The caller's tensors are not written.

    Returns:
        (posterior (batch, frames, states) float32, log_likelihood (batch,) float32) on the compute device.  Rows
        t >= batch_frames[b] are 0; an item of total probability 0 has log-likelihood -inf and NaN rows, an item that reads
        a NaN or +inf has NaN for both.
    """
    B, T, S = _check_shapes(observation, batch_frames, transition, initial)
    device = torch.device('cpu') if gpu is None else _compute_device(gpu)
    tiny = torch.finfo(torch.float32).tiny
    frames = _frames(batch_frames, B, T, device)
    # from_probabilities' defaults and preprocessing (core.py), element by element
    if initial is None:
        initial = torch.full((S,), math.log((1. / S) + tiny), dtype=torch.float32, device=device)
    else:
        if not log_probs:
            initial = torch.log(initial)
        initial = initial.to(device)
    uniform = None
    if transition is None:
        uniform = float(torch.tensor(math.log(1. / S), dtype=torch.float32))
    elif gpu is None:
        transition = (transition if log_probs else torch.log(transition)).to(device)
    else:
        transition = _prepared_transition(transition, log_probs, device)
    obs = _observation(observation, log_probs, device, gpu is None)
    if gpu is None:
        return _host(obs, frames, transition, uniform, initial.to(torch.float32))
    return _run(obs, frames, transition, uniform, initial, None)


def _observation(observation, log_probs, device, host):
    """log() unless `log_probs`, the move to `device` as float32 and the epsilon round trip, on a copy."""
    tiny = torch.finfo(torch.float32).tiny
    if host:
        x = observation if log_probs else torch.log(observation)
        x = x.to(device=device, dtype=torch.float32)
        if x.data_ptr() == observation.data_ptr():
            x = x.clone()
        torch.exp_(x)
        x += tiny
        torch.log_(x)
        return x.contiguous()
    clamped = None
    if not log_probs:
        if observation.device == device:
            clamped = log_epsilon_clamp(observation.contiguous())
        if clamped is None:
            observation = _host_log(observation)
    if clamped is not None:
        return clamped
    x = observation.to(device=device, dtype=torch.float32)
    if x.data_ptr() == observation.data_ptr():
        x = x.clone()
    x = x.contiguous()
    epsilon_clamp_(x)
    return x


def _host(obs, frames, transition, uniform, initial):
    """gpu=None: the scaled recurrence of the HIP route in float64 (torch CPU ops), returned as float32."""
    B, T, S = _check_shapes(obs, frames, transition, initial)
    o = obs.to(torch.float64)
    pi = initial.to(torch.float64)
    F = frames.to(torch.int64).clamp(1, T)
    t_index = torch.arange(T)
    valid = t_index[None, :] < F[:, None]                                          # (B, T)
    x = o.clone()
    x[:, 0] += pi
    m = torch.amax(x, dim=2)                                                        # NaN propagates
    m = torch.where(m == -math.inf, torch.zeros_like(m), m)
    e = torch.exp(x - m[..., None])                                                 # (B, T, S) in [0, 1] (or NaN)
    if uniform is not None:
        s = e.sum(dim=2)
        gamma = e / s[..., None]
        lse = m + torch.log(s)
        lse[:, 1:] += float(uniform)
        L = torch.where(valid, lse, torch.zeros_like(lse)).sum(dim=1)
    else:
        E = torch.exp(transition.to(torch.float64))                                 # [next, prev]
        alpha = torch.zeros((B, T, S), dtype=torch.float64)
        c = torch.zeros((B, T), dtype=torch.float64)
        alpha[:, 0] = e[:, 0]
        c[:, 0] = alpha[:, 0].sum(dim=1)
        for t in range(1, T):
            u = e[:, t] * (alpha[:, t - 1] @ E.T)
            prev = c[:, t - 1, None]
            alpha[:, t] = torch.where(prev == 0, u * 0., u / prev)
            c[:, t] = alpha[:, t].sum(dim=1)
        L = torch.where(valid, torch.log(c) + m, torch.zeros_like(m)).sum(dim=1)
        gamma = torch.zeros((B, T, S), dtype=torch.float64)
        w = torch.zeros((B, S), dtype=torch.float64)
        for t in range(T - 1, -1, -1):
            last = (F - 1 == t)[:, None]
            beta = torch.where(last, torch.ones((B, S), dtype=torch.float64), w @ E)
            ct = c[:, t, None]
            gamma[:, t] = alpha[:, t] * beta / ct
            w = torch.where((t <= F - 1)[:, None], e[:, t] * beta / ct, w)
    L = torch.where(torch.isnan(L) | (L == math.inf), torch.full_like(L, math.nan), L)
    bad = ~torch.isfinite(L)
    gamma = torch.where(valid[..., None], gamma, torch.zeros_like(gamma))
    gamma = torch.where(bad[:, None, None] & valid[..., None], torch.full_like(gamma, math.nan), gamma)
    return gamma.to(torch.float32), L.to(torch.float32)
