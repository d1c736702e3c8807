"""Training an HMM layer: expected transition counts, initial-state counts and a differentiable log-likelihood.

With xi_t(j, i) = P(s_{t-1} = i, s_t = j | obs_b), gamma the state posteriors and g_b a per-item weight (all ones unless
given), A indexed [next, prev]:

    X[j, i] = sum_b g_b sum_{1 <= t < F_b} xi_t(j, i)          I[j] = sum_b g_b gamma_0^b[j]
    dL_b / do_t^b = gamma_t^b        sum_b g_b dL_b / dA = X(g)          sum_b g_b dL_b / dinitial = I(g)

so `log_likelihood(...).sum().backward()` gives gamma, X and I, and one Baum-Welch step normalises X over its columns (next
states of one previous state).  The HIP route is csrc/counts.hpp behind torbi_hip_forward_backward_counts
(include/torbi_hip.h), fed by the passes of `forward_backward`; `gpu=None` and CPU tensors run the same scaled recurrence in
float64 with torch CPU ops.  POSTERIOR.md ("Expected counts") has the contract, the kernels and the numbers.
"""
import ctypes
import math
from typing import Optional, Tuple

import torch

from . import _lib
from .core import _compute_device, _prepared_transition
from .posterior import _check_shapes, _frames, _observation


def expected_counts_workspace_bytes(B: int, T: int, S: int) -> int:
    """Bytes of device scratch `forward_backward_counts` (and `log_likelihood`'s backward) needs for a (B, T, S) problem."""
    return int(_lib.load().torbi_hip_forward_backward_counts_workspace_bytes(B, T, S))


def forward_backward_counts(observation: torch.Tensor, batch_frames: Optional[torch.Tensor], transition: torch.Tensor,
                            initial: torch.Tensor, item_weights: Optional[torch.Tensor] = None,
                            workspace: Optional[torch.Tensor] = None):
    """`forward_backward` plus the weighted expected counts, on log inputs on a HIP device (the operator level).

    Args:
        observation: (B, T, S) float32 log scores
        batch_frames: (B,) valid frames per item (clamped to [1, T]); None = all T
        transition: (S, S) float32 log transition matrix [next, prev]
        initial: (S,) float32 log initial distribution
        item_weights: (B,) weights g_b; None = all ones.  An item with g_b == 0 or a non-finite log-likelihood is skipped.
        workspace: optional uint8 device tensor of >= `expected_counts_workspace_bytes(B, T, S)` bytes (a call that owns
            its workspace allocates nothing else but its outputs, so it can be captured into a graph)

    Returns:
        (posterior (B, T, S), log_likelihood (B,), transition_counts (S, S) [next, prev], initial_counts (S,)), float32 on
        the device; posterior and log_likelihood are bit for bit those of `forward_backward`
    """
    if transition is None or initial is None:
        raise RuntimeError('forward_backward_counts needs a transition matrix and an initial distribution')
    B, T, S = _check_shapes(observation, batch_frames, transition, initial)
    if item_weights is not None and tuple(item_weights.shape) != (B,):
        raise RuntimeError(f'item_weights must have shape ({B},); got {tuple(item_weights.shape)}')
    if not torch.cuda.is_available():
        raise RuntimeError('torbi_amd.forward_backward_counts needs a HIP device (expected_counts(gpu=None) runs on the CPU)')
    device = observation.device if observation.is_cuda else torch.device('cuda', torch.cuda.current_device())
    obs = observation.to(device=device, dtype=torch.float32).contiguous()
    return _run_counts(obs, _frames(batch_frames, B, T, device), transition, initial, item_weights, workspace)


def _run_counts(observation, frames, transition, initial, item_weights, workspace):
    B, T, S = observation.shape
    device = observation.device
    lib = _lib.load()
    posterior = torch.empty((B, T, S), dtype=torch.float32, device=device)
    loglik = torch.empty((B,), dtype=torch.float32, device=device)
    counts = torch.zeros((S, S), dtype=torch.float32, device=device)
    initial_counts = torch.zeros((S,), dtype=torch.float32, device=device)
    if B == 0:
        return posterior, loglik, counts, initial_counts
    need = lib.torbi_hip_forward_backward_counts_workspace_bytes(B, T, S)
    if workspace is None:
        workspace = torch.empty((need,), dtype=torch.uint8, device=device)
    elif (workspace.device != device or workspace.dtype != torch.uint8 or workspace.numel() < need
          or not workspace.is_contiguous()):
        raise RuntimeError(f'workspace must be a contiguous uint8 tensor of >= {need} bytes on {device}')
    index = device.index if device.index is not None else torch.cuda.current_device()
    stream = ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)
    trans = transition.to(device=device, dtype=torch.float32).contiguous()
    init = initial.to(device=device, dtype=torch.float32).contiguous()
    weights = None if item_weights is None else item_weights.to(device=device, dtype=torch.float32).contiguous()
    _lib.check(lib.torbi_hip_forward_backward_counts(
        observation.data_ptr(), frames.data_ptr(), trans.data_ptr(), init.data_ptr(),
        None if weights is None else weights.data_ptr(), posterior.data_ptr(), loglik.data_ptr(), counts.data_ptr(),
        initial_counts.data_ptr(), workspace.data_ptr(), workspace.numel(), B, T, S, index, stream),
        'torbi_hip_forward_backward_counts')
    return posterior, loglik, counts, initial_counts


def expected_counts(observation: torch.Tensor, batch_frames: Optional[torch.Tensor] = None,
                    transition: Optional[torch.Tensor] = None, initial: Optional[torch.Tensor] = None,
                    log_probs: bool = False, gpu: Optional[int] = None) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """Expected transition and initial-state counts (the E-step of Baum-Welch) and log P(observations) of every item.

    Arguments mean what they mean to `state_posteriors` (and `from_probabilities`), defaults and preprocessing included;
    `transition=None` runs the dense route on a matrix filled with fl(log(1/S)).  `gpu` is a HIP device index; None
    computes in float64 on the CPU.  An item whose log-likelihood is not finite adds nothing to the counts.

    Returns:
        (transition_counts (S, S) [next, prev], initial_counts (S,), log_likelihood (B,)), float32 on the compute device.
        transition_counts[j, i] is the expected number of steps from state i to state j; one M-step divides each column by
        its sum.
    """
    B, T, S = _check_shapes(observation, batch_frames, transition, initial)
    device = torch.device('cpu') if gpu is None else _compute_device(gpu)
    tiny = torch.finfo(torch.float32).tiny
    frames = _frames(batch_frames, B, T, device)
    # state_posteriors' defaults and preprocessing (posterior.py), element by element
    if initial is None:
        initial = torch.full((S,), math.log((1. / S) + tiny), dtype=torch.float32, device=device)
    else:
        if not log_probs:
            initial = torch.log(initial)
        initial = initial.to(device)
    if transition is None:
        uniform = float(torch.tensor(math.log(1. / S), dtype=torch.float32))
        transition = torch.full((S, S), uniform, dtype=torch.float32, device=device)
    elif gpu is None:
        transition = (transition if log_probs else torch.log(transition)).to(device)
    else:
        transition = _prepared_transition(transition, log_probs, device)
    obs = _observation(observation, log_probs, device, gpu is None)
    if gpu is None:
        _, L, X, I = _host_counts(obs, frames, transition.to(torch.float32), initial.to(torch.float32), None)
        return X.to(torch.float32), I.to(torch.float32), L.to(torch.float32)
    _, L, X, I = _run_counts(obs, frames, transition, initial, None, None)
    return X, I, L


def _host_counts(obs, frames, transition, initial, weights, counts=True):
    """The scaled recurrence of `posterior._host` in float64, keeping every w_t: (gamma, L, X, I) in float64 (X and I None
    unless `counts`).  The forward pass and L are those of `_host`, operation for operation."""
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
    e = torch.exp(x - m[..., None])
    E = torch.exp(transition.to(torch.float64))                                     # [next, prev]
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
    W = torch.zeros((B, T, S), dtype=torch.float64)
    w = torch.zeros((B, S), dtype=torch.float64)
    for t in range(T - 1, -1, -1):
        last = (F - 1 == t)[:, None]
        beta = torch.where(last, torch.ones((B, S), dtype=torch.float64), w @ E)
        ct = c[:, t, None]
        gamma[:, t] = alpha[:, t] * beta / ct
        w = torch.where((t <= F - 1)[:, None], e[:, t] * beta / ct, w)
        W[:, t] = w
    L = torch.where(torch.isnan(L) | (L == math.inf), torch.full_like(L, math.nan), L)
    bad = ~torch.isfinite(L)
    gamma = torch.where(valid[..., None], gamma, torch.zeros_like(gamma))
    gamma = torch.where(bad[:, None, None] & valid[..., None], torch.full_like(gamma, math.nan), gamma)
    if not counts:
        return gamma, L, None, None
    g = torch.ones(B, dtype=torch.float64) if weights is None else weights.detach().to('cpu', torch.float64)
    live = (g != 0) & ~bad                                                          # skipped, not multiplied
    pair = valid[:, 1:] & live[:, None]                                             # (B, T - 1): pair t = 1 .. F - 1
    zero = torch.zeros((), dtype=torch.float64)
    Wp = torch.where(pair[..., None], W[:, 1:], zero)
    Ap = torch.where(pair[..., None], alpha[:, :-1] / c[:, :-1, None] * g[:, None, None], zero)
    X = E * torch.einsum('btj,bti->ji', Wp, Ap)
    I = torch.where(live[:, None], g[:, None] * gamma[:, 0], zero).sum(dim=0)
    return gamma, L, X, I


class _LogLikelihood(torch.autograd.Function):
    @staticmethod
    def forward(ctx, observation, batch_frames, transition, initial):
        B, T, S = _check_shapes(observation, batch_frames, transition, initial)
        ctx.dtypes = (observation.dtype, transition.dtype, initial.dtype)
        ctx.devices = (observation.device, transition.device, initial.device)
        if observation.is_cuda:
            device = observation.device
            frames = _frames(batch_frames, B, T, device)
            obs = observation.detach().to(dtype=torch.float32).contiguous()
            trans = transition.detach().to(device=device, dtype=torch.float32).contiguous()
            init = initial.detach().to(device=device, dtype=torch.float32).contiguous()
            from .posterior import _run
            gamma, L = _run(obs, frames, trans, None, init, None)
            ctx.save_for_backward(obs, frames, trans, init, gamma, L)
            return L
        frames = _frames(batch_frames, B, T, torch.device('cpu'))
        obs, trans, init = (v.detach().to(torch.float64) for v in (observation, transition, initial))
        gamma, L, _, _ = _host_counts(obs, frames, trans, init, None, counts=False)
        ctx.save_for_backward(obs, frames, trans, init, gamma, L)
        return L.to(torch.float64 if observation.dtype == torch.float64 else torch.float32)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad):
        obs, frames, trans, init, gamma, L = ctx.saved_tensors
        need_o, _, need_t, need_i = ctx.needs_input_grad
        g = grad.to(device=gamma.device, dtype=gamma.dtype)
        d_obs = d_trans = d_init = None
        if need_o:
            d_obs = g[:, None, None] * gamma                                        # rows t >= F are 0 in gamma
        if need_t or need_i:
            if need_t:
                if obs.is_cuda:
                    _, _, X, I = _run_counts(obs, frames, trans, init, g.contiguous(), None)
                else:
                    _, _, X, I = _host_counts(obs, frames, trans, init, g)
            else:
                live = (g != 0) & torch.isfinite(L)
                I = torch.where(live[:, None], g[:, None] * gamma[:, 0], torch.zeros((), dtype=gamma.dtype,
                                                                                      device=gamma.device)).sum(dim=0)
                X = None
            # torch's convention: an item whose L is not finite and whose gradient is not zero poisons the parameters
            if bool(((g != 0) & ~torch.isfinite(L)).any()):
                I = torch.full_like(I, math.nan)
                X = None if X is None else torch.full_like(X, math.nan)
            d_trans = None if not need_t else X
            d_init = None if not need_i else I
        dtypes, devices = ctx.dtypes, ctx.devices
        cast = lambda v, k: None if v is None else v.to(device=devices[k], dtype=dtypes[k])
        return cast(d_obs, 0), None, cast(d_trans, 1), cast(d_init, 2)


def log_likelihood(observation: torch.Tensor, batch_frames: Optional[torch.Tensor], transition: torch.Tensor,
                   initial: torch.Tensor) -> torch.Tensor:
    """log P(observations) of every item, differentiable in observation, transition and initial (log inputs, the operator
    level, like `forward_backward`).

    Device tensors run the HIP route: the forward is one `forward_backward` call; the backward is one
    `forward_backward_counts` call with the incoming gradient as item weights, made only when the transition needs a
    gradient.  CPU tensors run the float64 route (the result is float64 for float64 inputs, so `gradcheck` applies).
    Gradients: d/dobservation = g gamma (rows t >= F_b are 0), d/dtransition = X(g), d/dinitial = I(g); a non-finite L_b
    with g_b != 0 makes the transition and initial gradients NaN.  First order only.

    Returns:
        (B,) log-likelihoods
    """
    if transition is None or initial is None:
        raise RuntimeError('log_likelihood needs a transition matrix and an initial distribution')
    return _LogLikelihood.apply(observation, batch_frames, transition, initial)
