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
import math
from typing import Optional, Tuple

import torch

from . import _lib, inputs
from .posterior import _host, _operands, _run


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
    obs, frames = _operands('forward_backward_counts', observation, batch_frames, transition, initial, item_weights)
    return _run(obs, frames, transition, None, initial, workspace, counts=True, item_weights=item_weights)


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
    B, T, S = inputs.check_shapes(observation, batch_frames, transition, initial)
    device = inputs._compute_device(gpu)
    frames = inputs.frames(batch_frames, B, T, device)
    transition, uniform, initial = inputs.model(transition, initial, log_probs, S, device)
    if transition is None:
        transition = torch.full((S, S), uniform, dtype=torch.float32, device=device)
    obs = inputs.observation(observation, log_probs, device)
    if gpu is None:
        _, L, X, I = _host_counts(obs, frames, transition.to(torch.float32), initial.to(torch.float32), None)
        return X.to(torch.float32), I.to(torch.float32), L.to(torch.float32)
    _, L, X, I = _run(obs, frames, transition, None, initial, counts=True)
    return X, I, L


def _host_counts(obs, frames, transition, initial, weights, counts=True):
    """The dense float64 route of `posterior._host` with the counts weighted by `weights` (None = all ones): (gamma, L, X,
    I) in float64 (X and I None unless `counts`)."""
    return _host(obs, frames, transition, None, initial, weights, counts)


class _LogLikelihood(torch.autograd.Function):
    @staticmethod
    def forward(ctx, observation, batch_frames, transition, initial):
        B, T, S = inputs.check_shapes(observation, batch_frames, transition, initial)
        ctx.dtypes = (observation.dtype, transition.dtype, initial.dtype)
        ctx.devices = (observation.device, transition.device, initial.device)
        if observation.is_cuda:
            device = observation.device
            frames = inputs.frames(batch_frames, B, T, device)
            obs = observation.detach().to(dtype=torch.float32).contiguous()
            trans = transition.detach().to(device=device, dtype=torch.float32).contiguous()
            init = initial.detach().to(device=device, dtype=torch.float32).contiguous()
            gamma, L = _run(obs, frames, trans, None, init)
            ctx.save_for_backward(obs, frames, trans, init, gamma, L)
            return L
        frames = inputs.frames(batch_frames, B, T, torch.device('cpu'))
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
                    _, _, X, I = _run(obs, frames, trans, None, init, counts=True, item_weights=g.contiguous())
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
