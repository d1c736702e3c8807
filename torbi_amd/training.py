"""Training an HMM layer: expected transition counts, initial-state counts and a differentiable log-likelihood.

With xi_t(j, i) = P(s_{t-1} = i, s_t = j | obs_b), gamma the state posteriors and g_b a per-item weight (all ones unless
given), A indexed [next, prev]:

    X[j, i] = sum_b g_b sum_{1 <= t < F_b} xi_t(j, i)          I[j] = sum_b g_b gamma_0^b[j]
    dL_b / do_t^b = gamma_t^b        sum_b g_b dL_b / dA = X(g)          sum_b g_b dL_b / dinitial = I(g)

so `log_likelihood(...).sum().backward()` gives gamma, X and I, and one Baum-Welch step normalises X over its columns (next
states of one previous state).  The HIP route is csrc/counts.hpp behind torbi_hip_forward_backward_counts
(include/torbi_hip.h), fed by the passes of `forward_backward`, and for a matrix that is -inf outside a band
csrc/counts_band.hpp behind torbi_hip_forward_backward_counts_band, which gathers the counts of the band's diagonals inside
the one launch of `forward_backward_banded`; `gpu=None` and CPU tensors run the same scaled recurrence in float64 with torch
CPU ops.  POSTERIOR.md ("Expected counts", "Band counts") has the contract, the kernels and the numbers.
"""
import math
from typing import Optional, Tuple

import torch

from . import _lib, band_route, inputs
from .posterior import _banded_operands, _counts_covered, _host, _operands, _run, _run_band, _run_band_counts, _shapes

ROUTES = band_route.ROUTES


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


def expected_counts_banded_workspace_bytes(B: int, T: int, S: int, reach_left: int, reach_right: int) -> int:
    """Bytes of device scratch `forward_backward_counts_banded` needs for a (B, T, S) problem with this band."""
    return int(_lib.load().torbi_hip_forward_backward_counts_band_workspace_bytes(B, T, S, int(reach_left),
                                                                                  int(reach_right)))


def forward_backward_counts_banded(observation: torch.Tensor, batch_frames: Optional[torch.Tensor],
                                   transition: torch.Tensor, initial: torch.Tensor, reach_left: int, reach_right: int,
                                   background: float = -math.inf, item_weights: Optional[torch.Tensor] = None,
                                   workspace: Optional[torch.Tensor] = None):
    """`forward_backward_banded` plus the weighted expected counts inside the band, at the cost of the band alone.

    The band, the promise about `background` and what a broken promise gives (NaN, here in the counts too) are
    `forward_backward_banded`'s.  With a finite background the model has mass outside the band; those counts are a dense
    product and are not computed: the call returns the in-band counts only.

    Args:
        observation, batch_frames, transition, initial, reach_left, reach_right, background: as `forward_backward_banded`
        item_weights: (B,) weights g_b; None = all ones.  An item with g_b == 0 or a non-finite log-likelihood is skipped.
        workspace: optional uint8 device tensor of >= `expected_counts_banded_workspace_bytes(B, T, S, reach_left,
            reach_right)` bytes (then the call allocates nothing but its outputs and can be captured into a graph)

    Returns:
        (posterior (B, T, S), log_likelihood (B,), band_counts (W, S), initial_counts (S,)), float32 on the device.
        band_counts[k, j] = X[j, j - reach_left + k] with X [next, prev] the counts of `forward_backward_counts` and
        W = reach_left + reach_right + 1 (the reaches clamped to S - 1); 0 where the matrix clips the diagonal
        (`band_counts_to_dense` gives X).  posterior and log_likelihood are bit for bit those of `forward_backward_banded`.

    Raises where the band counts route does not cover the call (torbi_hip_forward_backward_counts_band_covers: what
    `forward_backward_banded` covers and 4 W S bytes plus one item's rows within 160 KB of LDS).
    """
    shape = _shapes('forward_backward_counts_banded', observation, batch_frames, transition, initial)
    obs, frames, left, right, background = _banded_operands(
        'forward_backward_counts_banded', 'forward_backward_counts', _counts_covered, shape, (), observation, batch_frames,
        reach_left, reach_right, background, item_weights)
    return _run_band_counts(obs, frames, transition, initial, left, right, background, item_weights, workspace)


def band_counts_to_dense(band_counts: torch.Tensor, reach_left: int, reach_right: int) -> torch.Tensor:
    """The (S, S) matrix [next, prev] of the (W, S) `band_counts` of `forward_backward_counts_banded`: dense[j, j - reach_left
    + k] = band_counts[k, j], zeros outside the band.  On the tensor's device."""
    W, S = band_counts.shape
    left, right = min(int(reach_left), S - 1), min(int(reach_right), S - 1)
    if W != left + right + 1:
        raise RuntimeError(f'band_counts must have {left + right + 1} rows for reach {reach_left}/{reach_right} and {S} '
                           f'states; got {W}')
    j = torch.arange(S, device=band_counts.device)[None, :]
    i = j - left + torch.arange(W, device=band_counts.device)[:, None]
    inside = (i >= 0) & (i < S)
    dense = torch.zeros((S, S), dtype=band_counts.dtype, device=band_counts.device)
    dense[j.expand(W, S)[inside], i[inside]] = band_counts[inside]
    return dense


# The classes of (items, diagonals) route='auto' sends to the band counts route; route='band' takes whatever is covered.
# Measured on the pitch band (W = 23 at 1440 states, close to the largest plane that is covered) at 1, 8 and 512 items, the
# band route beat the dense one 3.0 to 8.1 times with a spread below 2.2 % (POSTERIOR.md "Band counts"), so no class is
# excluded; one that is found to lose goes here, as a function of (reach_left, reach_right, background).
_auto_takes = None


def _counts_band(trans, original, B, T, S, index, route):
    """(reach_left, reach_right) when `route` sends the counts of the device matrix `trans` (`inputs.plain_matrix`;
    `original`: the tensor the look is remembered with) to the band route, else None: the matrix is -inf outside a band (so
    the dense (S, S) result is exactly zero there),
    torbi_hip_forward_backward_counts_band_covers takes it and, for 'auto', the class was measured faster."""
    if route == 'dense':
        return None
    plan = band_route.plan(trans, original, _counts_take,
                           'the band counts route (-inf outside the band, torbi_hip_forward_backward_counts_band_covers)',
                           dict(batch=B, frames=T, states=S), index)
    band = band_route.choose(route, *plan, _auto_takes, "route='band'")
    return None if band is None else band[:2]


def _counts_take(B, T, S, reach_left, reach_right, background, index=0) -> bool:
    return background == -math.inf and _counts_covered(B, T, S, reach_left, reach_right, background, index)


def counts_route(transition: Optional[torch.Tensor], batch: int, frames: int, states: int, gpu: int = 0,
                 log_probs: bool = False) -> str:
    """The route `expected_counts(..., transition=transition, log_probs=log_probs, gpu=gpu, route='auto')` takes for a
    (batch, frames, states) observation: 'band' (`forward_backward_counts_banded`) or 'dense'
    (`forward_backward_counts`)."""
    if transition is None:
        return 'dense'
    if tuple(transition.shape) != (states, states):
        raise RuntimeError(f'transition must have shape ({states}, {states}); got {tuple(transition.shape)}')
    if gpu is None:
        return 'dense'
    device = inputs._compute_device(gpu)
    trans = inputs.device_matrix(transition, log_probs, device)
    band = _counts_band(trans, trans, int(batch), int(frames), states, device.index or 0, 'auto')
    return 'dense' if band is None else 'band'


def expected_counts(observation: torch.Tensor, batch_frames: Optional[torch.Tensor] = None,
                    transition: Optional[torch.Tensor] = None, initial: Optional[torch.Tensor] = None,
                    log_probs: bool = False, gpu: Optional[int] = None, route: str = 'auto'
                    ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """Expected transition and initial-state counts (the E-step of Baum-Welch) and log P(observations) of every item.

    Arguments mean what they mean to `state_posteriors` (and `from_probabilities`), defaults and preprocessing included;
    `transition=None` runs the dense route on a matrix filled with fl(log(1/S)).  `gpu` is a HIP device index; None
    computes in float64 on the CPU.  An item whose log-likelihood is not finite adds nothing to the counts.

    route: which device route a given matrix takes.  'auto': the band route where the matrix is -inf outside a band that
        `forward_backward_counts_banded` covers (`counts_route` answers which), else the dense one; 'dense': always the
        dense route; 'band': the band route, raising where auto would go dense.  The result is the same (S, S) matrix
        either way, exactly zero outside the band; the roundings differ.  Ignored by `gpu=None`.  'auto' and 'band' look at
        the matrix (`viterbi.band_over`: one small kernel and a host synchronisation the first time a tensor version is
        seen, for a dense matrix too when S % 4 == 0 and 64 <= S <= 3072); 'dense' does not.

    Returns:
        (transition_counts (S, S) [next, prev], initial_counts (S,), log_likelihood (B,)), float32 on the compute device.
        transition_counts[j, i] is the expected number of steps from state i to state j; one M-step divides each column by
        its sum.
    """
    band_route.check_route(route)
    B, T, S = inputs.check_shapes(observation, batch_frames, transition, initial)
    device = inputs._compute_device(gpu)
    frames = inputs.frames(batch_frames, B, T, device)
    original = transition
    transition, uniform, initial = inputs.model(transition, initial, log_probs, S, device, plain=gpu is not None)
    if transition is None:
        transition = torch.full((S, S), uniform, dtype=torch.float32, device=device)
    obs = inputs.observation(observation, log_probs, device)
    if gpu is None:
        _, L, X, I = _host_counts(obs, frames, transition.to(torch.float32), initial.to(torch.float32), None)
        return X.to(torch.float32), I.to(torch.float32), L.to(torch.float32)
    if original is None:
        if route == 'band':
            raise RuntimeError("route='band': a uniform transition matrix has no band")
        band = None
    else:
        band = _counts_band(transition, transition, B, T, S, device.index or 0, route)
    if band is not None:
        _, L, Xb, I = _run_band_counts(obs, frames, transition, initial, band[0], band[1], -math.inf)
        return band_counts_to_dense(Xb, band[0], band[1]), I, L
    _, L, X, I = _run(obs, frames, transition, None, initial, counts=True)
    return X, I, L


def _host_counts(obs, frames, transition, initial, weights, counts=True):
    """The dense float64 route of `posterior._host` with the counts weighted by `weights` (None = all ones): (gamma, L, X,
    I) in float64 (X and I None unless `counts`)."""
    return _host(obs, frames, transition, None, initial, weights, counts)


class _LogLikelihood(torch.autograd.Function):
    @staticmethod
    def forward(ctx, observation, batch_frames, transition, initial, route):
        B, T, S = inputs.check_shapes(observation, batch_frames, transition, initial)
        ctx.dtypes = (observation.dtype, transition.dtype, initial.dtype)
        ctx.devices = (observation.device, transition.device, initial.device)
        ctx.band = None
        if observation.is_cuda:
            device = observation.device
            frames = inputs.frames(batch_frames, B, T, device)
            obs = observation.detach().to(dtype=torch.float32).contiguous()
            trans = inputs.plain_matrix(transition.detach().to(device))
            init = initial.detach().to(device=device, dtype=torch.float32).contiguous()
            ctx.band = _counts_band(trans, transition, B, T, S, device.index or 0, route)
            if ctx.band is not None:
                gamma, L = _run_band(obs, frames, trans, init, ctx.band[0], ctx.band[1], -math.inf)
            else:
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
        need_o, _, need_t, need_i, _ = ctx.needs_input_grad
        g = grad.to(device=gamma.device, dtype=gamma.dtype)
        d_obs = d_trans = d_init = None
        if need_o:
            d_obs = g[:, None, None] * gamma                                        # rows t >= F are 0 in gamma
        if need_t or need_i:
            if need_t:
                if ctx.band is not None:
                    left, right = ctx.band
                    _, _, Xb, I = _run_band_counts(obs, frames, trans, init, left, right, -math.inf, g.contiguous())
                    X = band_counts_to_dense(Xb, left, right)
                elif obs.is_cuda:
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
        return cast(d_obs, 0), None, cast(d_trans, 1), cast(d_init, 2), None


def log_likelihood(observation: torch.Tensor, batch_frames: Optional[torch.Tensor], transition: torch.Tensor,
                   initial: torch.Tensor, route: str = 'auto') -> torch.Tensor:
    """log P(observations) of every item, differentiable in observation, transition and initial (log inputs, the operator
    level, like `forward_backward`).

    Device tensors run the HIP route: the forward is one `forward_backward` call; the backward is one
    `forward_backward_counts` call with the incoming gradient as item weights, made only when the transition needs a
    gradient.  CPU tensors run the float64 route (the result is float64 for float64 inputs, so `gradcheck` applies).
    Gradients: d/dobservation = g gamma (rows t >= F_b are 0), d/dtransition = X(g), d/dinitial = I(g); a non-finite L_b
    with g_b != 0 makes the transition and initial gradients NaN.  First order only.

    route: as `expected_counts` -- where a device matrix is -inf outside a band the band routes cover, 'auto' and 'band'
    make the forward one `forward_backward_banded` call and the backward one `forward_backward_counts_banded` call (the
    transition gradient is the (S, S) matrix either way, zero outside the band).  Ignored by CPU tensors.  'auto' and 'band'
    look at the matrix in the forward (`viterbi.band_over`: one small kernel and a host synchronisation per new tensor
    version, so once per step of a training loop that updates the matrix); `route='dense'` keeps the forward free of
    host synchronisation.

    Returns:
        (B,) log-likelihoods
    """
    if transition is None or initial is None:
        raise RuntimeError('log_likelihood needs a transition matrix and an initial distribution')
    band_route.check_route(route)
    return _LogLikelihood.apply(observation, batch_frames, transition, initial, route)
