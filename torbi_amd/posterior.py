"""Per-frame state posteriors and sequence log-likelihoods: the forward-backward algorithm on the HMM that
`from_probabilities` decodes.

For t < F_b (log space, A indexed [next, prev]):

    log alpha_0[j] = initial[j] + o_0[j]          log alpha_t[j] = o_t[j] + logsumexp_i (A[j, i] + log alpha_{t-1}[i])
    log beta_{F-1}[j] = 0                         log beta_t[i]  = logsumexp_j (A[j, i] + o_{t+1}[j] + log beta_{t+1}[j])
    L_b = logsumexp_j log alpha_{F-1}[j]          gamma_t[j]     = exp(log alpha_t[j] + log beta_t[j] - L_b)

The HIP route is csrc/forward_backward.hpp behind torbi_hip_forward_backward / _uniform (include/torbi_hip.h), and for a
matrix that holds one value outside a band csrc/forward_backward_band.hpp behind torbi_hip_forward_backward_band;
`gpu=None` runs the same scaled recurrence in float64 with torch CPU ops.  POSTERIOR.md has the contract, the kernels and
the numbers.
"""
import math
from typing import Optional, Tuple

import torch

from . import _lib, band_route, inputs


def forward_backward_workspace_bytes(B: int, T: int, S: int) -> int:
    """Bytes of device scratch `forward_backward` needs for a (B, T, S) problem (either route)."""
    return int(_lib.load().torbi_hip_forward_backward_workspace_bytes(B, T, S))


def _shapes(what, observation, batch_frames, transition, initial):
    """(B, T, S) of an operator-level call, which needs its matrix and its initial distribution."""
    if transition is None or initial is None:
        raise RuntimeError(f'{what} needs a transition matrix and an initial distribution')
    return inputs.check_shapes(observation, batch_frames, transition, initial)


def _moved(what, observation, batch_frames, B, T, item_weights=None):
    """The observation as contiguous float32 on its HIP device (the current one for a host tensor) and the frames there,
    after the last checks that come before anything runs."""
    if item_weights is not None and tuple(item_weights.shape) != (B,):
        raise RuntimeError(f'item_weights must have shape ({B},); got {tuple(item_weights.shape)}')
    if not torch.cuda.is_available():
        raise RuntimeError(f'torbi_amd.{what} needs a HIP device (state_posteriors / expected_counts with gpu=None run on '
                           'the CPU)')
    device = observation.device if observation.is_cuda else torch.device('cuda', torch.cuda.current_device())
    return observation.to(device=device, dtype=torch.float32).contiguous(), inputs.frames(batch_frames, B, T, device)


def _operands(what, observation, batch_frames, transition, initial, item_weights=None):
    """The front of the operator level (`forward_backward`, `forward_backward_counts`): every check before anything runs,
    then the observation as contiguous float32 on its HIP device (the current one for a host tensor) and the frames."""
    B, T, S = _shapes(what, observation, batch_frames, transition, initial)
    return _moved(what, observation, batch_frames, B, T, item_weights)


def _outputs(B, T, S, device, counts=None):
    """(posterior, log_likelihood) and, with `counts` rows of a counts matrix, (.., counts (rows, S), initial_counts)."""
    out = (torch.empty((B, T, S), dtype=torch.float32, device=device), torch.empty((B,), dtype=torch.float32, device=device))
    if counts is not None:
        out += (torch.zeros((counts, S), dtype=torch.float32, device=device),
                torch.zeros((S,), dtype=torch.float32, device=device))
    return out


def _run(observation, frames, transition, uniform, initial, workspace=None, counts=False, item_weights=None):
    """One call of the HIP route on the device of `observation` (float32, contiguous, log space) and (B,) int32 `frames`
    there: (posterior, log_likelihood), and with `counts` (torbi_hip_forward_backward_counts, dense route only) also
    (transition_counts, initial_counts) weighted by `item_weights` (None = all ones)."""
    B, T, S = inputs.check_shapes(observation, frames, transition, initial)
    if uniform is not None:
        name, model = 'torbi_hip_forward_backward_uniform', (uniform, initial)
    elif not counts:
        name, model = 'torbi_hip_forward_backward', (transition, initial)
    else:
        name, model = 'torbi_hip_forward_backward_counts', (transition, initial, item_weights)
    need = 'torbi_hip_forward_backward_counts_workspace_bytes' if counts else 'torbi_hip_forward_backward_workspace_bytes'
    return _lib.run(name, observation, frames, model, _outputs(B, T, S, observation.device, S if counts else None),
                    (need, (B, T, S)), (B, T, S), workspace)


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
    obs, frames = _operands('forward_backward', observation, batch_frames, transition, initial)
    return _run(obs, frames, transition, None, initial, workspace)


def forward_backward_banded_workspace_bytes(B: int, T: int, S: int, reach_left: int, reach_right: int) -> int:
    """Bytes of device scratch `forward_backward_banded` needs for a (B, T, S) problem with this band."""
    return int(_lib.load().torbi_hip_forward_backward_band_workspace_bytes(B, T, S, int(reach_left), int(reach_right)))


def _covered(B, T, S, reach_left, reach_right, background, index=0) -> bool:
    """torbi_hip_forward_backward_band_covers: the band route takes this shape, band and background."""
    return bool(_lib.load().torbi_hip_forward_backward_band_covers(B, T, S, int(reach_left), int(reach_right), background,
                                                                   index))


def _run_band(observation, frames, transition, initial, reach_left, reach_right, background, workspace=None):
    """One call of the band route on the device of `observation` (float32, contiguous, log space) and (B,) int32
    `frames` there: (posterior, log_likelihood)."""
    B, T, S = inputs.check_shapes(observation, frames, transition, initial)
    return _lib.run('torbi_hip_forward_backward_band', observation, frames,
                    (transition, initial, reach_left, reach_right, background), _outputs(B, T, S, observation.device),
                    ('torbi_hip_forward_backward_band_workspace_bytes', (B, T, S, reach_left, reach_right)), (B, T, S), workspace)


def _counts_covered(B, T, S, reach_left, reach_right, background, index=0) -> bool:
    """torbi_hip_forward_backward_counts_band_covers: the band counts route takes this shape, band and background."""
    return bool(_lib.load().torbi_hip_forward_backward_counts_band_covers(B, T, S, int(reach_left), int(reach_right),
                                                                          background, index))


def _run_band_counts(observation, frames, transition, initial, reach_left, reach_right, background, item_weights=None,
                     workspace=None):
    """One call of the band counts route (torbi_hip_forward_backward_counts_band) on the device of `observation` (float32,
    contiguous, log space) and (B,) int32 `frames` there: (posterior, log_likelihood, band_counts (W, S), initial_counts),
    the counts weighted by `item_weights` (None = all ones)."""
    B, T, S = inputs.check_shapes(observation, frames, transition, initial)
    W = min(reach_left, S - 1) + min(reach_right, S - 1) + 1
    return _lib.run('torbi_hip_forward_backward_counts_band', observation, frames,
                    (transition, initial, reach_left, reach_right, background, item_weights),
                    _outputs(B, T, S, observation.device, W),
                    ('torbi_hip_forward_backward_counts_band_workspace_bytes', (B, T, S, reach_left, reach_right)), (B, T, S),
                    workspace)


def _banded_operands(what, dense, covers, shape, own, observation, batch_frames, reach_left, reach_right, background,
                     item_weights=None, move=True):
    """The front of the stated-band entries (`forward_backward_banded`, `forward_backward_counts_banded`,
    `forward_sample_banded`, `decode_k_best_banded`) behind `_shapes` and the entry's own check, in one order: the band, then
    `covers(B, T, S, [the entry's own argument,] reach_left, reach_right, background)`, then the device operands of `_moved`
    -- or without `move` the observation where it is (an entry that refuses host tensors).  `own` is () or (name, value) of
    that argument, `dense` names the entry that takes any matrix.  Returns (observation, frames, reach_left, reach_right,
    background)."""
    B, T, S = shape
    reach_left, reach_right, background = band_route.stated(reach_left, reach_right, background)
    if B > 0 and not covers(B, T, S, *own[1:], reach_left, reach_right, background):
        said = f' {own[0]}={own[1]},' if own else ''
        raise RuntimeError(f'{what} does not cover B={B}, T={T}, S={S},{said} reach {reach_left}/{reach_right}, '
                           f'background {background} ({dense} takes any matrix)')
    if move:
        obs, frames = _moved(what, observation, batch_frames, B, T, item_weights)
    else:
        obs, frames = observation.to(torch.float32).contiguous(), inputs.frames(batch_frames, B, T, observation.device)
    return obs, frames, reach_left, reach_right, background


def forward_backward_banded(observation: torch.Tensor, batch_frames: Optional[torch.Tensor], transition: torch.Tensor,
                            initial: torch.Tensor, reach_left: int, reach_right: int, background: float = -math.inf,
                            workspace: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """`forward_backward` for a matrix that holds ONE value outside a band, at the cost of the band alone.

    The caller states the band -- transition[j, i] ([next, prev]) with j - reach_left <= i <= j + reach_right -- and
    promises that every entry outside it equals `background` bit for bit (`viterbi.band_over` answers both for a device
    matrix).  The call checks the promise on the device without waiting for it: where it is broken, every log-likelihood
    and every posterior row t < F_b is NaN.

    Args:
        observation, batch_frames, transition, initial: as `forward_backward`
        reach_left, reach_right: the band, >= 0
        background: the value outside the band, finite or -inf
        workspace: optional uint8 device tensor of >= `forward_backward_banded_workspace_bytes(B, T, S, reach_left,
            reach_right)` bytes (then the call allocates nothing but its outputs and can be captured into a graph)

    Returns:
        (posterior (B, T, S) float32, log_likelihood (B,) float32) on the device; rows t >= F_b are 0

    Raises where the band route does not cover the call (torbi_hip_forward_backward_band_covers: up to 4096 states, at most
    64 in-band entries in a matrix row, a background that is neither NaN nor +inf).
    """
    shape = _shapes('forward_backward_banded', observation, batch_frames, transition, initial)
    obs, frames, left, right, background = _banded_operands('forward_backward_banded', 'forward_backward', _covered, shape, (),
                                                            observation, batch_frames, reach_left, reach_right, background)
    return _run_band(obs, frames, transition, initial, left, right, background, workspace)


def _band(route, trans, original, B, T, S, index):
    """(reach_left, reach_right, background) where `route` sends the device matrix `trans` (`inputs.device_matrix`; also
    `original`, the tensor the look is remembered with) to the band route ('auto' takes every band
    torbi_hip_forward_backward_band_covers takes), else None."""
    if route == 'dense':
        return None
    plan = band_route.plan(trans, original, _covered, 'torbi_hip_forward_backward_band_covers', dict(batch=B, frames=T, states=S),
                           index)
    return band_route.choose(route, *plan, None, "state_posteriors(route='band')")


def posterior_route(transition: Optional[torch.Tensor], batch: int, frames: int, states: int, gpu: int = 0,
                    log_probs: bool = False) -> str:
    """The route `state_posteriors(..., transition=transition, log_probs=log_probs, gpu=gpu, route='auto')` takes for a
    (batch, frames, states) observation: 'uniform' (no matrix: the closed form), 'band' (one value outside a band:
    `forward_backward_banded`) or 'dense' (`forward_backward`)."""
    if transition is None:
        return 'uniform'
    if tuple(transition.shape) != (states, states):
        raise RuntimeError(f'transition must have shape ({states}, {states}); got {tuple(transition.shape)}')
    if gpu is None:
        return 'dense'
    device = inputs._compute_device(gpu)
    trans = inputs.device_matrix(transition, log_probs, device)
    return 'dense' if _band('auto', trans, trans, int(batch), int(frames), states, device.index or 0) is None else 'band'


def state_posteriors(observation: torch.Tensor, batch_frames: Optional[torch.Tensor] = None,
                     transition: Optional[torch.Tensor] = None, initial: Optional[torch.Tensor] = None,
                     log_probs: bool = False, gpu: Optional[int] = None, route: str = 'auto'
                     ) -> Tuple[torch.Tensor, torch.Tensor]:
    """P(state_t = j | all frames) of every frame, and log P(observations) of every item.

    Arguments mean what they mean to `from_probabilities`, defaults included (uniform initial log(1/S + tiny), uniform
    transition log(1/S)), and the inputs go through the same log() and epsilon round trip (torbi_amd/inputs.py), so the
    model is bit for bit the one `from_probabilities` decodes.  `transition=None` takes the closed form of a uniform matrix
    (beta is constant over states).  `gpu` is a HIP device index; None computes in float64 on the CPU.  The caller's
    tensors are not written.

    route: which device route a given matrix takes.  'auto': the band route where the matrix holds one value outside a
        band that route covers (`posterior_route` answers which), else the dense one; 'dense': always the dense route;
        'band': the band route, raising where the matrix has no covered band.  Both meet the same tolerance against
        float64; their roundings differ.  Ignored by `gpu=None` and `transition=None`.

    Returns:
        (posterior (batch, frames, states) float32, log_likelihood (batch,) float32) on the compute device.  Rows
        t >= batch_frames[b] are 0; an item of total probability 0 has log-likelihood -inf and NaN rows, an item that reads
        a NaN or +inf has NaN for both.
    """
    band_route.check_route(route)
    B, T, S = inputs.check_shapes(observation, batch_frames, transition, initial)
    device = inputs._compute_device(gpu)
    frames = inputs.frames(batch_frames, B, T, device)
    transition, uniform, initial = inputs.model(transition, initial, log_probs, S, device, plain=gpu is not None)
    obs = inputs.observation(observation, log_probs, device)
    if gpu is None:
        gamma, L, _, _ = _host(obs, frames, transition, uniform, initial.to(torch.float32))
        return gamma.to(torch.float32), L.to(torch.float32)
    band = None if uniform is not None else _band(route, transition, transition, B, T, S, device.index or 0)
    if band is not None:
        return _run_band(obs, frames, transition, initial, *band)
    return _run(obs, frames, transition, uniform, initial)


def _forward(obs, frames, transition, uniform, initial):
    """The forward half of the scaled recurrence in float64 with torch CPU ops: (alpha (B, T, S) unnormalised filtered rows,
    c (B, T) their sums, e (B, T, S) = exp(x - max x), E (S, S) [next, prev], L (B,), F (B,) int64, valid (B, T)).  `uniform`
    (not None) is the closed form of a uniform transition matrix: alpha is e and E None."""
    B, T, S = inputs.check_shapes(obs, frames, transition, initial)
    o = obs.to(torch.float64)
    pi = initial.to(torch.float64)
    F = frames.to(torch.int64).clamp(1, T)
    valid = torch.arange(T)[None, :] < F[:, None]                                   # (B, T)
    x = o.clone()
    x[:, 0] += pi
    m = torch.amax(x, dim=2)                                                        # NaN propagates
    m = torch.where(m == -math.inf, torch.zeros_like(m), m)
    e = torch.exp(x - m[..., None])                                                 # (B, T, S) in [0, 1] (or NaN)
    if uniform is not None:
        alpha, E = e, None
        c = e.sum(dim=2)
        lse = m + torch.log(c)
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
    L = torch.where(torch.isnan(L) | (L == math.inf), torch.full_like(L, math.nan), L)
    return alpha, c, e, E, L, F, valid


def _host(obs, frames, transition, uniform, initial, weights=None, counts=False):
    """The scaled recurrence of the HIP route in float64 with torch CPU ops: (gamma, L, X, I), float64.  `uniform` (not
    None) takes the closed form of a uniform transition matrix.  X (S, S) [next, prev] and I (S,), the expected counts
    weighted by `weights` (None = all ones), are computed only with `counts` (dense route), else None."""
    alpha, c, e, E, L, F, valid = _forward(obs, frames, transition, uniform, initial)
    B, T, S = alpha.shape
    if uniform is not None:
        gamma = e / c[..., None]
    else:
        gamma = torch.zeros((B, T, S), dtype=torch.float64)
        W = torch.zeros((B, T, S), dtype=torch.float64) if counts else None        # every w_t, for the counts
        w = torch.zeros((B, S), dtype=torch.float64)
        for t in range(T - 1, -1, -1):
            last = (F - 1 == t)[:, None]
            beta = torch.where(last, torch.ones((B, S), dtype=torch.float64), w @ E)
            ct = c[:, t, None]
            gamma[:, t] = alpha[:, t] * beta / ct
            w = torch.where((t <= F - 1)[:, None], e[:, t] * beta / ct, w)
            if counts:
                W[:, t] = w
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
