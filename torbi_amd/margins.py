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

The HIP route is csrc/max_marginals.hpp behind torbi_hip_max_marginals / _uniform (include/torbi_hip.h); for a matrix that
holds one value outside a band, csrc/max_marginals_band.hpp behind torbi_hip_max_marginals_band (`forward_backward_max_banded`,
`max_marginals(route=)`) gives the same values at the cost of the band.  `gpu=None` and host tensors run the same recurrences
with torch CPU ops.  MARGINALS.md has the contract, the kernels and the numbers.

This module is published as the submodule `torbi_amd.margins`, like `data`, `synth` and `distributed`; its functions are
not in `torbi_amd.__all__`.  Every top-level public function that takes an observation has a row in the operand-form table
of the test suite; lifting these names to the top level belongs to a later change that adds their rows there (the same
rows are already run from this feature's own tests).
"""
import math
from typing import Optional, Tuple

import torch

from . import _lib, band_route, inputs, posterior
from .k_best import _HOST_CHUNK_ELEMENTS

__all__ = ['max_marginals', 'forward_backward_max', 'max_marginals_workspace_bytes', 'forward_backward_max_banded',
           'max_marginals_banded_workspace_bytes', 'max_marginals_route']


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


def max_marginals_banded_workspace_bytes(B: int, T: int, S: int, reach_left: int, reach_right: int) -> int:
    """Bytes of device scratch `forward_backward_max_banded` needs: the band's diagonals, the alarm words and the verdict
    word.  No (B, T, S) region and, unlike the dense route, no beta rows."""
    return int(_lib.load().torbi_hip_max_marginals_band_workspace_size(B, T, S, int(reach_left), int(reach_right)))


def _covered(B, T, S, reach_left, reach_right, background, index=0) -> bool:
    """torbi_hip_max_marginals_band_covers: the band route takes this shape, band and background."""
    return bool(_lib.load().torbi_hip_max_marginals_band_covers(B, T, S, int(reach_left), int(reach_right), background, index))


def _run_band(observation, frames, transition, initial, reach_left, reach_right, background, workspace=None):
    """One call of the band route on the device of `observation` (float32, contiguous, log space)."""
    B, T, S = observation.shape
    device = observation.device
    outputs = (torch.empty((B, T, S), dtype=torch.float32, device=device), torch.empty((B,), dtype=torch.float32, device=device))
    return _lib.run('torbi_hip_max_marginals_band', observation, frames, (transition, initial, reach_left, reach_right, background),
                    outputs, ('torbi_hip_max_marginals_band_workspace_size', (B, T, S, reach_left, reach_right)), (B, T, S),
                    workspace)


def forward_backward_max_banded(observation: torch.Tensor, batch_frames: Optional[torch.Tensor], transition: torch.Tensor,
                                initial: torch.Tensor, reach_left: int, reach_right: int, background: float = -math.inf,
                                workspace: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """`forward_backward_max` on a HIP device for a matrix that holds ONE value outside a band, at the cost of the band alone.

    The caller states the band -- transition[j, i] ([next, prev]) with j - reach_left <= i <= j + reach_right -- and
    promises that every entry outside it equals `background` bit for bit, as for `forward_backward_banded`
    (`viterbi.band_over` answers both for a device matrix).  The matrix itself is never looked at on the host; the promise
    is checked on the device without waiting for it: where it is broken, every item has NaN in its rows t < F_b and a NaN
    score.

    Args:
        observation, batch_frames, transition, initial: as `forward_backward_max`
        reach_left, reach_right: the band, >= 0
        background: the value outside the band, finite or -inf
        workspace: optional uint8 device tensor of >= `max_marginals_banded_workspace_bytes(B, T, S, reach_left,
            reach_right)` bytes, no alignment and no initialisation (then the call allocates nothing but its outputs and can
            be captured into a graph)

    Returns:
        (marginals (B, T, S) float32, score (B,) float32) on the device: the values of `forward_backward_max`, by `==`
        (rounding is monotone, so the out-of-band candidates of a state are one sum: MARGINALS.md, "Band route").

    Raises where the band route does not cover the call (torbi_hip_max_marginals_band_covers: states % 4 == 0,
    64 <= states <= 3072, reach_left + reach_right + 4 <= 512, a background that is neither NaN nor +inf).
    """
    shape = posterior._shapes('forward_backward_max_banded', observation, batch_frames, transition, initial)
    obs, frames, left, right, background = posterior._banded_operands(
        'forward_backward_max_banded', 'forward_backward_max', _covered, shape, (), observation, batch_frames, reach_left,
        reach_right, background)
    return _run_band(obs, frames, transition, initial, left, right, background, workspace)


# Where 'auto' takes a covered band: the classes of (batch, band width as a share of the row) that
# tools/max_marginals_probe.py measured faster than the dense call on the same inputs by more than the dense call's own
# spread (MARGINALS.md, "Band route", timing).  Each entry: (smallest batch, largest batch, diagonals of 1440 states).
# Measured at 500 frames x 1440 states, each against the dense call on the same inputs: 1, 8 and 512 items on 23 and on 175
# diagonals, with -inf and with log(tiny) outside the band; the band route won every one of the twelve (4.0 x at 512 items
# on 175 diagonals with log(tiny), the narrowest win, to 23 x).  Anything outside -- a larger batch, a wider band -- is not
# measured and stays dense.
_AUTO_BAND = ((1, 512, 175),)


def _band_pays(batch: int, states: int, reach_left: int, reach_right: int) -> bool:
    return any(low <= batch <= high and band_route.share_within(states, reach_left, reach_right, diagonals)
               for low, high, diagonals in _AUTO_BAND)


def _band_plan(trans, original, B, T, S, index):
    """`band_route.plan` for this feature: the shape is what torbi_hip_max_marginals_band_covers takes."""
    return band_route.plan(trans, original, _covered, 'torbi_hip_max_marginals_band_covers', dict(batch=B, frames=T, states=S),
                           index)


def _band(route, trans, original, B, T, S, index):
    """The band `route` takes for the device matrix `trans` (also `original`, the tensor the look is remembered with), or
    None for the dense route (`band_route.choose`)."""
    return band_route.choose(route, *_band_plan(trans, original, B, T, S, index),
                             lambda left, right, background: _band_pays(B, S, left, right), "max_marginals(route='band')")


def max_marginals_route(transition: Optional[torch.Tensor], batch: int, frames: int, states: int, gpu: int = 0,
                        log_probs: bool = False) -> str:
    """The route `max_marginals(..., transition=transition, log_probs=log_probs, gpu=gpu, route='auto')` takes for a (batch,
    frames, states) observation: 'uniform' (no matrix), 'band' (one value outside a band, in a class of batch and band width
    that was measured faster: `forward_backward_max_banded`) or 'dense' (`forward_backward_max`)."""
    if transition is None:
        return 'uniform'
    states = int(states)
    if tuple(transition.shape) != (states, states):
        raise RuntimeError(f'transition must have shape ({states}, {states}); got {tuple(transition.shape)}')
    if gpu is None:
        return 'dense'
    device = inputs._compute_device(gpu)
    trans = inputs.device_matrix(transition, log_probs, device)
    band = _band('auto', trans, trans, int(batch), int(frames), states, device.index or 0)
    return 'dense' if band is None else 'band'


def max_marginals(observation: torch.Tensor, batch_frames: Optional[torch.Tensor] = None,
                  transition: Optional[torch.Tensor] = None, initial: Optional[torch.Tensor] = None, log_probs: bool = False,
                  gpu: Optional[int] = None, route: str = 'dense') -> Tuple[torch.Tensor, torch.Tensor]:
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

    route: which device route a given matrix takes; the values are the same by `==` on every one.  'dense' (the default):
        `forward_backward_max`, which never looks at the matrix and synchronises nothing.  'band':
        `forward_backward_max_banded` on the band `viterbi.band_over` finds (one look, with a host synchronisation, per
        tensor version), raising with the reason where the matrix has no covered band.  'auto': the band route where such a
        band is found, the call is covered and its class of batch and band width was measured faster than the dense route
        (`max_marginals_route` answers which), else the dense one.  Ignored by `transition=None` except that 'band' raises
        there; `gpu=None` is the host route and refuses 'band'.

    Returns:
        (marginals (batch, frames, states) float32, score (batch,) float32) on the compute device, as `forward_backward_max`.
    """
    band_route.check_route(route)
    B, T, S = inputs.check_shapes(observation, batch_frames, transition, initial)
    if route == 'band' and gpu is None:
        raise RuntimeError("max_marginals(route='band') needs a HIP device: gpu=None is the host route")
    if route == 'band' and transition is None:
        raise RuntimeError("max_marginals(route='band'): there is no transition matrix (the uniform model has a route of its "
                           'own); the band route needs a matrix that holds one value outside a band')
    device = inputs._compute_device(gpu)
    frames = inputs.frames(batch_frames, B, T, device)
    transition, uniform, initial = inputs.model(transition, initial, log_probs, S, device, plain=gpu is not None)
    band = None
    if gpu is not None and uniform is None and route != 'dense':
        # (before the observation is prepared: a matrix without a band raises before anything runs)
        band = _band(route, transition, transition, B, T, S, device.index or 0)
    obs = inputs.observation(observation, log_probs, device)
    if gpu is None:
        return _host(obs, frames, transition, uniform, initial)
    if band is not None:
        return _run_band(obs, frames, transition, initial, *band)
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
