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

The HIP route is csrc/path_entropy.hpp behind torbi_hip_path_entropy / _uniform (include/torbi_hip.h); for a matrix that
holds one value outside a band, csrc/path_entropy_band.hpp behind torbi_hip_path_entropy_band (`forward_entropy_banded`,
`path_entropy(route=)`) runs the same recursion at the cost of the band, within the same bound.  `gpu=None` and host tensors
run the recursion in float64 with torch CPU ops.  ENTROPY.md has the contract, the kernels and the numbers.

This module is published as the submodule `torbi_amd.entropy`, like `margins` and `paths`; its functions are not in
`torbi_amd.__all__` (every top-level public function that takes an observation has a row in the operand-form table of the
test suite; the rows of these are run from this feature's own tests).
"""
import math
from typing import Optional, Tuple

import torch

from . import _lib, band_route, inputs, posterior

__all__ = ['path_entropy', 'forward_entropy', 'path_entropy_workspace_bytes', 'forward_entropy_banded',
           'path_entropy_banded_workspace_bytes', 'path_entropy_route']


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


def path_entropy_banded_workspace_bytes(B: int, T: int, S: int, reach_left: int, reach_right: int) -> int:
    """Bytes of device scratch `forward_entropy_banded` needs: the band's two sets of diagonals, three scalars per item and
    frame and the promise flag.  No (B, T, S) region and, unlike the dense route, no matrix copies and no operand rows."""
    return int(_lib.load().torbi_hip_path_entropy_band_workspace_size(B, T, S, int(reach_left), int(reach_right)))


def _covered(B, T, S, reach_left, reach_right, background, index=0) -> bool:
    """torbi_hip_path_entropy_band_covers: the band route takes this shape, band and background."""
    return bool(_lib.load().torbi_hip_path_entropy_band_covers(B, T, S, int(reach_left), int(reach_right), background, index))


def _run_band(observation, frames, transition, initial, reach_left, reach_right, background, workspace=None, prefix=False):
    """One call of the band route on the device of `observation` (float32, contiguous, log space)."""
    B, T, S = observation.shape
    device = observation.device
    entropy = torch.empty((B,), dtype=torch.float32, device=device)
    log_likelihood = torch.empty((B,), dtype=torch.float32, device=device)
    rows = torch.empty((B, T), dtype=torch.float32, device=device) if prefix else None
    _lib.run('torbi_hip_path_entropy_band', observation, frames, (transition, initial, reach_left, reach_right, background),
             (entropy, rows, log_likelihood), ('torbi_hip_path_entropy_band_workspace_size', (B, T, S, reach_left, reach_right)),
             (B, T, S), workspace)
    return _answer(entropy, log_likelihood, rows, prefix)


def forward_entropy_banded(observation: torch.Tensor, batch_frames: Optional[torch.Tensor], transition: torch.Tensor,
                           initial: torch.Tensor, reach_left: int, reach_right: int, background: float = -math.inf,
                           workspace: Optional[torch.Tensor] = None, prefix: bool = False) -> Tuple[torch.Tensor, ...]:
    """`forward_entropy` on a HIP device for a matrix that holds ONE value outside a band, at the cost of the band alone.

    The caller states the band -- transition[j, i] ([next, prev]) with j - reach_left <= i <= j + reach_right -- and
    promises that every entry outside it equals `background` bit for bit, as for `forward_backward_banded`
    (`viterbi.band_over` answers both for a device matrix).  The matrix itself is never looked at on the host; the promise
    is checked on the device without waiting for it: where it is broken, every item has a NaN log-likelihood, a NaN entropy
    and NaN prefix entries t < F_b.

    Args:
        observation, batch_frames, transition, initial, prefix: as `forward_entropy`
        reach_left, reach_right: the band, >= 0
        background: the value outside the band, finite or -inf
        workspace: optional uint8 device tensor of >= `path_entropy_banded_workspace_bytes(B, T, S, reach_left,
            reach_right)` bytes, no alignment and no initialisation (then the call allocates nothing but its outputs and can
            be captured into a graph)

    Returns:
        what `forward_entropy` returns, on the device.  The values agree with the dense route's within the bound of
        ENTROPY.md, not bit for bit (the band route defers the division by the row sum), and a single-path model gives 0
        within that bound, not exactly.

    Raises where the band route does not cover the call (torbi_hip_path_entropy_band_covers: up to 4096 states, at most 64
    in-band entries in a matrix row, a background that is neither NaN nor +inf).
    """
    shape = posterior._shapes('forward_entropy_banded', observation, batch_frames, transition, initial)
    obs, frames, left, right, background = posterior._banded_operands(
        'forward_entropy_banded', 'forward_entropy', _covered, shape, (), observation, batch_frames, reach_left, reach_right,
        background)
    return _run_band(obs, frames, transition, initial, left, right, background, workspace, prefix)


# Where 'auto' takes a covered band: the classes of (batch, band width as a share of the row) that
# tools/path_entropy_probe.py measured faster than the dense call on the same inputs by more than the dense call's own
# spread (ENTROPY.md, "Band route", timing).  Each entry: (smallest batch, largest batch, diagonals of 1440 states).
# Measured at 500 frames x 1440 states, each against the dense call on the same inputs: 1, 8 and 512 items on 23 diagonals,
# with -inf and with log(tiny) outside the band; the band route won all six (6.0 x at one item, 8.3 x at 512).  The pitch
# matrix of 175 diagonals lies beyond the 64-entry window of torbi_hip_path_entropy_band_covers and stays dense, as does
# anything else outside -- a larger batch, a wider band -- which is not measured.
_AUTO_BAND = ((1, 512, 23),)


def _band_pays(batch: int, states: int, reach_left: int, reach_right: int) -> bool:
    return any(low <= batch <= high and band_route.share_within(states, reach_left, reach_right, diagonals)
               for low, high, diagonals in _AUTO_BAND)


def _band_plan(trans, original, B, T, S, index):
    """`band_route.plan` for this feature: the shape is what torbi_hip_path_entropy_band_covers takes."""
    return band_route.plan(trans, original, _covered, 'torbi_hip_path_entropy_band_covers', dict(batch=B, frames=T, states=S),
                           index)


def _band(route, trans, original, B, T, S, index):
    """The band `route` takes for the device matrix `trans` (also `original`, the tensor the look is remembered with), or
    None for the dense route (`band_route.choose`)."""
    return band_route.choose(route, *_band_plan(trans, original, B, T, S, index),
                             lambda left, right, background: _band_pays(B, S, left, right), "path_entropy(route='band')")


def path_entropy_route(transition: Optional[torch.Tensor], batch: int, frames: int, states: int, gpu: Optional[int] = 0,
                       log_probs: bool = False) -> str:
    """The route `path_entropy(..., transition=transition, log_probs=log_probs, gpu=gpu, route='auto')` takes for a (batch,
    frames, states) observation: 'uniform' (no matrix), 'band' (one value outside a band, in a class of batch and band width
    that was measured faster: `forward_entropy_banded`) or 'dense' (`forward_entropy`)."""
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


def path_entropy(observation: torch.Tensor, batch_frames: Optional[torch.Tensor] = None,
                 transition: Optional[torch.Tensor] = None, initial: Optional[torch.Tensor] = None, log_probs: bool = False,
                 gpu: Optional[int] = 0, prefix: bool = False, route: str = 'dense') -> Tuple[torch.Tensor, ...]:
    """The entropy of the posterior over whole state paths of every item, and log P(observations) of every item.

    Arguments mean what they mean to `from_probabilities`, defaults included (uniform initial log(1/S + tiny), uniform
    transition log(1/S)), and the inputs go through the same log() and epsilon round trip (torbi_amd/inputs.py), so the
    model is bit for bit the one `from_probabilities` decodes and `state_posteriors` takes.  `gpu` is a HIP device index;
    None computes in float64 on the CPU.  The caller's tensors are not written.

        H, L = path_entropy(observation, gpu=0)
        effective_paths = H.exp()              # 1: one certain path; 2: an even split between two

    route: which device route a given matrix takes; the values agree within the bound of ENTROPY.md on every one.  'dense'
        (the default): `forward_entropy`, which never looks at the matrix and synchronises nothing.  'band':
        `forward_entropy_banded` on the band `viterbi.band_over` finds (one look, with a host synchronisation, per tensor
        version), raising with the reason where the matrix has no covered band.  'auto': the band route where such a band is
        found, the call is covered and its class of batch and band width was measured faster than the dense route
        (`path_entropy_route` answers which), else the dense one.  Ignored by `transition=None` except that 'band' raises
        there; `gpu=None` is the host route and refuses 'band'.

    Returns:
        (entropy (batch,) float32, log_likelihood (batch,) float32) on the compute device, and with `prefix` also
        (batch, frames) float32: the entropy of the path up to each frame given the observations up to it, 0 for
        t >= batch_frames[b].  An item of total probability 0 has log-likelihood -inf and a NaN entropy, an item that reads
        a NaN or +inf has NaN for both.
    """
    band_route.check_route(route)
    B, T, S = inputs.check_shapes(observation, batch_frames, transition, initial)
    if route == 'band' and gpu is None:
        raise RuntimeError("path_entropy(route='band') needs a HIP device: gpu=None is the host route")
    if route == 'band' and transition is None:
        raise RuntimeError("path_entropy(route='band'): there is no transition matrix (the uniform model has a route of its "
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
        H, L, rows = _host(obs, frames, transition, uniform, initial)
        return _answer(H.to(torch.float32), L.to(torch.float32), rows.to(torch.float32), prefix)
    if band is not None:
        return _run_band(obs, frames, transition, initial, *band, None, prefix)
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
