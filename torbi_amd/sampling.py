"""Posterior path sampling: whole state sequences drawn from P(path | observations) of the HMM that `from_probabilities`
decodes, by forward filtering and backward sampling.

With a_t the unnormalised filtered rows and E = exp(A) ([next, prev]) of POSTERIOR.md ("Scaled recurrence"), draw n of item
b reads u = uniforms[b, n, t] and goes from the last frame down:

    t = F-1:      w[i] = a_{F-1}[i]
    t < F-1:      w[i] = a_t[i] * E[j_{t+1}][i]
    Z = sum_i w[i];  j_t = the smallest i with (w[0] + ... + w[i]) > u * Z  and  w[i] > 0;
                     if there is none (rounding): the largest i with w[i] > 0

The HIP route is csrc/sample.hpp behind torbi_hip_sample / _uniform (include/torbi_hip.h): the forward half of
`forward_backward`, then one launch that draws every path, one wave per draw.  For a matrix that holds one value outside a
band, csrc/sample_band.hpp behind torbi_hip_sample_band (`forward_sample_banded`, `sample_paths(route=)`) draws at the cost of
the band.  `gpu=None` runs the dense rule in float64 with torch CPU ops.  SAMPLING.md has the contract, the kernels and the
numbers.
"""
import math
from typing import Optional, Tuple

import torch

from . import _lib, band_route, inputs, posterior

MAX_DRAWS = 4096
_MAX_UNIFORM = 1. - 2. ** -24


def forward_sample_workspace_bytes(B: int, T: int, S: int, draws: int, uniform: bool = False) -> int:
    """Bytes of device scratch `forward_sample` needs for a (B, T, S) problem and `draws` paths per item: the layout of
    `forward_backward` and the filter rows (B, T, S) float32 behind it, or with `uniform` (`transition=None` in
    `sample_paths`) the (B, T) float64 row sums alone."""
    return int(_lib.load().torbi_hip_sample_workspace_bytes(B, T, S, int(draws), 1 if uniform else 0))


def _check_draws(draws) -> int:
    if isinstance(draws, bool) or not isinstance(draws, int) or not 1 <= draws <= MAX_DRAWS:
        raise RuntimeError(f'draws must be an integer in [1, {MAX_DRAWS}]; got {draws!r}')
    return draws


def _check_uniforms(uniforms, B, T, draws=None) -> int:
    """The number of draws of a (B, draws, T) tensor of uniforms; raises on any other shape."""
    if uniforms.dim() != 3 or uniforms.shape[0] != B or uniforms.shape[2] != T or (
            draws is not None and uniforms.shape[1] != draws):
        raise RuntimeError(f"uniforms must have shape ({B}, {'draws' if draws is None else draws}, {T}); "
                           f'got {tuple(uniforms.shape)}')
    return _check_draws(int(uniforms.shape[1]))


def _outputs(B, N, T, device):
    return (torch.empty((B, N, T), dtype=torch.int32, device=device), torch.empty((B,), dtype=torch.float32, device=device))


def _run(observation, frames, transition, uniform, initial, uniforms, workspace=None):
    """One call of the HIP route on the device of `observation` (float32, contiguous, log space) and (B,) int32 `frames`
    there: (indices (B, N, T) int32, log_likelihood (B,) float32)."""
    B, T, S = inputs.check_shapes(observation, frames, transition, initial)
    N = _check_uniforms(uniforms, B, T)
    name, model = ('torbi_hip_sample', transition) if uniform is None else ('torbi_hip_sample_uniform', uniform)
    return _lib.run(name, observation, frames, (model, initial, uniforms), _outputs(B, N, T, observation.device),
                    ('torbi_hip_sample_workspace_bytes', (B, T, S, N, 1 if uniform is not None else 0)), (B, T, S, N), workspace)


def forward_sample(observation: torch.Tensor, batch_frames: Optional[torch.Tensor], transition: torch.Tensor,
                   initial: torch.Tensor, uniforms: torch.Tensor, workspace: Optional[torch.Tensor] = None
                   ) -> Tuple[torch.Tensor, torch.Tensor]:
    """Forward filtering, backward sampling on log inputs, on a HIP device: the operator level, like `forward_backward`.

    Args:
        observation: (B, T, S) float32 log scores
        batch_frames: (B,) valid frames per item (clamped to [1, T]); None = all T
        transition: (S, S) float32 log transition matrix [next, prev]
        initial: (S,) float32 log initial distribution
        uniforms: (B, draws, T) float32, 1 <= draws <= 4096: the uniform draw n of item b uses at frame t, read as
            min(max(u, 0), 1 - 2^-24) and NaN as 0
        workspace: optional uint8 device tensor of >= `forward_sample_workspace_bytes(B, T, S, draws)` bytes (a call that
            owns its workspace and its uniforms allocates nothing else but its outputs, so it can be captured into a graph)

    Returns:
        (indices (B, draws, T) int32, log_likelihood (B,) float32) on the device.  Columns t >= F_b repeat the path's last
        state; the log-likelihood is `forward_backward`'s, bit for bit.  An item whose log-likelihood is not finite, and a
        draw whose weights underflow to a sum of 0 at some frame, have -1 in every column.
    """
    if transition is None or initial is None:
        raise RuntimeError('forward_sample needs a transition matrix and an initial distribution')
    B, T, S = inputs.check_shapes(observation, batch_frames, transition, initial)
    _check_uniforms(uniforms, B, T)
    obs, frames = posterior._operands('forward_sample', observation, batch_frames, transition, initial)
    return _run(obs, frames, transition, None, initial, uniforms, workspace)


def forward_sample_banded_workspace_bytes(B: int, T: int, S: int, draws: int, reach_left: int, reach_right: int) -> int:
    """Bytes of device scratch `forward_sample_banded` needs: the layout of `forward_backward_banded` for this band and the
    filter rows (B, T, S) float32 behind it, whatever `draws`."""
    return int(_lib.load().torbi_hip_sample_band_workspace_bytes(B, T, S, int(draws), int(reach_left), int(reach_right)))


def _covered(B, T, S, N, reach_left, reach_right, background, index=0) -> bool:
    """torbi_hip_sample_band_covers: the band route takes this shape, number of draws, band and background."""
    return bool(_lib.load().torbi_hip_sample_band_covers(B, T, S, int(N), int(reach_left), int(reach_right), background,
                                                         index))


def _run_band(observation, frames, transition, initial, uniforms, reach_left, reach_right, background, workspace=None):
    """One call of the band route on the device of `observation` (float32, contiguous, log space) and (B,) int32 `frames`
    there: (indices (B, N, T) int32, log_likelihood (B,) float32)."""
    B, T, S = inputs.check_shapes(observation, frames, transition, initial)
    N = _check_uniforms(uniforms, B, T)
    return _lib.run('torbi_hip_sample_band', observation, frames,
                    (transition, initial, reach_left, reach_right, background, uniforms), _outputs(B, N, T, observation.device),
                    ('torbi_hip_sample_band_workspace_bytes', (B, T, S, N, reach_left, reach_right)), (B, T, S, N), workspace)


def forward_sample_banded(observation: torch.Tensor, batch_frames: Optional[torch.Tensor], transition: torch.Tensor,
                          initial: torch.Tensor, uniforms: torch.Tensor, reach_left: int, reach_right: int,
                          background: float = -math.inf, workspace: Optional[torch.Tensor] = None
                          ) -> Tuple[torch.Tensor, torch.Tensor]:
    """`forward_sample` for a matrix that holds ONE value outside a band, at the cost of the band alone.

    The caller states the band -- transition[j, i] ([next, prev]) with j - reach_left <= i <= j + reach_right -- and
    promises that every entry outside it equals `background` bit for bit, as for `forward_backward_banded`
    (`viterbi.band_over` answers both for a device matrix).  The matrix itself is never looked at on the host; the promise
    is checked on the device without waiting for it: where it is broken, every log-likelihood is NaN and every index -1.

    Args:
        observation, batch_frames, transition, initial, uniforms: as `forward_sample`
        reach_left, reach_right: the band, >= 0
        background: the value outside the band, finite or -inf
        workspace: optional uint8 device tensor of >= `forward_sample_banded_workspace_bytes(B, T, S, draws, reach_left,
            reach_right)` bytes (with it and its own uniforms the call allocates nothing but its outputs and can be
            captured into a graph)

    Returns:
        (indices (B, draws, T) int32, log_likelihood (B,) float32) on the device, as `forward_sample`; the log-likelihood
        is `forward_backward_banded`'s, bit for bit.  Each draw is exact for the model (SAMPLING.md, "Band route"); for
        given uniforms its states are not those of `forward_sample`, which orders the weights of a frame differently.

    Raises where the band route does not cover the call (torbi_hip_sample_band_covers: what `forward_backward_banded`
    covers, and 1 <= draws <= 4096).
    """
    B, T, S = shape = posterior._shapes('forward_sample_banded', observation, batch_frames, transition, initial)
    own = ('draws', _check_uniforms(uniforms, B, T))
    obs, frames, left, right, background = posterior._banded_operands(
        'forward_sample_banded', 'forward_sample', _covered, shape, own, observation, batch_frames, reach_left, reach_right,
        background)
    return _run_band(obs, frames, transition, initial, uniforms, left, right, background, workspace)


# Where 'auto' takes a covered band: the classes of (batch, band width as a share of the row, draws) that
# tools/sample_probe.py --band measured faster than the dense call by more than the spread of the measurement (SAMPLING.md,
# "Band route", timing).  Each entry: (smallest batch, largest batch, diagonals of 1440 states, most draws).  Measured, all on
# 23 diagonals of 1440 states in both forms of the background: 1, 8 and 512 items at one draw (3.5 x, 3.4 x, 5.8 x) and 512
# items at 16 draws (6.0 x).  Anything outside -- a larger batch, a wider band, more draws -- is not measured and stays dense.
_AUTO_BAND = ((1, 512, 23, 1), (512, 512, 23, 16))


def _band_pays(batch: int, states: int, reach_left: int, reach_right: int, draws: int) -> bool:
    return any(low <= batch <= high and band_route.share_within(states, reach_left, reach_right, diagonals) and draws <= most
               for low, high, diagonals, most in _AUTO_BAND)


def _band_plan(trans, original, B, T, S, N, index):
    """`band_route.plan` for this feature: the shape is what torbi_hip_sample_band_covers takes."""
    return band_route.plan(trans, original, _covered, 'torbi_hip_sample_band_covers', dict(batch=B, frames=T, states=S, draws=N),
                           index)


def _band(route, trans, original, B, T, S, N, index):
    """The band `route` takes for the device matrix `trans` (`inputs.device_matrix`; also `original`, the tensor the look is
    remembered with), or None for the dense route (`band_route.choose`)."""
    return band_route.choose(route, *_band_plan(trans, original, B, T, S, N, index),
                             lambda left, right, background: _band_pays(B, S, left, right, N), "sample_paths(route='band')")


def sample_route(transition: Optional[torch.Tensor], batch: int, frames: int, states: int, draws: int = 1, gpu: int = 0,
                 log_probs: bool = False) -> str:
    """The route `sample_paths(..., draws, transition=transition, log_probs=log_probs, gpu=gpu, route='auto')` takes for a
    (batch, frames, states) observation: 'uniform' (no matrix: independent frames), 'band' (one value outside a band, in a
    class of batch, band width and draws that was measured faster: `forward_sample_banded`) or 'dense' (`forward_sample`)."""
    draws = _check_draws(draws)
    if transition is None:
        return 'uniform'
    states = int(states)
    if tuple(transition.shape) != (states, states):
        raise RuntimeError(f'transition must have shape ({states}, {states}); got {tuple(transition.shape)}')
    if gpu is None:
        return 'dense'
    device = inputs._compute_device(gpu)
    trans = inputs.device_matrix(transition, log_probs, device)
    band = _band('auto', trans, trans, int(batch), int(frames), states, draws, device.index or 0)
    return 'dense' if band is None else 'band'


def sample_paths(observation: torch.Tensor, draws: int = 1, batch_frames: Optional[torch.Tensor] = None,
                 transition: Optional[torch.Tensor] = None, initial: Optional[torch.Tensor] = None, log_probs: bool = False,
                 gpu: Optional[int] = None, uniforms: Optional[torch.Tensor] = None,
                 generator: Optional[torch.Generator] = None, route: str = 'dense') -> Tuple[torch.Tensor, torch.Tensor]:
    """`draws` state sequences per item from P(path | observations), and log P(observations) of every item.

    Arguments mean what they mean to `from_probabilities`, defaults included (uniform initial log(1/S + tiny), uniform
    transition log(1/S)), and the inputs go through the same log() and epsilon round trip (torbi_amd/inputs.py), so the
    model is bit for bit the one `from_probabilities` decodes.  `transition=None` draws every frame independently from its
    softmax.  `gpu` is a HIP device index; None computes in float64 on the CPU.  The caller's tensors are not written.

    uniforms: (batch, draws, frames) float32 -- a draw is a function of its item and its own row of uniforms, so equal
        uniforms give equal paths.  None: `torch.rand` on the compute device with `generator`.
    route: which device route a given matrix takes.  'dense' (the default): `forward_sample`, which synchronises nothing and
        whose draws for given uniforms are part of its behaviour.  'band': `forward_sample_banded` on the band
        `viterbi.band_over` finds (one look, with a host synchronisation, per tensor version), raising with the reason where
        the matrix has no covered band.  'auto': the band route where such a band is found, the call is covered and its
        class of batch, band width and draws was measured faster than the dense route (`sample_route` answers which), else
        the dense one.  Both routes draw exactly from the model; for given uniforms their draws differ.  Ignored by
        `transition=None`; `gpu=None` is the float64 dense rule and refuses 'band'.

    Returns:
        (indices (batch, draws, frames) int32, log_likelihood (batch,) float32) on the compute device.  Columns
        t >= batch_frames[b] repeat the path's last state.  An item of total probability 0 has log-likelihood -inf, an item
        that reads a NaN or +inf has NaN; both have -1 in every column of every draw.
    """
    band_route.check_route(route)
    draws = _check_draws(draws)
    B, T, S = inputs.check_shapes(observation, batch_frames, transition, initial)
    if uniforms is not None:
        _check_uniforms(uniforms, B, T, draws)
    if route == 'band' and gpu is None:
        raise RuntimeError("sample_paths(route='band') needs a HIP device: gpu=None is the float64 dense rule")
    if route == 'band' and transition is None:
        raise RuntimeError("sample_paths(route='band'): there is no transition matrix (the uniform model draws every frame "
                           'independently); the band route needs a matrix that holds one value outside a band')
    device = inputs._compute_device(gpu)
    frames = inputs.frames(batch_frames, B, T, device)
    transition, uniform, initial = inputs.model(transition, initial, log_probs, S, device, plain=gpu is not None)
    band = None
    if gpu is not None and uniform is None and route != 'dense':
        # (before the observation is prepared: a matrix without a band raises before anything runs)
        band = _band(route, transition, transition, B, T, S, draws, device.index or 0)
    obs = inputs.observation(observation, log_probs, device)
    if uniforms is None:
        uniforms = torch.rand((B, draws, T), dtype=torch.float32, device=device, generator=generator)
    if gpu is None:
        indices, L = _host(obs, frames, transition, uniform, initial.to(torch.float32), uniforms)
        return indices.to(torch.int32), L.to(torch.float32)
    if band is not None:
        return _run_band(obs, frames, transition, initial, uniforms, *band)
    return _run(obs, frames, transition, uniform, initial, uniforms)


def _filter(obs, frames, transition, uniform, initial):
    """The forward recurrence of `posterior._host` in float64 (`posterior._forward`): (a (B, T, S) unnormalised filtered
    rows -- with `uniform` the rows exp(x - max x) --, E (S, S) or None, L (B,), F (B,) int64)."""
    a, _, _, E, L, F, _ = posterior._forward(obs, frames, transition, uniform, initial)
    return a, E, L, F


def read_uniforms(uniforms: torch.Tensor) -> torch.Tensor:
    """The uniforms as every route reads them: float32 values clamped to [0, 1 - 2^-24], NaN as 0; float64."""
    u = uniforms.detach().to('cpu', torch.float32).to(torch.float64)
    u = torch.where(torch.isnan(u), torch.zeros_like(u), u)
    return u.clamp(0., _MAX_UNIFORM)


def draw(w: torch.Tensor, u: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """The draw rule on weights w (..., S) and uniforms u (...): (j (...) int64, ok (...) bool).  ok is False where the sum
    of the weights is 0 or not finite (j is 0 there)."""
    P = torch.cumsum(w, dim=-1)
    Z = P[..., -1]
    ok = torch.isfinite(Z) & (Z > 0)
    positive = w > 0
    over = positive & (P > (u * Z)[..., None])
    S = w.shape[-1]
    first = torch.argmax(over.to(torch.int8), dim=-1)
    last = S - 1 - torch.argmax(positive.flip(-1).to(torch.int8), dim=-1)
    j = torch.where(over.any(dim=-1), first, last)
    return torch.where(ok, j, torch.zeros_like(j)), ok


def _host(obs, frames, transition, uniform, initial, uniforms):
    """The float64 route with torch CPU ops: the forward recurrence of `posterior._host`, then the draw rule with cumsum.
    (indices (B, N, T) int64, L (B,) float64)."""
    a, E, L, F = _filter(obs, frames, transition, uniform, initial)
    B, T, S = a.shape
    u = read_uniforms(uniforms)
    N = u.shape[1]
    indices = torch.zeros((B, N, T), dtype=torch.int64)
    good = torch.isfinite(L)[:, None].expand(B, N).clone()
    j = torch.zeros((B, N), dtype=torch.int64)
    for t in range(T - 1, -1, -1):
        w = a[:, t, None, :].expand(B, N, S)
        if E is not None and t < T - 1:
            inner = (t < F - 1)[:, None, None]
            w = torch.where(inner, w * E[j], w)
        picked, ok = draw(w, u[:, :, t])
        active = (t <= F - 1)[:, None]
        good &= ok | ~active
        j = torch.where(active, picked, j)
        indices[:, :, t] = j
    last = torch.gather(indices, 2, (F - 1)[:, None, None].expand(B, N, 1))
    indices = torch.where(torch.arange(T)[None, None, :] >= F[:, None, None], last, indices)
    indices = torch.where(good[..., None], indices, torch.full_like(indices, -1))
    return indices, L


def _host_banded(obs, frames, transition, initial, uniforms, reach_left, reach_right, background):
    """The band rule (SAMPLING.md, "Band route") in float64 with torch CPU ops: the forward recurrence of `posterior._host`,
    frame F-1 by the draw rule over the whole row, and every frame t < F-1 by the same rule over the concatenated weights
        [ v[j - l] .. v[j + r],  ebg a_t[0] .. ebg a_t[S-1] ]        v[i] = a_t[i] max(E[j][i] - ebg, 0), j = j_{t+1}
    (slots the matrix clips have weight 0, which the rule never returns).  Where an entry outside the band differs from
    `background` every L is NaN and every index -1.  (indices (B, N, T) int64, L (B,) float64)."""
    a, E, L, F = _filter(obs, frames, transition, None, initial)
    B, T, S = a.shape
    u = read_uniforms(uniforms)
    N = u.shape[1]
    left, right = min(int(reach_left), S - 1), min(int(reach_right), S - 1)
    W = left + right + 1
    bg = torch.tensor(float(background), dtype=torch.float32)
    nxt, prv = torch.arange(S)[:, None], torch.arange(S)[None, :]
    outside = (prv < nxt - left) | (prv > nxt + right)
    A32 = transition.detach().to('cpu', torch.float32)
    if bool((outside & (A32.view(torch.int32) != bg.view(torch.int32))).any()):
        return torch.full((B, N, T), -1, dtype=torch.int64), torch.full_like(L, math.nan)
    ebg = float(torch.exp(bg.to(torch.float64)))
    V = (E - ebg).clamp_min(0.)                                                     # [next, prev]
    offsets = torch.arange(W) - left
    indices = torch.zeros((B, N, T), dtype=torch.int64)
    good = torch.isfinite(L)[:, None].expand(B, N).clone()
    j = torch.zeros((B, N), dtype=torch.int64)
    for t in range(T - 1, -1, -1):
        row = a[:, t, None, :].expand(B, N, S)
        state = j[..., None] + offsets                                              # (B, N, W): the band's slots
        inside = (state >= 0) & (state < S)
        at = state.clamp(0, S - 1)
        v = torch.where(inside, torch.gather(row, 2, at) * V[j[..., None], at], torch.zeros((), dtype=torch.float64))
        slot, ok_band = draw(torch.cat([v, ebg * row], dim=2), u[:, :, t])
        in_band = slot < W
        picked_band = torch.where(in_band, torch.gather(at, 2, slot.clamp(max=W - 1)[..., None])[..., 0], slot - W)
        picked_last, ok_last = draw(row, u[:, :, t])
        last = (t == F - 1)[:, None]
        picked = torch.where(last, picked_last, picked_band)
        ok = torch.where(last, ok_last, ok_band)
        active = (t <= F - 1)[:, None]
        good &= ok | ~active
        j = torch.where(active, picked, j)
        indices[:, :, t] = j
    tail = torch.gather(indices, 2, (F - 1)[:, None, None].expand(B, N, 1))
    indices = torch.where(torch.arange(T)[None, None, :] >= F[:, None, None], tail, indices)
    indices = torch.where(good[..., None], indices, torch.full_like(indices, -1))
    return indices, L
