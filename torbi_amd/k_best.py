"""k-best Viterbi decoding: the k best state sequences of every item with their exact scores, on the HMM that
`from_probabilities` decodes (list Viterbi).

Every state j of frame t keeps a list L_t(j) of up to k entries (value, back-pointer (i, r)), all sums in float32, A
indexed [next, prev]:

    L_0(j) = [fl(o_0[j] + pi[j])]
    t >= 1: candidates c = fl(L_{t-1}(i)[r] + A[j, i]) over every prev-state i and rank r of L_{t-1}(i); L_t(j) = the first
            min(k, count) in the order (c descending, i ascending, r ascending), each stored as fl(o_t[j] + c)
    result: the first min(k, S^F) entries (L_{F-1}(j)[r], j, r) in the order (value descending, j ascending, r ascending)

Rank 0 is the existing decoder's path and its score the maximum of the decoder's last posterior row.  The HIP route is
csrc/k_best.hpp behind torbi_hip_k_best / _uniform (include/torbi_hip.h); `gpu=None` and host tensors run the same
recurrence with torch CPU ops.  KBEST.md has the contract, the kernels and the numbers.

A matrix that holds ONE value outside a band (the reference's pitch matrix: 175 diagonals of 1440 states) takes the band
route on the device (csrc/k_best_band.hpp behind torbi_hip_k_best_band*; KBEST.md, "Band route"): every frame in one
launch, a state's list from its in-band prev-states unless an out-of-band candidate could enter it.  `route` chooses; the
outputs are the same bits either way.
"""
import math
from typing import Optional, Tuple

import torch

from . import _lib, band_route, inputs
from .posterior import _banded_operands, _shapes

MAX_K = 32
ROUTES = band_route.ROUTES
# candidates per chunk of next-states on the host route (4-byte values, 8-byte sort indices)
_HOST_CHUNK_ELEMENTS = 1 << 25


def decode_k_best_workspace_bytes(B: int, T: int, S: int, k: int, uniform: bool = False) -> int:
    """Bytes of device scratch `decode_k_best` needs for a (B, T, S) problem and k ranks: the general route's (4 bytes of
    back-pointer per item, frame, state and rank), or with `uniform` the uniform route's (`transition=None`: its pointers
    have no state axis, so it is torbi_hip_k_best_workspace_bytes(B, T, 1, k)).  The general size serves both routes."""
    return int(_lib.load().torbi_hip_k_best_workspace_bytes(B, T, 1 if uniform else S, k))


def _check_k(k) -> int:
    if isinstance(k, bool) or not isinstance(k, int) or not 1 <= k <= MAX_K:
        raise RuntimeError(f'k must be an integer in [1, {MAX_K}]; got {k!r}')
    return k


def decode_k_best(observation: torch.Tensor, batch_frames: Optional[torch.Tensor], transition: Optional[torch.Tensor],
                  initial: torch.Tensor, k: int, workspace: Optional[torch.Tensor] = None, route: str = 'auto'
                  ) -> Tuple[torch.Tensor, torch.Tensor]:
    """k-best Viterbi decoding on log inputs: the operator level, like `decode`.  Runs on the HIP device of `observation`,
    or on the host for a host tensor.

    Args:
        observation: (B, T, S) float32 log scores
        batch_frames: (B,) valid frames per item (clamped to [1, T]); None = all T
        transition: (S, S) float32 log transition matrix [next, prev]; None = uniform, fl(log(1/S)) everywhere
        initial: (S,) float32 log initial distribution
        k: paths per item, 1 <= k <= 32
        workspace: optional uint8 device tensor of >= `decode_k_best_workspace_bytes(B, T, S, k, uniform=transition is
            None)` bytes (a call that owns its workspace allocates nothing else but its outputs, so it can be captured into
            a graph); a call that takes the band route needs `decode_k_best_banded_workspace_bytes` instead, and 'auto'
            takes that route only where the workspace holds as much
        route: 'auto', 'dense' or 'band': which device route a given matrix takes.  'band' raises RuntimeError, naming
            the reason, where the band route cannot take the call.  'auto' here, at the operator level, does what a call
            that may be captured into a graph can do: it takes the band route only for a matrix whose structure is already
            known -- `k_best_route`, `best_paths`, a `route='band'` call or `decode` has looked at this tensor version --
            and never looks itself (a look is a small kernel, a host synchronisation and a first device allocation).
            The bits are the same on every route.  Ignored on the host; `transition=None` takes the uniform route under
            'auto' and 'dense', and 'band' raises there too.

    Returns:
        (indices (B, k, T) int32, scores (B, k) float32) where the observation lives.  Columns t >= F_b repeat the path's
        last state; ranks beyond S^F_b have score -inf and index -1; an item that reads a NaN or +inf has NaN scores and -1
        indices.
    """
    k = _check_k(k)
    band_route.check_route(route, ValueError)
    if initial is None:
        raise RuntimeError('decode_k_best needs an initial distribution')
    B, T, S = inputs.check_shapes(observation, batch_frames, transition, initial)
    uniform = None if transition is not None else float(torch.tensor(math.log(1. / S), dtype=torch.float32))
    if not observation.is_cuda:
        frames = inputs.frames(batch_frames, B, T, torch.device('cpu'))
        return _host(observation.to(torch.float32), frames, transition, uniform, initial, k)
    frames = inputs.frames(batch_frames, B, T, observation.device)
    obs = observation.to(torch.float32).contiguous()
    return _routed(obs, frames, transition, transition, uniform, initial, k, route, workspace, look=False)


def best_paths(observation: torch.Tensor, k: int, batch_frames: Optional[torch.Tensor] = None,
               transition: Optional[torch.Tensor] = None, initial: Optional[torch.Tensor] = None, log_probs: bool = False,
               gpu: Optional[int] = None, route: str = 'auto') -> Tuple[torch.Tensor, torch.Tensor]:
    """The k best state sequences of every item and their log scores.

    Arguments mean what they mean to `from_probabilities`, defaults included (uniform initial log(1/S + tiny), uniform
    transition log(1/S)), and the inputs go through the same log() and epsilon round trip (torbi_amd/inputs.py), so rank 0
    is bit for bit the path `from_probabilities` returns.  `gpu` is a HIP device index; None computes on the CPU with the
    same float32 sums.  The caller's tensors are not written.  `route` ('auto', 'dense' or 'band') is `decode_k_best`'s:
    the band route for a matrix that holds one value outside a band, with the same bits; ignored with `gpu=None`;
    'band' raises RuntimeError where that route cannot take the call, `transition=None` included.

    Returns:
        (indices (batch, k, frames) int32, scores (batch, k) float32) on the compute device, as `decode_k_best`.
    """
    k = _check_k(k)
    band_route.check_route(route, ValueError)
    B, T, S = inputs.check_shapes(observation, batch_frames, transition, initial)
    device = inputs._compute_device(gpu)
    frames = inputs.frames(batch_frames, B, T, device)
    transition, uniform, initial = inputs.model(transition, initial, log_probs, S, device, plain=gpu is not None)
    obs = inputs.observation(observation, log_probs, device)
    if gpu is None:
        return _host(obs, frames, transition, uniform, initial, k)
    return _routed(obs, frames, transition, transition, uniform, initial, k, route)


def decode_k_best_banded_workspace_bytes(B: int, T: int, S: int, k: int, reach_left: int, reach_right: int) -> int:
    """Bytes of device scratch `decode_k_best_banded` needs: `decode_k_best_workspace_bytes`'s layout with the
    (reach_left + reach_right + 1) * S diagonals in place of the transposed matrix, and a verdict word."""
    return int(_lib.load().torbi_hip_k_best_band_workspace_bytes(B, T, S, k, int(reach_left), int(reach_right)))


def _covered(B, T, S, k, reach_left, reach_right, background, index=0) -> bool:
    """torbi_hip_k_best_band_covers: the band route takes this shape, k, band and background."""
    return bool(_lib.load().torbi_hip_k_best_band_covers(B, T, S, k, int(reach_left), int(reach_right), background, index))


# (k, diagonals of 1440 states) up to which tools/k_best_probe.py measured the band route faster than the dense one by more
# than the dense route's spread (KBEST.md, "Band route"): k <= 4 up to 175 diagonals, k <= 8 up to 23; at k = 8 and 175
# diagonals the band route is the slower one
_AUTO_BAND = ((4, 175), (8, 23))


def _band_pays(k: int, states: int, reach_left: int, reach_right: int) -> bool:
    """Where 'auto' takes a covered band: for a (k, width) inside what the probe measured faster, the width as the band's
    share of the matrix.  Anything beyond -- k above 8, a band that holds more than 175 / 1440 of a row -- is not
    measured and stays dense."""
    return any(k <= top and band_route.share_within(states, reach_left, reach_right, diagonals) for top, diagonals in _AUTO_BAND)


def _band_plan(trans: torch.Tensor, original: torch.Tensor, B: int, T: int, S: int, k: int, index: int, look: bool = True):
    """`band_route.plan` for this feature: the shape is what torbi_hip_k_best_band_covers takes; without `look` only a
    structure that is already known counts."""
    return band_route.plan(trans, original, _covered, 'torbi_hip_k_best_band_covers', dict(batch=B, frames=T, states=S, k=k),
                           index, look)


def _routed(obs, frames, transition, original, uniform, initial, k, route, workspace=None, look=True):
    """The device call of `decode_k_best` / `best_paths` by `route` (prepared inputs; `original`: the tensor the look at the
    matrix is remembered with -- `best_paths`' device matrix itself, `decode_k_best`'s caller's log matrix --; `look`: whether
    'auto' may look at a matrix it has not seen)."""
    B, T, S = obs.shape
    if uniform is not None and route == 'band':
        raise RuntimeError("k-best decoding with route='band': there is no transition matrix (the uniform model), which the "
                           'uniform route decodes; the band route needs a matrix that holds one value outside a band')
    if uniform is None and route != 'dense' and B > 0:
        trans = inputs.plain_matrix(transition.to(obs.device))

        def pays(left, right, background):      # ... and the caller's workspace must also hold the band layout
            return _band_pays(k, S, left, right) and (
                workspace is None or workspace.numel() >= decode_k_best_banded_workspace_bytes(B, T, S, k, left, right))

        band = band_route.choose(route, *_band_plan(trans, original, B, T, S, k, obs.device.index or 0, look or route == 'band'),
                                 pays, "k-best decoding with route='band'")
        if band is not None:
            return _run_band(obs, frames, trans, initial, k, *band, workspace)
    return _run(obs, frames, transition, uniform, initial, k, workspace)


def k_best_route(transition: Optional[torch.Tensor], batch: int, frames: int, states: int, k: int, gpu: Optional[int] = 0,
                 log_probs: bool = False) -> str:
    """The route `best_paths(observation, k, transition=transition, log_probs=log_probs, gpu=gpu, route='auto')` takes for a
    (batch, frames, states) observation: 'host' (`gpu=None`), 'uniform' (no matrix), 'band' (one value outside a band the
    band kernels cover: `decode_k_best_banded`) or 'dense'."""
    k = _check_k(k)
    if gpu is None:
        return 'host'
    if transition is None:
        return 'uniform'
    states = int(states)
    if tuple(transition.shape) != (states, states):
        raise ValueError(f'transition must be ({states}, {states})')
    device = inputs._compute_device(gpu)
    trans = inputs.device_matrix(transition, log_probs, device)
    band, why = _band_plan(trans, trans, int(batch), int(frames), states, k, device.index or 0)
    pays = lambda left, right, background: _band_pays(k, states, left, right)
    return 'dense' if band_route.choose('auto', band, why, pays, 'k_best_route') is None else 'band'


def decode_k_best_banded(observation: torch.Tensor, batch_frames: Optional[torch.Tensor], transition: torch.Tensor,
                         initial: torch.Tensor, k: int, reach_left: int, reach_right: int, background: float = -math.inf,
                         workspace: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """`decode_k_best` on a HIP device for a matrix that holds ONE value outside a band, at the cost of the band.

    The caller states the band -- transition[j, i] ([next, prev]) with j - reach_left <= i <= j + reach_right -- and
    promises that every entry outside it equals `background` bit for bit (`viterbi.band_over` answers both for a device
    matrix).  The call checks the promise on the device without waiting for it: where it is broken, every item gets NaN
    scores and -1 indices.  Otherwise the result is `decode_k_best`'s, bit for bit.

    Args:
        observation, batch_frames, transition, initial, k: as `decode_k_best`
        reach_left, reach_right: the band, >= 0
        background: the value outside the band, finite or -inf
        workspace: optional uint8 device tensor of >= `decode_k_best_banded_workspace_bytes(B, T, S, k, reach_left,
            reach_right)` bytes (then the call allocates nothing but its outputs and can be captured into a graph)

    Raises RuntimeError where the band route does not cover the call (torbi_hip_k_best_band_covers: states % 4 == 0,
    64 .. 3072 states, reach_left + reach_right + 4 <= 512, 8 k (states + reach_left + reach_right) <= 159 * 1024, a
    background that is neither NaN nor +inf).
    """
    k = _check_k(k)
    shape = _shapes('decode_k_best_banded', observation, batch_frames, transition, initial)
    if not observation.is_cuda:
        raise RuntimeError('decode_k_best_banded runs on a HIP device; decode_k_best takes host tensors')
    obs, frames, left, right, background = _banded_operands(
        'decode_k_best_banded', 'decode_k_best', _covered, shape, ('k', k), observation, batch_frames, reach_left, reach_right,
        background, move=False)
    return _run_band(obs, frames, transition, initial, k, left, right, background, workspace)


def _outputs(B, k, T, device):
    return (torch.empty((B, k, T), dtype=torch.int32, device=device), torch.empty((B, k), dtype=torch.float32, device=device))


def _run_band(observation, frames, transition, initial, k, reach_left, reach_right, background, workspace=None):
    """One call of the band route on the device of `observation` (float32, contiguous, log space)."""
    B, T, S = observation.shape
    return _lib.run('torbi_hip_k_best_band', observation, frames, (transition, initial, reach_left, reach_right, background),
                    _outputs(B, k, T, observation.device),
                    ('torbi_hip_k_best_band_workspace_bytes', (B, T, S, k, reach_left, reach_right)), (B, T, S, k), workspace)


def _run(observation, frames, transition, uniform, initial, k, workspace=None):
    """One call of the HIP route on the device of `observation` (float32, contiguous, log space).  The uniform route's
    pointers have no state axis (`decode_k_best_workspace_bytes`)."""
    B, T, S = observation.shape
    name, model = ('torbi_hip_k_best', transition) if uniform is None else ('torbi_hip_k_best_uniform', uniform)
    return _lib.run(name, observation, frames, (model, initial), _outputs(B, k, T, observation.device),
                    ('torbi_hip_k_best_workspace_bytes', (B, T, S if uniform is None else 1, k)), (B, T, S, k), workspace)


def _host(obs, frames, transition, uniform, initial, k):
    """The recurrence with torch CPU ops in float32.  A stable descending sort over the candidates of a next-state, flattened
    as i * n + r (n: entries per list of the previous frame), gives the tie order exactly.  `uniform` (not None) stands
    for the float32 fill matrix of that value.  A chunk of items and next-states holds at most _HOST_CHUNK_ELEMENTS
    candidates; what is kept is the current frame's lists, every item's final lists and the int32 back-pointers
    (4 B T S k bytes, as the device route)."""
    B, T, S = obs.shape
    if B == 0:
        return torch.empty((0, k, T), dtype=torch.int32), torch.empty((0, k), dtype=torch.float32)
    obs = obs.detach().to('cpu', torch.float32)
    F = frames.detach().to('cpu', torch.int64).clamp(1, T)
    pi = initial.detach().to('cpu', torch.float32)
    A = (torch.full((S, S), uniform, dtype=torch.float32) if uniform is not None
         else transition.detach().to('cpu', torch.float32))
    L = (obs[:, 0] + pi)[:, :, None]                                       # (B, S, n): L_t(j) of every item
    ns, pointers = [1], [None]                                             # n_t; (B, S, n_t) int32 i * n_{t-1} + r
    final = [L[b].clone() if F[b] == 1 else None for b in range(B)]        # (S, n) of L_{F_b - 1}
    for t in range(1, int(F.max())):
        n = L.shape[2]
        m = min(k, S * n)
        per = S * n                                                        # candidates of one (item, next-state)
        jstep = max(1, min(S, _HOST_CHUNK_ELEMENTS // per))
        bstep = max(1, _HOST_CHUNK_ELEMENTS // (per * jstep))
        vals = torch.empty((B, S, m), dtype=torch.float32)
        ptr = torch.empty((B, S, m), dtype=torch.int32)
        for b0 in range(0, B, bstep):
            b1 = min(B, b0 + bstep)
            for j0 in range(0, S, jstep):
                j1 = min(S, j0 + jstep)
                c = (L[b0:b1, None, :, :] + A[j0:j1, :, None]).reshape(b1 - b0, j1 - j0, per)
                c, order = torch.sort(c, dim=2, descending=True, stable=True)
                vals[b0:b1, j0:j1] = obs[b0:b1, t, j0:j1, None] + c[..., :m]
                ptr[b0:b1, j0:j1] = order[..., :m]
        L = vals
        ns.append(m)
        pointers.append(ptr)
        for b in torch.nonzero(F == t + 1).flatten().tolist():
            final[b] = L[b].clone()
    indices = torch.full((B, k, T), -1, dtype=torch.int32)
    scores = torch.full((B, k), -math.inf, dtype=torch.float32)
    bad = (~(pi < math.inf)).any().expand(B).clone()
    if T > 1:
        bad |= (F >= 2) & (~(A < math.inf)).any()
    rows = ~(obs < math.inf)                                               # NaN or +inf
    bad |= (rows & (torch.arange(T)[None, :, None] < F[:, None, None])).flatten(1).any(dim=1)
    for b in range(B):
        if bad[b]:
            scores[b] = math.nan
            continue
        f = int(F[b])
        last = final[b]                                                    # (S, n)
        n = last.shape[1]
        v, order = torch.sort(last.reshape(-1), descending=True, stable=True)
        m = min(k, S * n)
        scores[b, :m] = v[:m]
        for q in range(m):
            s, r = divmod(int(order[q]), n)
            indices[b, q, f:] = s
            for t in range(f - 1, 0, -1):
                indices[b, q, t] = s
                s, r = divmod(int(pointers[t][b, s, r]), ns[t - 1])
            indices[b, q, 0] = s
    return indices, scores
