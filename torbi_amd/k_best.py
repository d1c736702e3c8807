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
"""
import ctypes
import math
from typing import Optional, Tuple

import torch

from . import _lib, inputs

MAX_K = 32
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
                  initial: torch.Tensor, k: int, workspace: Optional[torch.Tensor] = None
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
            a graph)

    Returns:
        (indices (B, k, T) int32, scores (B, k) float32) where the observation lives.  Columns t >= F_b repeat the path's
        last state; ranks beyond S^F_b have score -inf and index -1; an item that reads a NaN or +inf has NaN scores and -1
        indices.
    """
    k = _check_k(k)
    if initial is None:
        raise RuntimeError('decode_k_best needs an initial distribution')
    B, T, S = inputs.check_shapes(observation, batch_frames, transition, initial)
    uniform = None if transition is not None else float(torch.tensor(math.log(1. / S), dtype=torch.float32))
    if not observation.is_cuda:
        frames = inputs.frames(batch_frames, B, T, torch.device('cpu'))
        return _host(observation.to(torch.float32), frames, transition, uniform, initial, k)
    frames = inputs.frames(batch_frames, B, T, observation.device)
    return _run(observation.to(torch.float32).contiguous(), frames, transition, uniform, initial, k, workspace)


def best_paths(observation: torch.Tensor, k: int, batch_frames: Optional[torch.Tensor] = None,
               transition: Optional[torch.Tensor] = None, initial: Optional[torch.Tensor] = None, log_probs: bool = False,
               gpu: Optional[int] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """The k best state sequences of every item and their log scores.

    Arguments mean what they mean to `from_probabilities`, defaults included (uniform initial log(1/S + tiny), uniform
    transition log(1/S)), and the inputs go through the same log() and epsilon round trip (torbi_amd/inputs.py), so rank 0
    is bit for bit the path `from_probabilities` returns.  `gpu` is a HIP device index; None computes on the CPU with the
    same float32 sums.  The caller's tensors are not written.

    Returns:
        (indices (batch, k, frames) int32, scores (batch, k) float32) on the compute device, as `decode_k_best`.
    """
    k = _check_k(k)
    B, T, S = inputs.check_shapes(observation, batch_frames, transition, initial)
    device = inputs._compute_device(gpu)
    frames = inputs.frames(batch_frames, B, T, device)
    transition, uniform, initial = inputs.model(transition, initial, log_probs, S, device)
    obs = inputs.observation(observation, log_probs, device)
    if gpu is None:
        return _host(obs, frames, transition, uniform, initial, k)
    return _run(obs, frames, transition, uniform, initial, k)


def _run(observation, frames, transition, uniform, initial, k, workspace=None):
    """One call of the HIP route on the device of `observation` (float32, contiguous, log space)."""
    B, T, S = observation.shape
    device = observation.device
    lib = _lib.load()
    indices = torch.empty((B, k, T), dtype=torch.int32, device=device)
    scores = torch.empty((B, k), dtype=torch.float32, device=device)
    if B == 0:
        return indices, scores
    need = decode_k_best_workspace_bytes(B, T, S, k, uniform=uniform is not None)
    workspace, index, stream = _lib.launch(device, need, workspace)
    frames = frames.to(device=device, dtype=torch.int32).contiguous()
    init = initial.to(device=device, dtype=torch.float32).contiguous()
    tail = (indices.data_ptr(), scores.data_ptr(), workspace.data_ptr(), workspace.numel(), B, T, S, k, index, stream)
    if uniform is not None:
        _lib.check(lib.torbi_hip_k_best_uniform(observation.data_ptr(), frames.data_ptr(), ctypes.c_float(uniform),
                                                init.data_ptr(), *tail), 'torbi_hip_k_best_uniform')
    else:
        trans = transition.to(device=device, dtype=torch.float32).contiguous()
        _lib.check(lib.torbi_hip_k_best(observation.data_ptr(), frames.data_ptr(), trans.data_ptr(), init.data_ptr(), *tail),
                   'torbi_hip_k_best')
    return indices, scores


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
