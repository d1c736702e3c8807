"""Path statistics: the exact log score and the transition counts of GIVEN state paths, on the HMM that
`from_probabilities` decodes.

`from_probabilities` gives the best path, `best_paths` the k best, `sample_paths` posterior draws; this module consumes
them.  A path q of item b (T int32 columns), A indexed [next, prev], F the item's frames clamped to [1, T], every sum in
float32 with one rounding:

    s_0   = fl(o_0[q_0] + pi[q_0])
    s_t   = fl(o_t[q_t] + fl(s_{t-1} + A[q_t, q_{t-1}]))          1 <= t < F
    score = s_{F-1}

which is the decoder's alpha recurrence (`margins`) followed along one path: the score of a path `best_paths` returns at
any rank is that rank's score bit for bit, and the score of `from_probabilities`' path is `best_paths(k=1)`'s score and
`margins.max_marginals`' `score`.  The score reads the cells on the path and no others: a NaN or an infinity on the path
propagates by plain IEEE arithmetic, one elsewhere in the item does not matter, columns t >= F are never read.

A path that holds an index outside [0, S) at a column t < F is VOID -- the -1 ranks of `best_paths`, the -1 rows of
`sample_paths`: its score is -inf and it adds nothing to any count.

Counts, with path weights w[b, k] (all ones unless given), in the orientation of `expected_counts`:

    X[j, i] = sum_{b, k} w[b, k] #{1 <= t < F : q_t = j, q_{t-1} = i}          I[j] = sum_{b, k} w[b, k] [q_0 = j]

accumulated in float64 and rounded to float32 once, so unweighted counts (and counts under weights that are small multiples
of a power of two) are exact whatever the order of the adds, and one M-step divides each column of X by its sum.

The HIP route is csrc/path_statistics.hpp behind torbi_hip_path_statistics (include/torbi_hip.h): one launch, one wavefront
per path.  Host tensors and `gpu=None` run the same chain with torch CPU ops.  PATHS.md has the contract, the kernel and the
numbers.

This module is published as the submodule `torbi_amd.paths`, like `margins`; its functions are not in `torbi_amd.__all__`
(every top-level function that takes an observation has a row in the operand-form table of the test suite; the same forms
are run from this feature's own tests).
"""
import math
from typing import Optional, Tuple

import torch

from . import _lib, inputs, viterbi

__all__ = ['path_statistics', 'path_statistics_workspace_bytes', 'score_paths', 'count_paths', 'viterbi_counts',
           'best_path_score']


def path_statistics_workspace_bytes(B: int, T: int, S: int, K: int, counts: bool = True) -> int:
    """Bytes of device scratch `path_statistics` needs for K paths of each of B items of a (B, T, S) problem: the S * S + S
    float64 accumulators of the counts; 0 without `counts`."""
    return int(_lib.load().torbi_hip_path_statistics_workspace_size(B, T, S, K, 1 if counts else 0))


def _indices(indices: torch.Tensor, B: int, T: int):
    """((B, K, T) view of `indices`, whether it came as (B, T))."""
    if indices.dtype not in (torch.int32, torch.int64):
        raise RuntimeError(f'indices must be int32 or int64; got {indices.dtype}')
    flat = indices.dim() == 2
    if flat:
        indices = indices[:, None, :]
    if indices.dim() != 3 or indices.shape[0] != B or indices.shape[2] != T or indices.shape[1] < 1:
        raise RuntimeError(f'indices must have shape ({B}, K, {T}) or ({B}, {T}); got {tuple(indices.shape)}')
    return indices, flat


def _weights(path_weights, B: int, K: int, flat: bool):
    """`path_weights` as (B, K), or None."""
    if path_weights is None:
        return None
    if flat and path_weights.dim() == 1:
        path_weights = path_weights[:, None]
    if tuple(path_weights.shape) != (B, K):
        raise RuntimeError(f'path_weights must have shape ({B}, {K}){f" or ({B},)" if flat else ""}; got '
                           f'{tuple(path_weights.shape)}')
    return path_weights


def path_statistics(observation: torch.Tensor, batch_frames: Optional[torch.Tensor], transition: Optional[torch.Tensor],
                    initial: torch.Tensor, indices: torch.Tensor, path_weights: Optional[torch.Tensor] = None,
                    counts: bool = True, workspace: Optional[torch.Tensor] = None
                    ) -> Tuple[torch.Tensor, Optional[torch.Tensor], Optional[torch.Tensor]]:
    """Scores and counts of given paths on log inputs: the operator level, like `forward_backward_max`.  Runs on the HIP
    device of `observation`, or on the host for a host tensor.

    Args:
        observation: (B, T, S) float32 log scores
        batch_frames: (B,) valid frames per item (clamped to [1, T]); None = all T
        transition: (S, S) float32 log transition matrix [next, prev]; None = uniform, fl(log(1/S)) everywhere
        initial: (S,) float32 log initial distribution
        indices: (B, K, T) int32 or int64 state paths, K per item; or (B, T), one per item
        path_weights: (B, K) weights of the paths in the counts ((B,) too with (B, T) indices); None = all ones
        counts: also return the counts
        workspace: optional uint8 device tensor of >= `path_statistics_workspace_bytes(B, T, S, K, counts)` bytes, no
            alignment and no initialisation (a call that owns its workspace allocates nothing but its outputs, so it can be
            captured into a graph; the graph is linear); not needed without `counts`; ignored on the host

    Returns:
        (scores (B, K) float32 -- (B,) for (B, T) indices --, transition_counts (S, S) float32 [next, prev] or None,
        initial_counts (S,) float32 or None) where the observation lives.  A void path scores -inf and counts nothing.
    """
    if initial is None:
        raise RuntimeError('path_statistics needs an initial distribution')
    B, T, S = inputs.check_shapes(observation, batch_frames, transition, initial)
    q, flat = _indices(indices, B, T)
    K = q.shape[1]
    w = _weights(path_weights, B, K, flat)
    uniform = None if transition is not None else float(torch.tensor(math.log(1. / S), dtype=torch.float32))
    device = observation.device
    frames = inputs.frames(batch_frames, B, T, device)
    if not observation.is_cuda:
        model = (observation.to(torch.float32), transition, uniform, initial)
        scores, X, I = _host(model, frames, q, w, S, counts)
    else:
        model = (observation.to(torch.float32).contiguous(), transition, uniform, initial)
        scores, X, I = _run(model, frames, q.to(device), w, S, counts, workspace)
    return (scores[:, 0] if flat else scores), X, I


def score_paths(observation: torch.Tensor, indices: torch.Tensor, batch_frames: Optional[torch.Tensor] = None,
                transition: Optional[torch.Tensor] = None, initial: Optional[torch.Tensor] = None, log_probs: bool = False,
                gpu: Optional[int] = None) -> torch.Tensor:
    """The log score of every given path under the model `from_probabilities` decodes.

    Arguments mean what they mean to `from_probabilities`, defaults included (uniform initial log(1/S + tiny), uniform
    transition log(1/S)), and the inputs go through the same log() and epsilon round trip (torbi_amd/inputs.py), so scoring
    the indices `best_paths` returns gives its scores bit for bit, at every rank.  `gpu` is a HIP device index; None
    computes on the CPU with the same float32 sums.  The caller's tensors are not written.

        indices, scores = best_paths(observation, 4, gpu=0)
        assert torch.equal(score_paths(observation, indices, gpu=0), scores)
        posterior = (score_paths(observation, path, gpu=0) - log_likelihood).exp()     # P(path | observations)

    indices: (batch, K, frames) or (batch, frames), int32 or int64, anywhere (moved to the compute device).

    Returns:
        scores (batch, K) float32 -- (batch,) for (batch, frames) indices -- on the compute device; -inf for a void path.
    """
    B, T, S = inputs.check_shapes(observation, batch_frames, transition, initial)
    q, flat = _indices(indices, B, T)
    device = inputs._compute_device(gpu)
    frames = inputs.frames(batch_frames, B, T, device)
    transition, uniform, initial = inputs.model(transition, initial, log_probs, S, device, plain=gpu is not None)
    obs = inputs.observation(observation, log_probs, device)
    route = _host if gpu is None else _run
    scores = route((obs, transition, uniform, initial), frames, q.to(device), None, S, False)[0]
    return scores[:, 0] if flat else scores


def count_paths(indices: torch.Tensor, states: int, batch_frames: Optional[torch.Tensor] = None,
                path_weights: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """Transition and initial-state counts of given paths: no model, no observation.  The statistic of `sample_paths`
    draws (stochastic EM) and of decoded paths (Viterbi training).  Runs where `indices` lives.

        draws, _ = sample_paths(observation, 16, transition=A, initial=pi, gpu=0)
        X, I = count_paths(draws, states, batch_frames)
        A = X / X.sum(0, keepdim=True).clamp_min(1)         # the M-step of stochastic EM, [next, prev]

    Args:
        indices: (batch, K, frames) or (batch, frames) int32 or int64 paths
        states: S
        batch_frames: (batch,) valid frames per item (clamped to [1, frames]); None = all
        path_weights: (batch, K) weights ((batch,) too with (batch, frames) indices); None = all ones

    Returns:
        (transition_counts (S, S) float32 [next, prev], initial_counts (S,) float32) where the indices live.  Void paths
        (an index outside [0, S) at a column < F: the -1 rows of `sample_paths`) count nothing.
    """
    if indices.dim() not in (2, 3):
        raise RuntimeError(f'indices must have shape (batch, K, frames) or (batch, frames); got {tuple(indices.shape)}')
    B, T = indices.shape[0], indices.shape[-1]
    S = int(states)
    if T < 1 or S < 1:
        raise RuntimeError('count_paths needs at least one frame and one state')
    if batch_frames is not None and tuple(batch_frames.shape) != (B,):
        raise RuntimeError(f'batch_frames must have shape ({B},); got {tuple(batch_frames.shape)}')
    q, flat = _indices(indices, B, T)
    w = _weights(path_weights, B, q.shape[1], flat)
    frames = inputs.frames(batch_frames, B, T, indices.device)
    route = _run if indices.is_cuda else _host
    return route(None, frames, q, w, S, True)[1:]


def viterbi_counts(observation: torch.Tensor, batch_frames: Optional[torch.Tensor] = None,
                   transition: Optional[torch.Tensor] = None, initial: Optional[torch.Tensor] = None,
                   log_probs: bool = False, gpu: Optional[int] = None, item_weights: Optional[torch.Tensor] = None
                   ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """The hard E-step: the transition and initial-state counts of every item's best path, and that path's score -- what
    `expected_counts` is to Baum-Welch, for Viterbi training (hard EM, segmental k-means).

    Arguments mean what they mean to `from_probabilities`, defaults and preprocessing included; the operands are prepared
    once, decoded by the decoder `from_probabilities` uses (whatever route its dispatcher picks) and counted by
    `path_statistics` on the same prepared tensors.  `gpu` is a HIP device index; None decodes with the CPU operator.
    item_weights: (batch,) weights of the items in the counts; None = all ones.

    A Viterbi-training loop (the Baum-Welch loop with `expected_counts` replaced):

        A, pi = A0.clone(), pi0.clone()                                  # probabilities, [next, prev]
        for step in range(steps):
            X, I, score = viterbi_counts(observation, frames, A, pi, gpu=0)
            A = (X + prior) / (X + prior).sum(0, keepdim=True)           # each column: the next states of one state
            pi = (I + prior) / (I + prior).sum()
            # score.sum() never decreases while prior == 0

    Returns:
        (transition_counts (S, S) [next, prev], initial_counts (S,), score (batch,)), float32 on the compute device;
        score is `best_paths(..., k=1)`'s, bit for bit.
    """
    B, T, S = inputs.check_shapes(observation, batch_frames, transition, initial)
    if item_weights is not None and tuple(item_weights.shape) != (B,):
        raise RuntimeError(f'item_weights must have shape ({B},); got {tuple(item_weights.shape)}')
    device = inputs._compute_device(gpu)
    frames = inputs.frames(batch_frames, B, T, device)
    transition, uniform, initial = inputs.model(transition, initial, log_probs, S, device, plain=gpu is not None)
    obs = inputs.observation(observation, log_probs, device)
    init = initial.to(torch.float32)
    trans = None if transition is None else transition.to(torch.float32)
    path = _decode(obs, frames, trans, uniform, init)
    w = None if item_weights is None else item_weights.to(device)[:, None]
    route = _host if gpu is None else _run
    scores, X, I = route((obs, trans, uniform, init), frames, path[:, None, :], w, S, True)
    return X, I, scores[:, 0]


def _decode(obs, frames, transition, uniform, initial):
    """The best path of prepared float32 operands through the existing decoders: `viterbi.decode` / `decode_uniform` on the
    device, `decode_cpu` on the host (the uniform matrix materialised there, like `from_probabilities`)."""
    if not obs.is_cuda:
        if transition is None:
            transition = torch.full((obs.shape[2],) * 2, uniform, dtype=torch.float32)
        return viterbi.decode_cpu(obs, frames, transition.contiguous(), initial.contiguous())
    if transition is None:
        return viterbi.decode_uniform(obs, frames, uniform, initial)
    return viterbi.decode(obs, frames, transition, initial)


class _BestPathScore(torch.autograd.Function):
    @staticmethod
    def forward(ctx, observation, batch_frames, transition, initial):
        B, T, S = inputs.check_shapes(observation, batch_frames, transition, initial)
        device = observation.device
        ctx.dtypes = (observation.dtype, None if transition is None else transition.dtype, initial.dtype)
        ctx.devices = (device, None if transition is None else transition.device, initial.device)
        ctx.states = S
        frames = inputs.frames(batch_frames, B, T, device)
        obs = observation.detach().to(torch.float32).contiguous()
        init = initial.detach().to(device=device, dtype=torch.float32).contiguous()
        uniform, trans = None, None
        if transition is None:
            uniform = float(torch.tensor(math.log(1. / S), dtype=torch.float32))
        elif device.type == 'cuda':
            trans = inputs.plain_matrix(transition.detach().to(device))
        else:
            trans = transition.detach().to(torch.float32).contiguous()
        path = _decode(obs, frames, trans, uniform, init)
        route = _run if device.type == 'cuda' else _host
        scores = route((obs, trans, uniform, init), frames, path[:, None, :], None, S, False)[0][:, 0]
        ctx.save_for_backward(frames, path)
        return scores

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad):
        frames, path = ctx.saved_tensors
        need_o, _, need_t, need_i = ctx.needs_input_grad
        B, T = path.shape
        S = ctx.states
        g = grad.to(device=path.device, dtype=torch.float32).contiguous()
        d_obs = d_trans = d_init = None
        if need_o:
            live = torch.arange(T, device=path.device)[None, :] < frames.clamp(1, T)[:, None]             # (B, T)
            d_obs = torch.zeros((B, T, S), dtype=torch.float32, device=path.device)
            d_obs.scatter_(2, path.to(torch.int64).clamp(0, S - 1)[:, :, None], (g[:, None] * live)[:, :, None])
        if need_t or need_i:
            route = _run if path.is_cuda else _host
            _, d_trans, d_init = route(None, frames, path[:, None, :], g[:, None], S, True)
        dtypes, devices = ctx.dtypes, ctx.devices
        cast = lambda v, k, need: None if v is None or not need else v.to(device=devices[k], dtype=dtypes[k])
        return cast(d_obs, 0, need_o), None, cast(d_trans, 1, need_t), cast(d_init, 2, need_i)


def best_path_score(observation: torch.Tensor, batch_frames: Optional[torch.Tensor], transition: Optional[torch.Tensor],
                    initial: torch.Tensor) -> torch.Tensor:
    """The score of every item's best path, differentiable in observation, transition and initial (log inputs, the operator
    level): the structured-perceptron / max-margin counterpart of `log_likelihood`.

    The forward is one decode (the existing decoder, on the device of `observation`; `decode_cpu` for host tensors) and one
    scores-only `path_statistics` call.  The backward: d/dobservation is g_b at (t, q_t) for t < F_b and 0 elsewhere;
    d/dtransition = X(g) and d/dinitial = I(g) come from one counts-only `path_statistics` call with the incoming gradient
    as path weights, made only when one of them is needed.  At a tie the subgradient is the decoded path's.  First order
    only.  `transition=None` is the uniform model (and has no gradient).

    Returns:
        (B,) float32 scores: `best_paths(..., k=1)`'s, bit for bit.
    """
    if initial is None:
        raise RuntimeError('best_path_score needs an initial distribution')
    return _BestPathScore.apply(observation, batch_frames, transition, initial)


def _run(model, frames, indices, weights, S, counts, workspace=None):
    """One call of torbi_hip_path_statistics on the device of `indices` ((B, K, T)).  `model`: (observation (float32,
    contiguous, log space), transition or None, uniform value, initial), or None for a counts-only call."""
    B, K, T = indices.shape
    device = indices.device
    scores = None if model is None else torch.empty((B, K), dtype=torch.float32, device=device)
    X = I = None
    if counts:
        fresh = torch.zeros if B == 0 else torch.empty
        X, I = fresh((S, S), dtype=torch.float32, device=device), fresh((S,), dtype=torch.float32, device=device)
    if B == 0:
        return scores, X, I
    lib = _lib.load()
    need = int(lib.torbi_hip_path_statistics_workspace_size(B, T, S, K, 1 if counts else 0))
    workspace, index, stream = _lib.launch(device, need if counts else None, workspace if counts else None)
    # (every converted copy lives until the call is queued)
    q = indices.to(torch.int32).contiguous()
    frames = frames.to(device, torch.int32).contiguous()
    w = None if weights is None or not counts else weights.to(device, torch.float32).contiguous()
    obs = trans = init = None
    uniform = 0.
    if model is not None:
        obs, trans, uniform, init = model
        if obs.device != device:
            raise RuntimeError(f'indices are on {device}, the observation on {obs.device}')
        trans = None if trans is None else trans.to(device, torch.float32).contiguous()
        init = init.to(device, torch.float32).contiguous()
        uniform = 0. if uniform is None or trans is not None else uniform
    ptr = lambda t: None if t is None else t.data_ptr()
    _lib.check(lib.torbi_hip_path_statistics(ptr(obs), frames.data_ptr(), ptr(trans), uniform, ptr(init), q.data_ptr(), ptr(w),
                                             ptr(scores), ptr(X), ptr(I), ptr(workspace),
                                             0 if workspace is None else workspace.numel(), B, T, S, K, index, stream),
               'torbi_hip_path_statistics')
    return scores, X, I


def _host(model, frames, indices, weights, S, counts, workspace=None):
    """The same with torch CPU ops: the chain as elementwise float32 operations over (B, K), frame by frame (one rounding
    per operation, so the same bits), the counts with `index_add_` in float64."""
    B, K, T = indices.shape
    q = indices.detach().to('cpu', torch.int64)
    F = frames.detach().to('cpu', torch.int64).clamp(1, T)
    live = torch.arange(T)[None, :] < F[:, None]                                        # (B, T)
    void = (((q < 0) | (q >= S)) & live[:, None, :]).any(dim=2)                         # (B, K)
    q = q.clamp(0, S - 1)
    scores = X = I = None
    if model is not None:
        obs, A, uniform, pi = model
        obs = obs.detach().to('cpu', torch.float32)
        pi = pi.detach().to('cpu', torch.float32)
        A = None if A is None else A.detach().to('cpu', torch.float32)
        u = None if A is not None else torch.tensor(uniform, dtype=torch.float32)
        scores = torch.empty((B, K), dtype=torch.float32)
        if B:
            s = obs[:, 0].gather(1, q[:, :, 0]) + pi[q[:, :, 0]]
            for t in range(1, int(F.max())):
                a = A[q[:, :, t], q[:, :, t - 1]] if A is not None else u
                s = torch.where(live[:, t, None], obs[:, t].gather(1, q[:, :, t]) + (s + a), s)
            scores = torch.where(void, torch.tensor(-math.inf), s)
    if counts:
        w = torch.ones((B, K), dtype=torch.float64) if weights is None else weights.detach().to('cpu', torch.float64)
        keep = ~void
        I = torch.zeros((S,), dtype=torch.float64).index_add_(0, q[:, :, 0][keep], w[keep])
        X = torch.zeros((S * S,), dtype=torch.float64)
        if T > 1:
            step = (keep[:, :, None] & live[:, None, 1:]).expand(B, K, T - 1)
            cell = q[:, :, 1:] * S + q[:, :, :-1]
            X.index_add_(0, cell[step], w[:, :, None].expand(B, K, T - 1)[step])
        X, I = X.view(S, S).to(torch.float32), I.to(torch.float32)
    return scores, X, I
