"""The model's inputs as upstream prepares them before any kernel runs (reference torbi/core.py:145-197): the defaults of
`initial` and `transition`, `log()` where the input lives, the move to the compute device as float32 and the epsilon round
trip `log(exp(x) + tiny)`.  `from_probabilities`, `StreamDecoder`, `state_posteriors` and `expected_counts` take their
model from here, so all of them see it bit for bit alike.
"""
import math

import torch

from . import slabs, state, viterbi


def _compute_device(gpu) -> torch.device:
    """The device a `gpu` argument names: HIP device `gpu`, or the CPU for None (like upstream)."""
    if gpu is None:
        return torch.device('cpu')
    if gpu == 'mps':
        raise RuntimeError('the MPS backend of the reference is out of scope on MI355X')
    if not torch.cuda.is_available():
        raise RuntimeError(
            f'from_probabilities(gpu={gpu!r}) needs a HIP device and PyTorch-ROCm reports none; there is no CPU '
            'fallback for a GPU request (gpu=None selects the CPU operator, like upstream)')
    return torch.device(f'cuda:{gpu}')


def check_shapes(observation, batch_frames, transition, initial):
    """(B, T, S) of a call; raises before anything is launched or computed unless batch_frames is (B,), transition (S, S)
    and initial (S,) (None: not given).  The kernels read exactly those extents."""
    if observation.dim() != 3:
        raise RuntimeError(f'observation must have shape (batch, frames, states); got {tuple(observation.shape)}')
    B, T, S = observation.shape
    if T < 1 or S < 1:
        raise RuntimeError('observation needs at least one frame and one state')
    if batch_frames is not None and tuple(batch_frames.shape) != (B,):
        raise RuntimeError(f'batch_frames must have shape ({B},); got {tuple(batch_frames.shape)}')
    if transition is not None and tuple(transition.shape) != (S, S):
        raise RuntimeError(f'transition must have shape ({S}, {S}); got {tuple(transition.shape)}')
    if initial is not None and tuple(initial.shape) != (S,):
        raise RuntimeError(f'initial must have shape ({S},); got {tuple(initial.shape)}')
    return B, T, S


def frames(batch_frames, B: int, T: int, device) -> torch.Tensor:
    """(B,) int32 valid frames per item on `device`; None = all T (core.py:152-158)."""
    if batch_frames is None:
        return torch.full((B,), T, dtype=torch.int32, device=device)
    return batch_frames.to(device=device, dtype=torch.int32).contiguous()


def model(transition, initial, log_probs: bool, states: int, device, plain: bool = False):
    """(transition or None, uniform or None, initial) in log space on `device` (core.py:161-187).  A missing initial
    becomes log(1/S + tiny); a missing transition is returned as the float value of upstream's float32 fill log(1/S)
    (`torch.full((S, S), uniform)` gives upstream's matrix).  Dtypes are kept, like upstream, whose operator then refuses
    what is not float32 -- unless `plain`: the device routes of the features that convert (posteriors, counts, k-best,
    sampling, the stream classes) take the matrix as `device_matrix` gives it, the one tensor their band planner looks at
    and their kernels read (their `gpu=None` routes compute in the dtype they are given)."""
    if initial is None:
        initial = torch.full((states,), math.log((1. / states) + torch.finfo(torch.float32).tiny), dtype=torch.float32,
                             device=device)
    else:
        initial = (initial if log_probs else torch.log(initial)).to(device)
    uniform = None
    if transition is None:
        uniform = float(torch.tensor(math.log(1. / states), dtype=torch.float32))
    elif plain:
        transition = device_matrix(transition, log_probs, device)
    elif device.type == 'cpu':
        transition = (transition if log_probs else torch.log(transition)).to(device)
    else:
        transition = _prepared_transition(transition, log_probs, device)
    return transition, uniform, initial


def observation(observation: torch.Tensor, log_probs: bool, device, in_place: bool = False,
                non_blocking: bool = False) -> torch.Tensor:
    """log() unless `log_probs` (where the observation lives, core.py:189-191), the move to `device` as float32 and the
    epsilon round trip (core.py:193-197): a contiguous float32 tensor on `device`.

    in_place: the round trip may write the caller's tensor when it is already float32 on `device` (upstream does it in
        place); otherwise such a tensor is copied first
    non_blocking: the host-to-device copy of a pinned host batch is asynchronous
    """
    source = observation
    if not log_probs:
        clamped = viterbi.log_epsilon_clamp(observation) if observation.device == device else None
        if clamped is not None:
            return clamped                      # log() and the round trip as ONE pass on the device, out of place
        observation = torch.log(observation) if device.type == 'cpu' else _host_log(observation)
    moved = observation.to(device=device, dtype=torch.float32, non_blocking=non_blocking)
    slab = getattr(observation, 'torbi_slab', None)
    if slab is not None:                        # (_host_log's pooled buffer: free again once the copy has left)
        left = torch.cuda.Event()
        left.record(torch.cuda.current_stream(device))
        slabs.pool(None).give(slab, left)
    if not in_place and moved.data_ptr() == source.data_ptr():
        moved = moved.clone(memory_format=torch.contiguous_format)
    return viterbi.epsilon_clamp_(moved).contiguous()


def _prepared_transition(transition: torch.Tensor, log_probs: bool, device) -> torch.Tensor:
    """log() (unless `log_probs`) and device move of the transition matrix (core.py:181-187), remembered with the
    caller's tensor (object and version, torbi_amd/state.py): repeated calls with one matrix then hand torbi_amd.decode
    the SAME device tensor, which is what its structure look and path measurements hang off."""
    kept = state.notes(transition)             # None under torch.inference_mode(): nothing to remember it by
    key = ('prepared', bool(log_probs), str(device))
    if kept is not None and key in kept:
        return kept[key]
    prepared = (transition if log_probs else torch.log(transition)).to(device)
    if kept is not None and prepared is not transition:        # (a tensor in its own notes would never be collected)
        kept[key] = prepared
    return prepared


def device_matrix(transition: torch.Tensor, log_probs: bool, device) -> torch.Tensor:
    """`_prepared_transition` as every device route of a feature reads it: float32, contiguous, its base 16-byte aligned.
    THE matrix of a call: what the band planner looks at (`viterbi.band_over` reads S * S float32 words, row-major, behind
    the pointer and refuses anything else) is what the kernels are handed, so a band is never found in one layout and
    promised for another, and nothing is copied twice."""
    return plain_matrix(_prepared_transition(transition, log_probs, device))


def plain_matrix(matrix: torch.Tensor) -> torch.Tensor:
    """A matrix where it lives as float32, contiguous, its base 16-byte aligned: the tensor itself when it is all that --
    whatever is known about it stays known --, else ONE copy (S x S: nothing next to a call), remembered with the tensor's
    notes (object and version, torbi_amd/state.py) so that repeated calls look at, and hand on, the SAME copy."""
    kept = state.notes(matrix)
    if kept is not None and 'plain' in kept:
        return kept['plain']
    plain = (matrix.detach() if matrix.requires_grad else matrix).to(torch.float32).contiguous()
    if plain.data_ptr() % 16:
        plain = plain.clone()
    if plain is matrix:
        return matrix
    if kept is not None:
        kept['plain'] = plain
    return plain


def _host_log(observation: torch.Tensor) -> torch.Tensor:
    """`torch.log(observation)` where the observation lives, like upstream (core.py:189-191: the log is taken BEFORE the device
    move, so a host batch is logged by the host and the operator sees the host's roundings).  A large float32 host batch is
    logged into a pinned buffer of the process-wide pool (torbi_amd/slabs.py; `release_job_memory()` frees it): the same
    kernel, the same bits, but no fresh 1.5 GB of first-touched pages per call and an asynchronous copy at the host link's rate
    behind it -- 512 x 500 x 1440: 398 -> ~65 ms per call.  The size from which on it does so is core.HOST_LOG_POOL_BYTES,
    a setting next to core's other host-link settings (read here at call time: core imports this module)."""
    from . import core
    nbytes = observation.numel() * 4
    if (observation.device.type != 'cpu' or observation.dtype != torch.float32 or nbytes < core.HOST_LOG_POOL_BYTES
            or observation.requires_grad or not torch.cuda.is_available()):          # (`out=` is not for tensors in a graph)
        return torch.log(observation)
    slab = slabs.pool(None).take(nbytes, limit=2)
    out = slab[:nbytes].view(torch.float32).view(observation.shape)
    torch.log(observation, out=out)
    out.torbi_slab = slab
    return out
