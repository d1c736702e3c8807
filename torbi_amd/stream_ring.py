"""How a stream's frames live in a device ring: what `StreamDecoder` (stream.py) and `StreamPosteriors`
(stream_posterior.py) share, and stream::Info (csrc/stream.hpp) mirrors.

A stream holds n frames, the first `base` of them already returned; frame t lives in ring slot t % capacity, the capacity a
power of two that `round_capacity` chooses.  Every device call gets one (batch, 4) int32 table, `_info`: pending frames, slot
of frame `base`, new frames (push) or a mark (flush), and whether the stream starts afresh.  `StreamRing` owns these rules, the
checks of a push's and a flush's arguments, the model preparation and the band preparation; each class keeps its own state
layout, its host route and its device calls.  STREAM.md has the layouts.
"""
import ctypes
import operator
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib, band_route, inputs

# ring slots of a new decoder; the ring grows to the power of two a push needs
INITIAL_CAPACITY = 16


def depth(name: str, value, optional: bool = False) -> Optional[int]:
    """`max_lag=` (`optional`: None is no bound) or `lag=` as an integer >= 0, or a ValueError."""
    if value is None and optional:
        return None
    what = f'{name} must be {"None or " if optional else ""}an integer >= 0'
    try:
        if isinstance(value, bool):
            raise TypeError
        value = operator.index(value)
    except TypeError:
        raise ValueError(f'{what}, got {value!r}') from None
    if value < 0:
        raise ValueError(f'{what}, got {value!r}')
    return value


def model(transition: Optional[torch.Tensor], initial: Optional[torch.Tensor], log_probs: bool, states: int, gpu: Optional[int]):
    """(device, original, transition, initial): the model of `from_probabilities` (torbi_amd/inputs.py) as contiguous float32
    on the compute device, so that chunking cannot change a bit.  `transition=None` is the constant matrix it stands for;
    `original` is the tensor the band planner's look is remembered with: the matrix itself (`inputs.plain_matrix`), which is
    the caller's tensor where that is already a plain log matrix on the device."""
    device = inputs._compute_device(gpu)
    transition, uniform, initial = inputs.model(transition, initial, log_probs, states, device, plain=gpu is not None)
    if transition is None:
        transition = torch.full((states, states), uniform, dtype=torch.float32, device=device)
    initial = initial.to(device=device, dtype=torch.float32).contiguous()
    if tuple(transition.shape) != (states, states) or tuple(initial.shape) != (states,):
        raise ValueError(f'transition must be ({states}, {states}) and initial ({states},)')
    transition = inputs.plain_matrix(transition)
    return device, transition, transition, initial


class StreamRing:
    """The bookkeeping of `batch` streams in a ring: `_frames` and `_base` on the host, `_capacity` slots per stream in the
    subclass's `_state` on the device."""

    def _check(self, batch: int, states: int, route: str) -> None:
        if batch < 1 or states < 1:
            raise ValueError(f'{type(self).__name__} needs batch >= 1 and states >= 1')
        band_route.check_route(route, ValueError)

    def _model(self, batch, states, transition, initial, log_probs, gpu) -> Tuple[torch.Tensor, torch.Tensor]:
        """Sets the shape, the device, `initial` and the counters; returns `model`'s (original, transition)."""
        self.batch, self.states, self.log_probs, self.gpu = int(batch), int(states), bool(log_probs), gpu
        self.device, original, transition, self.initial = model(transition, initial, log_probs, self.states, gpu)
        self._frames = np.zeros(self.batch, dtype=np.int64)        # frames pushed
        self._base = np.zeros(self.batch, dtype=np.int64)          # first frame not yet returned
        return original, transition

    # ------------------------------------------------------------------ public
    @staticmethod
    def round_capacity(slots: int) -> int:
        """Ring slots the device route allocates for `slots` rows per stream: the power of two at or above, at least
        INITIAL_CAPACITY."""
        return max(INITIAL_CAPACITY, 1 << (max(int(slots), 1) - 1).bit_length())

    @property
    def frames(self) -> torch.Tensor:
        """(batch,) int64: frames pushed to each stream since it started."""
        return torch.from_numpy(self._frames.copy())

    @property
    def pending(self) -> torch.Tensor:
        """(batch,) int64: frames pushed and not yet returned."""
        return torch.from_numpy(self._frames - self._base)

    @property
    def capacity(self) -> int:
        """Ring slots per stream on the device; on the host the most rows a stream has held."""
        return self._held if self.gpu is None else self._capacity

    # ------------------------------------------------------------------ the arguments of a push and of a flush
    def _push_front(self, observation: torch.Tensor, frames: Optional[torch.Tensor]) -> Tuple[int, np.ndarray]:
        """(Tc, f): the frames of the push and, (batch,) int64, how many of them each stream takes."""
        if observation.dim() != 3 or observation.shape[0] != self.batch or observation.shape[2] != self.states:
            raise ValueError(f'observation must be ({self.batch}, Tc, {self.states}), got {tuple(observation.shape)}')
        Tc = int(observation.shape[1])
        if frames is None:
            return Tc, np.full(self.batch, Tc, dtype=np.int64)
        f = torch.as_tensor(frames).detach().to('cpu', torch.int64).reshape(-1).numpy().copy()
        if f.shape[0] != self.batch or (f < 0).any() or (f > Tc).any():
            raise ValueError(f'frames must hold {self.batch} counts in 0 .. {Tc}')
        return Tc, f

    def _flush_front(self, items: Optional[Sequence[int]]) -> Tuple[List[int], np.ndarray]:
        """(items as a list, default all; marks (batch,) int64: 1 for every stream among them)."""
        items = list(range(self.batch)) if items is None else [int(k) for k in items]
        if any(k < 0 or k >= self.batch for k in items):
            raise IndexError(f'stream index out of range 0 .. {self.batch - 1}')
        marks = np.zeros(self.batch, dtype=np.int64)
        marks[items] = 1
        return items, marks

    # ------------------------------------------------------------------ the ring on the device
    def _upload(self, values: np.ndarray) -> torch.Tensor:
        """A small host array on the compute device.  A plain copy; a class whose calls never synchronise overrides it."""
        return torch.from_numpy(values).to(self.device)

    def _info(self, pending: np.ndarray, third: np.ndarray) -> torch.Tensor:
        """stream::Info of every stream; `third`: the new frames of a push, the marks of a flush."""
        info = np.empty((self.batch, 4), dtype=np.int32)
        info[:, 0], info[:, 1], info[:, 2], info[:, 3] = pending, self._base % self._capacity, third, self._frames == 0
        return self._upload(info)

    def _moving(self, first: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
        """(stream index, frame) of the rows a growing ring moves: frames first[b] .. n_b - 1 of every stream b."""
        counts = self._frames - first
        bi = np.repeat(np.arange(self.batch, dtype=np.int64), counts)
        rank = np.arange(bi.size, dtype=np.int64) - np.repeat(np.cumsum(counts) - counts, counts)     # (within its stream)
        return bi, first[bi] + rank

    def _newest_and_pending(self) -> Tuple[np.ndarray, np.ndarray]:
        """`_moving` for a ring that also holds the newest returned row: frames min(base, n - 1) .. n - 1."""
        return self._moving(np.minimum(self._base, np.maximum(self._frames - 1, 0)))

    def _move(self, pairs, moving: Tuple[np.ndarray, np.ndarray], capacity: int) -> None:
        """new[b, t % capacity] = old[b, t % self._capacity] for every (new, old) of `pairs` and (b, t) of `moving`."""
        bi, fr = moving
        if bi.size:
            bi, to, at = self._upload(bi), self._upload(fr % capacity), self._upload(fr % self._capacity)
            for new, old in pairs:
                new[bi, to] = old[bi, at]

    def _band_diagonals(self, size: str, prepare: str, private: torch.Tensor, over: Tuple[int, int, float]):
        """(diagonals, None) of band `over` = (reach_left, reach_right, background) of the private matrix, from the entries
        named `size` and `prepare`; (None, reason) where the device finds an entry outside the band that is not the
        background.  Reads that verdict back: the constructor's one read-back."""
        left, right, background = over
        diagonals = torch.empty(getattr(self._lib, size)(self.states, left, right) // 4, dtype=torch.float32, device=self.device)
        ok = torch.empty(1, dtype=torch.int32, device=self.device)
        _, index, stream = _lib.launch(self.device)
        _lib.check(getattr(self._lib, prepare)(private.data_ptr(), self.states, left, right, ctypes.c_float(background),
                                               diagonals.data_ptr(), ok.data_ptr(), index, stream), prepare)
        if int(ok.item()) == 1:
            return diagonals, None
        return None, f'an entry outside the band of reach {left}/{right} differs from the background {background}'
