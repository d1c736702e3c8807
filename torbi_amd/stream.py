"""Exact streaming Viterbi decoding: frames pushed in pieces, indices returned as soon as they are final.

Frame c of a stream is DECIDED once the survivor paths of every state at the newest frame pass through one single state at
c: no later observation can change the path up to c any more.  `push` returns, per stream, the frames that became decided,
`flush` the rest; concatenated they are bit-identical to `from_probabilities` on the whole sequence (NaN and +/-inf
included).  The HIP route is csrc/stream.hpp behind torbi_hip_stream_* (include/torbi_hip.h); `gpu=None` runs the same
decoder on the host with torch CPU ops.  STREAM.md has the layout and the kernels.

A matrix that holds ONE value outside a band (the reference's pitch matrix: 175 diagonals of 1440 states) takes the band
route on the device (csrc/stream_band.hpp behind torbi_hip_stream_band_*; STREAM.md, "Band route"): a frame costs the band
and two scans, and the backpointers are stored, not recomputed.  `route` chooses; the outputs are the same bits either way.

`max_lag` bounds the delay and the memory (truncated, or fixed-lag, Viterbi): a push leaves at most `max_lag` frames pending
and returns the older ones along the path that is best at the newest frame (STREAM.md, "Bounded lag").
"""
import ctypes
import math
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib, band_route, inputs, stream_ring
from .stream_ring import INITIAL_CAPACITY

ROUTES = band_route.ROUTES


def _covered(batch, states, reach_left, reach_right, background, index=0) -> bool:
    """torbi_hip_stream_band_covers: the band route takes this many streams, this band and background."""
    return bool(_lib.load().torbi_hip_stream_band_covers(int(batch), states, reach_left, reach_right, background, index))


def _band_plan(trans: torch.Tensor, original: torch.Tensor, batch: int, states: int, index: int
               ) -> Tuple[Optional[Tuple[int, int, float]], str]:
    """`band_route.plan` for this feature: the shape is what torbi_hip_stream_band_covers takes."""
    return band_route.plan(trans, original, _covered, 'torbi_hip_stream_band_covers', dict(batch=int(batch), states=states),
                           index, finite='a finite value below every entry of the band')


def stream_route(transition: Optional[torch.Tensor], batch: int, states: int, gpu: Optional[int] = 0,
                 log_probs: bool = False) -> str:
    """The route `StreamDecoder(batch, states, transition, log_probs=log_probs, gpu=gpu, route='auto')` takes: 'band' (one
    value outside a band the band kernels cover), 'dense', or 'host' for `gpu=None`.  `transition=None` is asked about as
    the constant matrix it stands for."""
    if gpu is None:
        return 'host'
    states = int(states)
    if transition is not None and tuple(transition.shape) != (states, states):
        raise ValueError(f'transition must be ({states}, {states})')
    device, original, trans, _ = stream_ring.model(transition, None, log_probs, states, gpu)
    return 'dense' if _band_plan(trans, original, batch, states, device.index or 0)[0] is None else 'band'


class StreamDecoder(stream_ring.StreamRing):
    """Viterbi decoding of `batch` independent streams whose frames arrive in pieces.

    `transition` (states, states) [next, prev], `initial` (states,) and `log_probs` mean what they mean to
    `from_probabilities`, defaults included (uniform initial log(1/S + tiny), uniform transition log(1/S)); observations go
    through the same log() and epsilon round trip.  `gpu` is a HIP device index; None decodes on the host.

    Device memory per stream: (4 * states + 4) bytes per pending frame (a posterior row and a word of the frontier walk) plus
    4 * states; the ring grows by doubling, so a stream whose frames never become decided (an identity transition matrix)
    holds all of them until `flush` -- unless `max_lag` is set.

    `max_lag` (None: no bound, the exact decoder above; an integer >= 0): the decision depth.  A stream with n frames that
    receives at least one frame in a push returns its frames up to max(newest decided frame, n - 1 - max_lag), so that
    `pending <= max_lag` after every push.  The frames beyond the decided ones are FORCED: their states lie on the backtrace
    from the final state of the newest row (`flush`'s rule).  Every push's output is therefore the corresponding span of the
    whole-sequence decode of the stream's first n frames, and `forced` counts the frames that left this way.
    * A stream whose `forced` count is 0 is still bit-identical to the whole-sequence decode.
    * A forced span and the span after it may not join into one path: a later observation can move the best path.  That is
      the price of the bound; nothing is repaired or decoded again.
    * The device ring (`capacity`) never exceeds the power of two at or above max_lag + (largest Tc pushed) + 1, nor does it
      fall below INITIAL_CAPACITY; the host route holds at most max_lag + Tc + 1 rows per stream.

        dec = StreamDecoder(batch, states, transition, initial)
        out = dec.push(observation)       # (batch, Tc, states) -> `batch` int32 tensors, the frames decided by this push
        rest = dec.flush()                # the remaining frames of every stream; the streams start afresh

    `route` ('auto', 'dense' or 'band'; ignored with `gpu=None`): which device route the decoder takes.  'band' is the
    band route for a matrix that holds one value outside a band (`viterbi.band_over` finds the band,
    torbi_hip_stream_band_covers says whether the kernels take it, and the constructor extracts the diagonals from a private
    copy of the matrix and reads the device's verdict on it back once); it raises RuntimeError, naming the reason, where
    any of these says no.  'auto' takes the band route where all of them say yes and the dense route otherwise
    (`torbi_amd.stream_route` answers which); 'dense' is the route for any matrix.  `dec.route` tells: 'band', 'dense' or
    'host'.  Outputs, `pending`, `forced` and the memory per pending frame are the same on every route, bit for bit.
    """

    def __init__(self, batch: int, states: int, transition: Optional[torch.Tensor] = None,
                 initial: Optional[torch.Tensor] = None, log_probs: bool = False, gpu: Optional[int] = 0,
                 max_lag: Optional[int] = None, route: str = 'auto'):
        self._check(batch, states, route)
        self.max_lag = stream_ring.depth('max_lag', max_lag, optional=True)
        original, self.transition = self._model(batch, states, transition, initial, log_probs, gpu)
        self._forced = np.zeros(self.batch, dtype=np.int64)        # frames returned by forced commits (max_lag)
        if gpu is None:
            self._rows = [[] for _ in range(self.batch)]            # posterior rows of frames base-1 .. n-1 (host)
            self._memo = [{} for _ in range(self.batch)]            # frame -> survivor-set size of an earlier walk
            self._held = 0                                          # most rows any stream has held
            self.route = 'host'
        else:
            self._lib = _lib.load()
            self._band = None if route == 'dense' else self._prepare_band(original, route)
            self.route = 'dense' if self._band is None else 'band'
            if self._band is None:
                self._transposed = self.transition.t().contiguous()
            self._capacity = 0
            self._state = None
            self._grow(INITIAL_CAPACITY)

    # ------------------------------------------------------------------ public
    @property
    def forced(self) -> torch.Tensor:
        """(batch,) int64: frames of each stream returned by forced commits (`max_lag`) since it started."""
        return torch.from_numpy(self._forced.copy())

    def push(self, observation: torch.Tensor, frames: Optional[torch.Tensor] = None) -> List[torch.Tensor]:
        """Append frames to the streams and return what became decided.

        observation (batch, Tc, states); frames (batch,) valid frames per stream, 0 .. Tc (None = all Tc).  Returns `batch`
        1-D int32 tensors on the compute device: the indices of the frames this push decided, oldest first.  On the GPU this
        reads one small per-stream count array back, so every call synchronises the host with the current stream once.
        """
        _, f = self._push_front(observation, frames)
        obs = inputs.observation(observation, self.log_probs, self.device)
        if self.gpu is None:
            return self._push_host(obs, f)
        return self._push_device(obs, f)

    def flush(self, items: Optional[Sequence[int]] = None) -> List[torch.Tensor]:
        """End streams `items` (default: all): return their remaining indices (one 1-D int32 tensor per item, in the
        order given) and reset them, so that their next push starts a new sequence from `initial`.  The final state is the
        first NaN of the newest posterior row, otherwise its first maximum (the reference's argmax)."""
        items, marks = self._flush_front(items)
        if self.gpu is None:
            rest = {k: self._flush_host(k) for k in items}
        else:
            rest = self._flush_device(marks)
        for k in set(items):
            self._frames[k] = self._base[k] = self._forced[k] = 0
        return [rest[k] for k in items]

    # ------------------------------------------------------------------ host route
    def _row(self, prev: torch.Tensor, obs_row: torch.Tensor) -> torch.Tensor:
        cand = prev[None, :] + self.transition                    # [next, prev]
        nan = torch.isnan(cand)
        best = cand.masked_fill(nan, -math.inf).amax(dim=1)
        # the reference's scan keeps a NaN candidate of prev-state 0 and never takes one elsewhere
        best = torch.where(nan[:, 0], torch.full_like(best, math.nan), best)
        return obs_row + best

    def _backpointers(self, prev: torch.Tensor, states: torch.Tensor) -> torch.Tensor:
        cand = prev[None, :] + self.transition[states]
        nan = torch.isnan(cand)
        arg = cand.masked_fill(nan, -math.inf).argmax(dim=1)     # first maximum of the non-NaN candidates
        return torch.where(nan[:, 0], torch.zeros_like(arg), arg)

    @staticmethod
    def _final_state(row: torch.Tensor) -> int:
        nan = torch.isnan(row)
        if bool(nan.any()):
            return int(nan.to(torch.uint8).argmax())
        return int(row.argmax())

    def _backtrace_host(self, b: int, c: int, state: int) -> torch.Tensor:
        """Indices of frames base .. c of stream b, the path through `state` at frame c."""
        base, rows = int(self._base[b]), self._rows[b]
        first = int(self._frames[b]) - len(rows)                  # frame of rows[0]
        out = [state]
        for t in range(c, base, -1):
            state = int(self._backpointers(rows[t - 1 - first], torch.tensor([state]))[0])
            out.append(state)
        return torch.tensor(out[::-1], dtype=torch.int32)

    def _push_host(self, obs: torch.Tensor, f: np.ndarray) -> List[torch.Tensor]:
        S, result = self.states, []
        for b in range(self.batch):
            rows = self._rows[b]
            for t in range(int(f[b])):
                rows.append(obs[b, t] + self.initial if self._frames[b] == 0 else self._row(rows[-1], obs[b, t]))
                self._frames[b] += 1
            self._held = max(self._held, len(rows))
            n, base = int(self._frames[b]), int(self._base[b])
            c, state = -1, 0
            if f[b] > 0 and S == 1:
                c = n - 1
            elif f[b] > 0 and n - base >= 2:
                first = n - len(rows)
                memo = self._memo[b]
                alive = torch.arange(S)
                for t in range(n - 1, base, -1):                      # alive: the set at frame t
                    alive = torch.unique(self._backpointers(rows[t - 1 - first], alive))
                    k = int(alive.numel())
                    if k == 1:
                        c, state = t - 1, int(alive[0])
                        break
                    # same size as an earlier walk's set here: the same set, and that walk found no single state below
                    same = memo.get(t - 1) == k
                    memo[t - 1] = k
                    if same:
                        break
            if self.max_lag is not None and f[b] > 0 and n - 1 - self.max_lag > max(c, base - 1):
                # more than max_lag frames would stay: the oldest leave along the path that is best at the newest frame
                # (the decided frames lie on it as on every survivor)
                target, first = n - 1 - self.max_lag, n - len(rows)
                self._forced[b] += target - max(c, base - 1)
                state = self._final_state(rows[-1])
                for t in range(n - 1, target, -1):
                    state = int(self._backpointers(rows[t - 1 - first], torch.tensor([state]))[0])
                c = target
            if c >= 0:
                result.append(self._backtrace_host(b, c, state))
                self._base[b] = c + 1
                keep = n - (c + 1) + 1                                # pending rows and the one before them
                del rows[:max(0, len(rows) - keep)]
                for t in [t for t in self._memo[b] if t <= c]:
                    del self._memo[b][t]
            else:
                result.append(torch.empty(0, dtype=torch.int32))
        return result

    def _flush_host(self, b: int) -> torch.Tensor:
        n, base = int(self._frames[b]), int(self._base[b])
        out = torch.empty(0, dtype=torch.int32)
        if n > base:
            out = self._backtrace_host(b, n - 1, self._final_state(self._rows[b][-1]))
        self._rows[b], self._memo[b] = [], {}
        return out

    # ------------------------------------------------------------------ HIP route
    def _prepare_band(self, original: torch.Tensor, route: str):
        """(reach_left, reach_right, background, diagonals) where the band route takes the decoder's matrix, else None --
        or, under 'band', a RuntimeError that names the reason.  The diagonals come from a private copy of the matrix, so that
        the look, the extraction and the device's verdict all speak of the same values whatever the caller later writes."""
        over, reason = _band_plan(self.transition, original, self.batch, self.states, self.device.index or 0)
        if over is not None:
            diagonals, reason = self._band_diagonals('torbi_hip_stream_band_diagonals_bytes', 'torbi_hip_stream_band_prepare',
                                                     self.transition.clone(), over)
            if diagonals is not None:
                return (*over, diagonals)
        return band_route.choose(route, None, reason, None, "StreamDecoder(route='band')")

    def _grow(self, capacity: int) -> None:
        """Ring of round_capacity(`capacity`) slots (a push that needs more than the old ring at least doubles it); pending
        rows and the newest row move to their new slots by one device copy, the walk memo starts empty.  On the band route the
        rows are the pending frames' pointer rows (moved through an int32 view) and the newest row is the carried row behind
        the memo."""
        B, S = self.batch, self.states
        capacity = self.round_capacity(capacity)
        nbytes = self._lib.torbi_hip_stream_state_bytes(B, S, capacity)
        if nbytes == 0:
            raise ValueError('torbi_hip_stream_state_bytes rejected the shape')
        state = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
        ring = state[:B * capacity * S * 4].view(torch.float32).view(B, capacity, S)
        state[B * capacity * S * 4:B * capacity * (S + 1) * 4].zero_()
        if self._state is not None and self._band is not None:
            old = self._state[:B * self._capacity * S * 4].view(torch.int32).view(B, self._capacity, S)
            self._move([(ring.view(torch.int32), old)], self._moving(self._base), capacity)
            state[B * capacity * (S + 1) * 4:nbytes] = self._state[B * self._capacity * (S + 1) * 4:self._state_bytes]
        elif self._state is not None:
            self._move([(ring, self._ring())], self._newest_and_pending(), capacity)
        self._state, self._capacity, self._state_bytes = state, capacity, nbytes

    def _ring(self) -> torch.Tensor:
        B, S, cap = self.batch, self.states, self._capacity
        return self._state[:B * cap * S * 4].view(torch.float32).view(B, cap, S)

    def _results(self, out: torch.Tensor, counts: torch.Tensor, what: str) -> np.ndarray:
        """`counts` (B,) or, from a push with a maximum lag, (2, B): counts and forced counts, read back in one copy."""
        got = counts.cpu().numpy().astype(np.int64)           # (the one host synchronisation of the call)
        if (got < 0).any():
            raise _lib.TorbiHipError(f'{what}: stream state does not match the call (counts {got.tolist()})')
        return got

    def _push_device(self, obs: torch.Tensor, f: np.ndarray) -> List[torch.Tensor]:
        B, S = self.batch, self.states
        pending = self._frames - self._base
        need = int((pending + f).max())
        if need > self._capacity:
            self._grow(need)
        info = self._info(pending, f)
        out = torch.empty((B, max(1, need)), dtype=torch.int32, device=self.device)
        _, index, stream = _lib.launch(self.device)
        Tc = int(obs.shape[1])
        if self._band is not None:
            left, right, background, diagonals = self._band
            lag = self.max_lag is not None
            counts = torch.empty((2, B) if lag else (B,), dtype=torch.int32, device=self.device)
            _lib.check(self._lib.torbi_hip_stream_band_push(
                obs.data_ptr() if Tc > 0 else None, Tc, info.data_ptr(), diagonals.data_ptr(), self.initial.data_ptr(), left, right,
                ctypes.c_float(background), self._state.data_ptr(), self._state_bytes, self._capacity, out.data_ptr(), out.shape[1],
                counts.data_ptr(), min(self.max_lag, 2 ** 31 - 1) if lag else -1, counts[1].data_ptr() if lag else None,
                B, S, index, stream), 'torbi_hip_stream_band_push')
            got = self._results(out, counts, 'torbi_hip_stream_band_push')
            if lag:
                got, forced = got
                self._forced += forced
        elif self.max_lag is None:
            counts = torch.empty(B, dtype=torch.int32, device=self.device)
            _lib.check(self._lib.torbi_hip_stream_push(
                obs.data_ptr() if Tc > 0 else None, Tc, info.data_ptr(), self.transition.data_ptr(), self._transposed.data_ptr(),
                self.initial.data_ptr(), self._state.data_ptr(), self._state_bytes, self._capacity, out.data_ptr(), out.shape[1],
                counts.data_ptr(), B, S, index, stream), 'torbi_hip_stream_push')
            got = self._results(out, counts, 'torbi_hip_stream_push')
        else:
            counts = torch.empty((2, B), dtype=torch.int32, device=self.device)      # counts, then forced counts
            _lib.check(self._lib.torbi_hip_stream_push_lag(
                obs.data_ptr() if Tc > 0 else None, Tc, info.data_ptr(), self.transition.data_ptr(), self._transposed.data_ptr(),
                self.initial.data_ptr(), self._state.data_ptr(), self._state_bytes, self._capacity, out.data_ptr(), out.shape[1],
                counts[0].data_ptr(), min(self.max_lag, 2 ** 31 - 1), counts[1].data_ptr(), B, S, index, stream),
                'torbi_hip_stream_push_lag')
            got, forced = self._results(out, counts, 'torbi_hip_stream_push_lag')
            self._forced += forced
        self._frames += f
        self._base += got
        return [out[b, :got[b]] for b in range(B)]

    def _flush_device(self, marks: np.ndarray) -> dict:
        B, S = self.batch, self.states
        pending = self._frames - self._base
        info = self._info(pending, marks)
        out = torch.empty((B, max(1, int(pending.max()))), dtype=torch.int32, device=self.device)
        counts = torch.empty(B, dtype=torch.int32, device=self.device)
        _, index, stream = _lib.launch(self.device)
        if self._band is not None:
            _lib.check(self._lib.torbi_hip_stream_band_flush(
                info.data_ptr(), self._state.data_ptr(), self._state_bytes, self._capacity, out.data_ptr(), out.shape[1],
                counts.data_ptr(), B, S, index, stream), 'torbi_hip_stream_band_flush')
        else:
            _lib.check(self._lib.torbi_hip_stream_flush(
                info.data_ptr(), self.transition.data_ptr(), self._state.data_ptr(), self._state_bytes, self._capacity,
                out.data_ptr(), out.shape[1], counts.data_ptr(), B, S, index, stream),
                'torbi_hip_stream_flush')
        got = self._results(out, counts, 'torbi_hip_stream_flush')
        return {k: out[k, :got[k]] for k in np.flatnonzero(marks).tolist()}
