"""Online filtering and fixed-lag smoothing: the forward-backward recurrence of POSTERIOR.md on frames that arrive in pieces.

A stream holds n frames, the first `base` of them already returned.  A push that brings a stream f >= 1 frames returns, with
n' = n + f, the rows gamma_{t|n'} = P(state_t = j | frames 0 .. n' - 1) for t = base .. n' - 1 - lag: the corresponding rows of
`state_posteriors` on the stream's first n' frames (the rule `StreamDecoder(max_lag=...)` follows for indices).  `filtered()`
is the newest row, `log_likelihood` the running log P(frames so far), `flush` the remaining rows.  The HIP route is
csrc/stream_posterior.hpp behind torbi_hip_stream_posterior_* (include/torbi_hip.h); `gpu=None` runs the same rule on the
host in float64 with torch CPU ops.  STREAM.md, "Streaming posteriors", has the layout, the kernels and the numbers.

A matrix that holds ONE value outside a band (the pitch matrix of a live pitch tracker: 23 diagonals of 1440 states) can
take the band route on the device (csrc/stream_posterior_band.hpp behind torbi_hip_stream_smooth_band_*; STREAM.md,
"Streaming posteriors: band route"): a step costs the band, not the matrix.  `route` and `band` choose.
"""
import ctypes
import math
import operator
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib, band_route, inputs, stream_ring
from .stream_ring import INITIAL_CAPACITY

ROUTES = band_route.ROUTES
# Where 'auto' takes a covered band: the classes in which tools/stream_posterior_probe.py --band measured the band route's
# slowest of five runs faster than the dense route's fastest of five (STREAM.md, "Streaming posteriors: band route").  Each
# entry: (smallest batch, largest batch, diagonals of 1440 states).  Measured, all on 23 diagonals of 1440 states in both forms
# of the background at lag 8: 1 stream in one-frame pushes (27 x), 8 streams in pushes of 15 (61 x), 512 streams in pushes of
# 100 (33 x).  Anything outside -- a larger batch, a band that holds more of a row -- is not measured and stays dense.
_AUTO_BAND = ((1, 512, 23),)


def _covered(batch, states, reach_left, reach_right, background, index=0) -> bool:
    """torbi_hip_stream_smooth_band_covers: the band route takes this many streams, this band and background."""
    return bool(_lib.load().torbi_hip_stream_smooth_band_covers(int(batch), int(states), reach_left, reach_right, background,
                                                                index))


def _band_pays(batch: int, states: int, reach_left: int, reach_right: int) -> bool:
    return any(low <= batch <= high and band_route.share_within(states, reach_left, reach_right, diagonals)
               for low, high, diagonals in _AUTO_BAND)


def _band_plan(trans: torch.Tensor, original: torch.Tensor, batch: int, states: int, index: int):
    """`band_route.plan` for this feature: the shape is what torbi_hip_stream_smooth_band_covers takes."""
    return band_route.plan(trans, original, _covered, 'torbi_hip_stream_smooth_band_covers',
                           dict(batch=int(batch), states=int(states)), index)


def _stated_band(band):
    """`band=` of the constructor as (reach_left, reach_right, background), or a ValueError."""
    try:
        reach_left, reach_right, background = band
        return band_route.stated(operator.index(reach_left), operator.index(reach_right), background)
    except (TypeError, ValueError, RuntimeError) as error:
        raise ValueError(f'band must be (reach_left >= 0, reach_right >= 0, background); got {band!r} ({error})') from None


def stream_posterior_route(transition: Optional[torch.Tensor], batch: int, states: int, gpu: Optional[int] = 0,
                           log_probs: bool = False) -> str:
    """The route `StreamPosteriors(batch, states, transition, log_probs=log_probs, gpu=gpu, route='auto')` takes: 'band' (one
    value outside a band the band kernels cover, in a class where the band route was measured faster), 'dense', or 'host'
    for `gpu=None`.  `transition=None` is 'dense'."""
    if gpu is None:
        return 'host'
    if transition is None:
        return 'dense'
    states = int(states)
    if tuple(transition.shape) != (states, states):
        raise ValueError(f'transition must be ({states}, {states})')
    device, original, trans, _ = stream_ring.model(transition, None, log_probs, states, gpu)
    band, why = _band_plan(trans, original, batch, states, device.index or 0)
    pays = lambda left, right, background: _band_pays(int(batch), states, left, right)
    return 'dense' if band_route.choose('auto', band, why, pays, 'stream_posterior_route') is None else 'band'


class StreamPosteriors(stream_ring.StreamRing):
    """State posteriors of `batch` independent streams whose frames arrive in pieces; memory per stream is bounded by `lag`.

    `transition` (states, states) [next, prev], `initial` (states,), `log_probs` and `gpu` mean what they mean to
    `StreamDecoder` and `state_posteriors`, defaults included, and go through the same preparation (torbi_amd/inputs.py);
    `transition=None` is the constant matrix it stands for.  `lag` (an integer >= 0, required to be one): how many frames
    a row waits for before it leaves.

        sp = StreamPosteriors(batch, states, transition, initial, lag=8)
        rows = sp.push(observation)       # (batch, Tc, states) -> `batch` float32 tensors (k_b, states), oldest frame first
        now = sp.filtered()               # (batch, states): P(state of the newest frame | frames so far)
        score = sp.log_likelihood         # (batch,): log P(frames so far)
        rest, final = sp.flush()          # the remaining rows of every stream and the final log-likelihoods

    * One-frame pushes give exact fixed-lag smoothing, gamma_{t|t+lag}; in a longer push the older frames see more than
      `lag` frames ahead, never fewer.  Afterwards `pending == min(pending + f, lag)`; a stream with f == 0 returns
      nothing and does not change.
    * Non-finite rules are POSTERIOR.md's: a stream whose running log-likelihood is not finite (total probability 0, or a
      NaN or +inf in anything it has read) gets NaN rows until it is flushed; other streams' bits never change for it.
    * A stream's bits depend on its own data and on (t, n') only: not on the batch it runs in, the cut into pushes or
      the ring's size.
    * Device memory per stream: (8 * states + 8) bytes per ring slot plus 8; `capacity` (a power of two, at least
      INITIAL_CAPACITY) never exceeds `round_capacity(lag + largest Tc pushed)`.  The host route holds at most lag + Tc
      rows per stream.
    * On the device exp(transition) and its transpose are built once, here, with torch.exp from a private copy of the matrix.

    `route` ('auto', 'dense' or 'band'; validated and otherwise ignored with `gpu=None`): which device route the decoder
    takes.  'dense', the default, is the route for any matrix, and every call that does not say otherwise keeps its bits.
    'band' is the band route for a matrix that holds one value outside a band: `viterbi.band_over` finds the band,
    torbi_hip_stream_smooth_band_covers says whether the kernels take it, and the constructor builds the diagonals from a
    private copy of the matrix and reads the device's verdict on it back once (its one read-back; `push`, `flush`,
    `filtered()` and `log_likelihood` still never synchronise).  It raises RuntimeError, naming the reason, where any of
    these says no.  'auto' takes the band route where all of them say yes and the class was measured faster
    (`torbi_amd.stream_posterior_route` answers which), else the dense route.
    `band=(reach_left, reach_right, background)` states the band instead of looking for it -- every entry [next j][prev i]
    outside j - reach_left <= i <= j + reach_right (log scores, after the preparation) equals `background` -- which also
    reaches what the look cannot answer for (1 <= states <= 4096, odd counts included; min(reach_left + reach_right + 1,
    states) <= 64).  A band the kernels do not cover, or a matrix that breaks the promise, raises RuntimeError; `band=`
    with route='dense' is a ValueError.  `sp.route` tells: 'band', 'dense' or 'host'.  The state, the memory per slot and the
    rules above are the same on either device route; the bits of the two differ (within 2e-4).
    """

    def __init__(self, batch: int, states: int, transition: Optional[torch.Tensor] = None,
                 initial: Optional[torch.Tensor] = None, log_probs: bool = False, gpu: Optional[int] = 0, lag: int = 8,
                 route: str = 'dense', band: Optional[Tuple[int, int, float]] = None):
        self._check(batch, states, route)
        if band is not None:
            band = _stated_band(band)
            if route == 'dense':
                raise ValueError("band= states a band for the band route: pass route='band' or 'auto' with it, not 'dense'")
        self.lag = stream_ring.depth('lag', lag)
        original, transition = self._model(batch, states, transition, initial, log_probs, gpu)
        if gpu is None:
            self._E = torch.exp(transition.to(torch.float64))                         # [next, prev]
            self._rows = [[] for _ in range(self.batch)]            # (a_t, e_t, c_t) of the pending frames
            self._carry = [None] * self.batch                       # (a, c) of the newest frame
            self._sum = [0.] * self.batch                           # running sums of log c_t + m_t
            self._held = 0
            self.route = 'host'
        else:
            self._lib = _lib.load()
            private = transition.clone()
            self._band = self._prepare_band(private, original, route, band)
            self.route = 'dense' if self._band is None else 'band'
            if self._band is None:
                self._expa = torch.exp(private).contiguous()        # [next, prev]
                self._expa_t = self._expa.t().contiguous()          # [prev, next]
            self._capacity = 0
            self._state = None
            self._grow(INITIAL_CAPACITY)

    # ------------------------------------------------------------------ public
    @property
    def log_likelihood(self) -> torch.Tensor:
        """(batch,) float32 on the compute device: log P(frames so far), the fp64 running sum of log c_t + m_t rounded on
        read; NaN where the sum is NaN or +inf, 0 for a stream without frames.  Reads nothing back."""
        if self.gpu is None:
            total = torch.tensor(self._sum, dtype=torch.float64)
        else:
            total = self._state[:8 * self.batch].view(torch.float64)
        started = self._mask(self._frames > 0)
        total = torch.where(started, total, torch.zeros_like(total))
        total = torch.where(torch.isnan(total) | (total == math.inf), torch.full_like(total, math.nan), total)
        return total.to(torch.float32)

    def filtered(self) -> torch.Tensor:
        """(batch, states) float32 on the compute device: P(state of the newest frame | frames so far), a_{n-1} / c_{n-1}
        (NaN where the running log-likelihood is not finite); zeros for a stream without frames.  Reads nothing back."""
        B, S = self.batch, self.states
        if self.gpu is None:
            a = torch.stack([torch.zeros(S, dtype=torch.float64) if k is None else k[0] for k in self._carry])
            c = torch.stack([torch.ones((), dtype=torch.float64) if k is None else k[1] for k in self._carry])
        else:
            slot = self._upload((np.maximum(self._frames, 1) - 1) % self._capacity)
            item = torch.arange(B, device=self.device)
            ring_a, _, ring_c, _ = self._rings()
            a, c = ring_a[item, slot], ring_c[item, slot]
        row = a / c[:, None]
        row = torch.where(torch.isfinite(self.log_likelihood)[:, None], row, torch.full_like(row, math.nan))
        return torch.where(self._mask(self._frames > 0)[:, None], row, torch.zeros_like(row)).to(torch.float32)

    def push(self, observation: torch.Tensor, frames: Optional[torch.Tensor] = None) -> List[torch.Tensor]:
        """Append frames to the streams and return the rows that reached the lag.

        observation (batch, Tc, states); frames (batch,) valid frames per stream, 0 .. Tc (None = all Tc).  Returns `batch`
        float32 tensors (k_b, states) on the compute device, oldest frame first: k_b = max(0, pending_b + f_b - lag) for
        f_b >= 1, else 0.  Performs NO host synchronisation: k_b is a function of values the host already holds, so nothing
        is read back (the per-call stream table goes to the device through pinned memory).
        """
        _, f = self._push_front(observation, frames)
        if not f.any():
            return [torch.empty((0, self.states), dtype=torch.float32, device=self.device) for _ in range(self.batch)]
        obs = inputs.observation(observation, self.log_probs, self.device)
        pending = self._frames - self._base
        counts = np.where(f > 0, np.maximum(pending + f - self.lag, 0), 0)
        if self.gpu is None:
            out = self._push_host(obs, f, counts)
        else:
            out = self._push_device(obs, f, counts)
        self._frames += f
        self._base += counts
        return out

    def flush(self, items: Optional[Sequence[int]] = None) -> Tuple[List[torch.Tensor], torch.Tensor]:
        """End streams `items` (default: all): (rows, final) with one (pending_k, states) float32 tensor per item, in the
        order given -- the stream's remaining frames as gamma_{t|n} -- and final (len(items),) float32, their log-likelihoods.
        The streams are reset: their next push starts from `initial`.  A stream without frames returns a (0, states) tensor
        and a log-likelihood of 0.  Reads nothing back."""
        items, marks = self._flush_front(items)
        final = self.log_likelihood[self._upload(np.asarray(items, dtype=np.int64))]
        chosen = np.flatnonzero(marks).tolist()
        if self.gpu is None:
            rest = {k: self._sweep_host(k, int(self._frames[k] - self._base[k])) for k in chosen}
            for k in chosen:
                self._rows[k], self._carry[k], self._sum[k] = [], None, 0.
        else:
            rest = self._flush_device(chosen, marks) if chosen else {}        # (no stream ends: nothing to launch)
        for k in chosen:
            self._frames[k] = self._base[k] = 0
        return [rest[k] for k in items], final

    # ------------------------------------------------------------------ shared
    def _upload(self, values: np.ndarray) -> torch.Tensor:
        """A small host array on the compute device without a host synchronisation (through pinned memory)."""
        host = torch.from_numpy(np.ascontiguousarray(values))
        if self.gpu is None:
            return host
        return host.pin_memory().to(self.device, non_blocking=True)

    def _mask(self, flags: np.ndarray) -> torch.Tensor:
        return self._upload(flags.astype(np.bool_))

    # ------------------------------------------------------------------ host route
    def _sweep_host(self, b: int, count: int, pending: Optional[int] = None) -> torch.Tensor:
        """gamma_{t|n} of the oldest `count` of stream b's `pending` newest rows (default: `count`), float32: one
        backward sweep from the newest row."""
        rows, S = self._rows[b], self.states
        if count == 0:
            return torch.empty((0, S), dtype=torch.float32)
        pending = rows[len(rows) - (count if pending is None else pending):]
        total = self._sum[b]
        out = torch.empty((count, S), dtype=torch.float64)
        beta = torch.ones(S, dtype=torch.float64)
        for r in range(len(pending) - 1, -1, -1):
            a, e, c = pending[r]
            if r < count:
                out[r] = a * beta / c
            beta = (e * beta / c) @ self._E
        if not math.isfinite(total):
            out.fill_(math.nan)
        return out.to(torch.float32)

    def _push_host(self, obs: torch.Tensor, f: np.ndarray, counts: np.ndarray) -> List[torch.Tensor]:
        result = []
        pi = self.initial.to(torch.float64)
        for b in range(self.batch):
            rows = self._rows[b]
            n = int(self._frames[b])
            for t in range(int(f[b])):
                x = obs[b, t].to(torch.float64)
                if n + t == 0:
                    x = x + pi
                m = torch.amax(x)                                                     # NaN propagates
                m = torch.zeros_like(m) if m == -math.inf else m
                e = torch.exp(x - m)
                if n + t == 0:
                    a = e
                else:
                    prev_a, prev_c = self._carry[b]
                    u = e * (self._E @ prev_a)
                    a = u * 0. if prev_c == 0 else u / prev_c
                c = a.sum()
                rows.append((a, e, c))
                self._carry[b] = (a, c)
                self._sum[b] = self._sum[b] + float(torch.log(c) + m)
            self._held = max(self._held, len(rows))
            pending_now = int(self._frames[b] - self._base[b] + f[b])
            result.append(self._sweep_host(b, int(counts[b]), pending_now))
            del rows[:int(counts[b])]
        return result

    # ------------------------------------------------------------------ HIP route
    def _prepare_band(self, private: torch.Tensor, original: torch.Tensor, route: str, stated):
        """(reach_left, reach_right, c_float(background), diagonals) where the decoder takes the band route, else None -- or a
        RuntimeError that names the reason, under 'band' and for a stated band.  The diagonals come from `private`, the
        decoder's own copy of the matrix, so that the look, the diagonals and the device's verdict all speak of the same values
        whatever the caller later writes."""
        B, S, index = self.batch, self.states, self.device.index or 0
        who = "StreamPosteriors(route='band')"
        if stated is not None:
            who = f'StreamPosteriors(band={stated!r})'
            if not _covered(B, S, *stated, index):
                raise RuntimeError(f'{who}: torbi_hip_stream_smooth_band_covers turns down batch={B}, states={S}, reach '
                                   f'{stated[0]}/{stated[1]}, background {stated[2]}')
            over = stated
        elif route == 'dense':
            return None
        else:
            over = band_route.choose(route, *_band_plan(private, original, B, S, index),
                                     lambda left, right, background: _band_pays(B, S, left, right), who)
            if over is None:
                return None
        diagonals, reason = self._band_diagonals('torbi_hip_stream_smooth_band_diagonals_size',
                                                 'torbi_hip_stream_smooth_band_prepare', private, over)
        if diagonals is not None:
            return over[0], over[1], ctypes.c_float(over[2]), diagonals
        if stated is not None:
            raise RuntimeError(f'{who}: {reason}')
        return band_route.choose(route, None, reason, None, who)

    def _rings(self, state=None, capacity=None):
        """(a (B, cap, S), e (B, cap, S), c (B, cap), m (B, cap)) float32 views of the state."""
        state = self._state if state is None else state
        cap = self._capacity if capacity is None else capacity
        B, S = self.batch, self.states
        at, views = 8 * B, []
        for shape in ((B, cap, S), (B, cap, S), (B, cap), (B, cap)):
            size = 4 * int(np.prod(shape))
            views.append(state[at:at + size].view(torch.float32).view(shape))
            at += size
        return views

    def _grow(self, slots: int) -> None:
        """Ring of round_capacity(slots) slots; the running sums and the rows of the pending frames and of the newest frame
        move to their new slots by device copies."""
        B, S = self.batch, self.states
        capacity = self.round_capacity(slots)
        nbytes = self._lib.torbi_hip_stream_posterior_state_size(B, S, capacity)
        if nbytes == 0:
            raise ValueError('torbi_hip_stream_posterior_state_size rejected the shape')
        state = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
        if self._state is not None:
            state[:8 * B] = self._state[:8 * B]
            self._move(zip(self._rings(state, capacity), self._rings()), self._newest_and_pending(), capacity)
        self._state, self._capacity, self._state_bytes = state, capacity, nbytes

    def _push_device(self, obs: torch.Tensor, f: np.ndarray, counts: np.ndarray) -> List[torch.Tensor]:
        B, S = self.batch, self.states
        pending = self._frames - self._base
        need = int((pending + f).max())
        if need > self._capacity:
            self._grow(need)
        info = self._info(pending, f)
        out = torch.empty((B, max(1, int(counts.max())), S), dtype=torch.float32, device=self.device)
        _, index, stream = _lib.launch(self.device)
        tail = (self._state.data_ptr(), self._state_bytes, self._capacity, out.data_ptr(), out.shape[1], None,
                min(self.lag, 2 ** 31 - 1), B, S, index, stream)
        if self._band is not None:
            left, right, background, diagonals = self._band
            _lib.check(self._lib.torbi_hip_stream_smooth_band_push(
                obs.data_ptr(), int(obs.shape[1]), info.data_ptr(), diagonals.data_ptr(), left, right, background,
                self.initial.data_ptr(), *tail), 'torbi_hip_stream_smooth_band_push')
        else:
            _lib.check(self._lib.torbi_hip_stream_posterior_push(
                obs.data_ptr(), int(obs.shape[1]), info.data_ptr(), self._expa.data_ptr(), self._expa_t.data_ptr(),
                self.initial.data_ptr(), *tail), 'torbi_hip_stream_posterior_push')
        return [out[b, :counts[b]] for b in range(B)]

    def _flush_device(self, items: List[int], marks: np.ndarray) -> dict:
        B, S = self.batch, self.states
        pending = self._frames - self._base
        info = self._info(pending, marks)
        out = torch.empty((B, max(1, int(pending[items].max())), S), dtype=torch.float32, device=self.device)
        _, index, stream = _lib.launch(self.device)
        tail = (self._state.data_ptr(), self._state_bytes, self._capacity, out.data_ptr(), out.shape[1], None, B, S, index, stream)
        if self._band is not None:
            left, right, background, diagonals = self._band
            _lib.check(self._lib.torbi_hip_stream_smooth_band_flush(info.data_ptr(), diagonals.data_ptr(), left, right, background,
                                                                    *tail), 'torbi_hip_stream_smooth_band_flush')
        else:
            _lib.check(self._lib.torbi_hip_stream_posterior_flush(info.data_ptr(), self._expa.data_ptr(), *tail),
                       'torbi_hip_stream_posterior_flush')
        return {k: out[k, :pending[k]] for k in items}
