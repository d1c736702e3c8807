"""What the StreamDecoder(max_lag=...) tests of both routes share, built on tests/stream_cases.py: the brute-force rule of a
bounded push and a feeding loop that checks every push against it.

The rule needs no new oracle.  A stream with n frames, the first `base` of them returned, that receives at least one frame
returns frames base .. c, c = max(c_nat, n - 1 - max_lag), where c_nat is the newest frame `stream_cases.decided` finds; and
what it returns is that span of the whole-sequence decode (`stream_cases.reference_path`) of its first n frames."""
import math

import numpy as np
import torch

from torbi_amd import synth
from stream_cases import plan, clamp, reference_arrays, reference_path, decided


def identity(S):
    eye = np.full((S, S), -np.inf, np.float32)
    np.fill_diagonal(eye, 0.)
    return eye


def prefix_path(post, bp, n):
    """`reference_path` of the first n frames, from the whole sequence's arrays (a prefix of the recurrence is the
    recurrence of the prefix): the final state is the first NaN of row n - 1, otherwise its first maximum."""
    nan = np.isnan(post[n - 1])
    state = int(nan.argmax()) if nan.any() else int(post[n - 1].argmax())
    path = [state]
    for t in range(n - 1, 0, -1):
        state = int(bp[t][state])
        path.append(state)
    return np.array(path[::-1], dtype=np.int32)


class Expected:
    """The brute-force bounded decoder of one stream: `push(f)` and `flush()` return what the decoder must return."""

    def __init__(self, seq, trans, init, max_lag):
        self.S, self.max_lag = seq.shape[1], max_lag
        self.post, self.bp = reference_arrays(seq, trans, init)
        self.n = self.base = self.forced = 0

    def natural_pending(self):
        return self.n - (decided(self.bp, self.n, self.S) + 1) if self.n else 0

    def push(self, f):
        self.n += int(f)
        if f == 0:
            return np.empty(0, np.int32)
        c_nat = decided(self.bp, self.n, self.S)
        c = c_nat if self.max_lag is None else max(c_nat, self.n - 1 - self.max_lag)
        if c < self.base:
            return np.empty(0, np.int32)
        self.forced += c - max(c_nat, self.base - 1)
        out = prefix_path(self.post, self.bp, self.n)[self.base:c + 1]
        self.base = c + 1
        return out

    def flush(self):
        out = prefix_path(self.post, self.bp, self.n)[self.base:] if self.n > self.base else np.empty(0, np.int32)
        self.n = self.base = self.forced = 0
        return out


def chunk_of(source, pos, f, Tc, S):
    """(B, Tc, S) of a push: stream b's next f[b] frames, NaN where nothing may be read."""
    chunk = torch.full((len(source), Tc, S), math.nan)
    for b in range(len(source)):
        chunk[b, :f[b]] = torch.from_numpy(source[b][pos[b]:pos[b] + f[b]])
    return chunk


def feed_bounded(dec, source, trans, init, pushes, prepare=clamp, device=None, twin=None, after=None):
    """Push `source[b]` (frames, S) piece by piece to a decoder with a maximum lag and check after EVERY push, per stream:
    the output is frames base .. base + count - 1 of the whole decode of the stream's first n frames, `pending` is
    min(natural pending, max_lag), `forced` the brute-force count, a stream without frames returns nothing and its
    `forced` does not move.  `prepare`: the epsilon round trip of the decoder's device.  `twin`: a second decoder (the
    host's) fed the same chunks, whose outputs, pending and forced must equal the first's bit for bit.  `after(k, dec)`
    runs after push k.  Returns the outputs per push (lists of arrays), flush last, and the expectations."""
    B, S, max_lag = len(source), dec.states, dec.max_lag
    want = [Expected(prepare(source[b]), trans, init, max_lag) for b in range(B)]
    pos = np.zeros(B, dtype=np.int64)
    outputs = []
    for k, (Tc, f) in enumerate(pushes):
        f = np.asarray(f)
        chunk = chunk_of(source, pos, f, Tc, S)
        before = dec.forced.clone()
        out = [o.cpu().numpy() for o in dec.push(chunk if device is None else chunk.to(device), torch.from_numpy(f))]
        pos += f
        for b in range(B):
            exp = want[b].push(f[b])
            assert out[b].dtype == np.int32 and np.array_equal(out[b], exp), (k, b, out[b], exp)
            natural = want[b].natural_pending()
            bound = natural if max_lag is None or f[b] == 0 else min(natural, max_lag)
            assert int(dec.pending[b]) == want[b].n - want[b].base, (k, b, dec.pending, want[b].n, want[b].base)
            if f[b] > 0:
                assert int(dec.pending[b]) == bound, (k, b, int(dec.pending[b]), natural, max_lag)
            else:
                assert out[b].size == 0 and int(dec.forced[b]) == int(before[b]), (k, b)
            assert max_lag is None or int(dec.pending[b]) <= max_lag
            assert int(dec.forced[b]) == want[b].forced, (k, b, dec.forced, want[b].forced)
        assert dec.frames.tolist() == pos.tolist()
        if twin is not None:
            other = [o.numpy() for o in twin.push(chunk, torch.from_numpy(f))]
            assert all(np.array_equal(a, o) for a, o in zip(out, other)), (k, out, other)
            assert torch.equal(dec.pending, twin.pending) and torch.equal(dec.forced, twin.forced), k
        outputs.append(out)
        if after is not None:
            after(k, dec)
    rest = [r.cpu().numpy() for r in dec.flush()]
    for b in range(B):
        exp = want[b].flush()
        assert np.array_equal(rest[b], exp), ('flush', b, rest[b], exp)
    if twin is not None:
        assert all(np.array_equal(a, o.numpy()) for a, o in zip(rest, twin.flush()))
    assert (dec.frames == 0).all() and (dec.pending == 0).all() and (dec.forced == 0).all()
    outputs.append(rest)
    return outputs, want


def reference_prefix_check(seq, trans, init, n):
    """`prefix_path` IS `reference_path` of the prefix (asserted where a test wants the reassurance)."""
    post, bp = reference_arrays(seq, trans, init)
    assert np.array_equal(prefix_path(post, bp, n), reference_path(seq[:n], trans, init))


def nonfinite_scenario(make, max_lag, prepare=clamp, device=None):
    """`make(B, S, trans, init, max_lag)` builds the decoder.  On an identity matrix (nothing is ever decided) a NaN at
    states 2 and 5 of the newest row: the forced path starts at the first NaN.  An all -inf matrix: every row after the first
    is -inf, every backpointer and every final state a tie, and ties go to state 0."""
    B, T, S = 2, 10, 7
    obs, _, init = synth.problem(B, T, S, seed=3)
    obs = obs.copy()
    obs[0, 4, [5, 2]] = np.nan
    source = [obs[b] for b in range(B)]
    outputs, _ = feed_bounded(make(B, S, identity(S), init, max_lag), source, identity(S), init, plan(B, T, 'one'),
                              prepare=prepare, device=device)
    if max_lag == 0:                                          # the frame returned is the newest: its final state
        assert outputs[4][0].tolist() == [2]
    dead = np.full((S, S), -np.inf, np.float32)
    outputs, _ = feed_bounded(make(B, S, dead, init, max_lag), [source[1]] * B, dead, init, plan(B, T, 'ragged', seed=1),
                              prepare=prepare, device=device)
    paths = [np.concatenate([o[b] for o in outputs]) for b in range(B)]
    assert all(len(p) == T and (p[1:] == 0).all() for p in paths)


def flush_scenario(make, prepare=clamp, device=None):
    """`flush(items=[k])` half-way on an identity matrix (every stream forces from its fourth frame on): stream k restarts
    from `initial` with forced[k] == 0 and returns what a decoder of its own returns for the remaining frames; its
    neighbours go on as if nothing had happened."""
    B, T, S, k, max_lag = 3, 12, 5, 1, 2
    obs, _, init = synth.problem(B, 2 * T, S, seed=50)
    source, eye = [obs[b] for b in range(B)], identity(S)
    dec = make(B, S, eye, init, max_lag)
    pos = np.zeros(B, dtype=np.int64)
    ones = np.ones(B, dtype=np.int64)

    def pushes(into):
        for _ in range(T):
            chunk = chunk_of(source, pos, ones, 1, S)
            for b, o in enumerate(dec.push(chunk if device is None else chunk.to(device))):
                into[b].append(o.cpu().numpy())
            pos[:] += ones
    first, second = [[] for _ in range(B)], [[] for _ in range(B)]
    pushes(first)
    assert dec.forced.tolist() == [T - max_lag] * B
    rest = dec.flush(items=[k])[0].cpu().numpy()
    assert dec.forced.tolist() == [T - max_lag, 0, T - max_lag] and dec.frames.tolist() == [T, 0, T]
    assert dec.pending.tolist() == [max_lag, 0, max_lag] and len(rest) == max_lag
    pushes(second)
    assert dec.forced.tolist() == [2 * T - max_lag, T - max_lag, 2 * T - max_lag]
    tail = [r.cpu().numpy() for r in dec.flush()]
    # the same streams, each in one piece, checked push by push against the brute-force rule
    outputs, _ = feed_bounded(make(B, S, eye, init, max_lag), [source[0], source[k][T:], source[2]], eye, init,
                              [(1, ones)] * T + [(1, np.array([1, 0, 1]))] * T, prepare=prepare, device=device)
    whole = [np.concatenate([o[b] for o in outputs]) for b in range(B)]
    assert np.array_equal(np.concatenate(second[k] + [tail[k]]), whole[k])
    for b in (0, 2):
        assert np.array_equal(np.concatenate(first[b] + second[b] + [tail[b]]), whole[b]), b
