"""What the StreamDecoder tests of both routes share: push plans, the feeding loop, and references that are independent of
the decoder -- the reference's recurrence in numpy float32 and the brute-force survivor-set rule for what a push must
commit."""
import math

import numpy as np
import torch

def plan(B, T, mode, seed=0):
    """Per push: (Tc, frames per stream) for streams of T frames each (ragged modes: streams end at different times)."""
    rng = np.random.default_rng(seed)
    if mode == 'all':
        return [(T, np.full(B, T))]
    if mode == 'one':
        return [(1, np.ones(B, dtype=np.int64))] * T
    left, pushes = np.full(B, T), []
    while left.any():
        Tc = int(rng.integers(1, 9))
        f = np.minimum(left, rng.integers(0, Tc + 1, size=B)) if mode == 'ragged' else np.minimum(left, Tc)
        left -= f
        pushes.append((Tc, f))
    return pushes


def feed(dec, source, pushes, check=None, device=None):
    """Push `source[b]` (frames, S) to stream b piece by piece (invalid positions hold NaN: they must not be read), the
    chunks placed on `device` (None: the host); returns the concatenated outputs (flush included) and the frames pushed per stream."""
    B, S = len(source), dec.states
    pos = np.zeros(B, dtype=np.int64)
    got = [[] for _ in range(B)]
    for Tc, f in pushes:
        chunk = torch.full((B, Tc, S), math.nan)
        for b in range(B):
            chunk[b, :f[b]] = torch.from_numpy(source[b][pos[b]:pos[b] + f[b]])
        out = dec.push(chunk if device is None else chunk.to(device), torch.from_numpy(np.asarray(f)))
        for b in range(B):
            got[b].append(out[b].cpu())
        pos += f
        if check is not None:
            check(dec, pos)
    for b, rest in enumerate(dec.flush()):
        got[b].append(rest.cpu())
    assert (dec.frames == 0).all() and (dec.pending == 0).all()
    return [torch.cat(g).numpy() for g in got], pos


def clamp(obs):
    """The epsilon round trip from_probabilities applies to log inputs (what the oracle must be given)."""
    x = torch.from_numpy(np.ascontiguousarray(obs, dtype=np.float32)).clone()
    torch.exp_(x)
    x += torch.finfo(torch.float32).tiny
    torch.log_(x)
    return x.numpy()


def reference_arrays(seq, trans, init):
    """Posterior rows and backpointers with the reference's rules, numpy float32."""
    T, S = seq.shape
    post = np.empty((T, S), np.float32)
    bp = np.zeros((T, S), np.int64)
    post[0] = seq[0] + init
    for t in range(1, T):
        cand = post[t - 1][None, :] + trans
        nan = np.isnan(cand)
        masked = np.where(nan, -np.inf, cand)
        best = np.where(nan[:, 0], np.nan, masked.max(axis=1))
        bp[t] = np.where(nan[:, 0], 0, masked.argmax(axis=1))
        post[t] = seq[t] + best
    return post, bp


def decided(bp, n, S):
    """Frames 0 .. c are decided after n frames: the largest c whose ancestor set of all S states is one state (-1)."""
    alive = np.arange(S)
    if S == 1:
        return n - 1
    for t in range(n - 1, 0, -1):
        alive = np.unique(bp[t][alive])
        if alive.size == 1:
            return t - 1
    return -1


def reference_path(seq, trans, init):
    """The decoded path of one sequence from `reference_arrays`: the final state is the first NaN of the last row, otherwise
    its first maximum; then the backpointers."""
    post, bp = reference_arrays(seq, trans, init)
    nan = np.isnan(post[-1])
    state = int(nan.argmax()) if nan.any() else int(post[-1].argmax())
    path = [state]
    for t in range(len(seq) - 1, 0, -1):
        state = int(bp[t][state])
        path.append(state)
    return np.array(path[::-1], dtype=np.int32)


def commit_checker(source, trans, init, prepare=clamp):
    """A `check` for `feed`: after every push, `pending` is what the brute-force rule leaves.  `prepare`: the epsilon round
    trip the decoder's device applies (the host's by default)."""
    B, S = len(source), source[0].shape[1]
    bps = [reference_arrays(prepare(source[b]), trans, init)[1] for b in range(B)]

    def check(dec, pos):
        for b in range(B):
            n = int(pos[b])
            want = n - (decided(bps[b], n, S) + 1) if n else 0
            assert int(dec.pending[b]) == want, (b, n, int(dec.pending[b]), want)
        assert dec.frames.tolist() == pos.tolist()
    return check
