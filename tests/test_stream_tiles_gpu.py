"""torbi_amd.StreamDecoder's HIP route where tests/test_stream_gpu.py does not reach: every instantiation of the forward
kernel (streams per workgroup G = 1 .. 16, J = 1 and 4 next-states per thread) with partial last tiles, uneven pushes and
fresh streams beside carried ones; ring growth with a wrapped window; forced ties; the maximal-commit rule by brute force;
state-count edges; and the C ABI's answer to an info that does not fit.

The references are independent of the code under test: the C oracle and the numpy recurrence of tests/stream_cases.py, both
given the epsilon round trip computed by plain torch ops ON THE DEVICE (exp_, += tiny, log_: the values the decoder sees,
which matters once scores tie), and the device's whole-sequence decode (other kernels) as the cross-check of every stream."""
import ctypes
import math

import numpy as np
import pytest
import torch

import oracle
import torbi_amd
from torbi_amd import _lib, synth
from torbi_amd.stream import INITIAL_CAPACITY
from stream_cases import plan, feed, reference_arrays, reference_path, decided, commit_checker

pytestmark = pytest.mark.gpu

DEV = torch.device('cuda:0')


def tile(B, S):
    return _lib.load().torbi_hip_stream_tile(B, S, 0)


def clamp(obs):
    """log(exp(x) + tiny) by torch ops on the device."""
    x = torch.from_numpy(np.ascontiguousarray(obs, dtype=np.float32)).to(DEV)
    torch.exp_(x)
    x += torch.finfo(torch.float32).tiny
    torch.log_(x)
    return x.cpu().numpy()


def decoder(B, S, trans, init, gpu=0):
    where = DEV if gpu is not None else 'cpu'
    return torbi_amd.StreamDecoder(B, S, None if trans is None else torch.from_numpy(trans).to(where),
                                   None if init is None else torch.from_numpy(init).to(where), log_probs=True, gpu=gpu)


def device_whole(segments, trans, init):
    """from_probabilities(gpu=0) of a list of (n, S) sequences (n may be 0): a list of index arrays."""
    S = trans.shape[0]
    n = np.array([len(s) for s in segments])
    batch = np.zeros((len(segments), max(1, int(n.max())), S), np.float32)
    for k, s in enumerate(segments):
        batch[k, :len(s)] = s
    frames = torch.from_numpy(np.maximum(n, 1).astype(np.int32)).to(DEV)
    got = torbi_amd.from_probabilities(torch.from_numpy(batch).to(DEV), frames, torch.from_numpy(trans).to(DEV),
                                       torch.from_numpy(init).to(DEV), True, gpu=0).cpu().numpy()
    return [got[k, :n[k]] for k in range(len(segments))]


def oracle_whole(segments, trans, init):
    """The oracle on the clamped sequences (every n >= 1)."""
    S = trans.shape[0]
    n = np.array([len(s) for s in segments], np.int32)
    batch = np.zeros((len(segments), int(n.max()), S), np.float32)
    for k, s in enumerate(segments):
        batch[k, :len(s)] = s
    got = oracle.decode(clamp(batch), n, trans, init, num_threads=oracle.max_threads())
    return [got[k, :n[k]] for k in range(len(segments))]


def check_streams(source, trans, init, pushes, references=True, check=None):
    """Feed `source` to a device decoder; every stream against the device's whole-sequence decode, the oracle and the numpy
    recurrence."""
    B, S = len(source), source[0].shape[1]
    dec = decoder(B, S, trans, init)
    got, pos = feed(dec, source, pushes, check=check, device=DEV)
    fed = [source[b][:pos[b]] for b in range(B)]
    for b, want in enumerate(device_whole(fed, trans, init)):
        assert np.array_equal(got[b], want), ('device', b, got[b], want)
    if references:
        some = [b for b in range(B) if pos[b] > 0]
        for b, want in zip(some, oracle_whole([fed[b] for b in some], trans, init)):
            assert np.array_equal(got[b], want), ('oracle', b, got[b], want)
            path = reference_path(clamp(fed[b]), trans, init)
            assert np.array_equal(got[b], path), ('numpy', b, got[b], path)
    return got, pos


# ------------------------------------------------------------------------------------------------------- D1: tiles
def smallest_batch(G, S):
    """The smallest B whose push runs G streams per workgroup at S states on device 0 (None: no B does)."""
    lo, hi = 1, 1 << 16
    if tile(hi, S) < G:
        return None
    while lo < hi:
        mid = (lo + hi) // 2
        if tile(mid, S) >= G:
            hi = mid
        else:
            lo = mid + 1
    return lo if tile(lo, S) == G else None


# (G the push must run, S, G the batch is sized for at S = 64 / 63): the last three are capped by the LDS (2 * G * S floats),
# not by the batch.  Ring of the largest: 16 slots * 4084 streams * 516 states * 4 B = 135 MB on 256 compute units.
TILE_CASES = [(G, S, G) for G in (1, 2, 4, 8, 16) for S in (64, 63)] + [(8, 516, 16), (4, 1025, 8), (2, 2052, 4)]


@pytest.mark.parametrize('G,S,sized_for', TILE_CASES, ids=[f'G{G}-S{S}' for G, S, _ in TILE_CASES])
def test_tile_matrix(G, S, sized_for):
    """stream_forward_kernel<G, J> (J = 4 where S % 4 == 0, else 1), proven by torbi_hip_stream_tile: ragged pushes in which
    every tile has a stream with 0 frames and one with all Tc, a partial last tile, streams of different lengths, NaN where
    nothing may be read, and three streams flushed half-way that restart from `initial` beside carried neighbours."""
    small = 64 if S % 4 == 0 else 63
    B = smallest_batch(sized_for, small)
    if B is None:
        pytest.skip(f'no batch gives {sized_for} streams per workgroup on this device')
    B += 3
    while G > 1 and B % G == 0:        # (the smallest batch of G = 2 is odd: + 3 would fill the last tile)
        B += 1
    assert tile(B, small) == sized_for and tile(B, S) == G, (B, tile(B, small), tile(B, S))
    assert G == 1 or B % G != 0
    print(f'stream_forward_kernel<{G}, {4 if S % 4 == 0 else 1}>: B = {B}, S = {S}')

    T = 16 if S < 512 else 12
    rng = np.random.default_rng(1000 * G + S)
    source, trans, init = synth.problem(B, T, S, seed=G + S)
    cut = rng.integers(T // 2, T + 1, size=B)                # where a stream stops taking frames of its own accord
    sizes = []
    while sum(sizes) < T:
        sizes.append(min(int(rng.integers(1, 5)), T - sum(sizes)))
    tiles = (B + G - 1) // G
    dec = decoder(B, S, trans, init)
    pos = np.zeros(B, dtype=np.int64)
    segments = [dict(b=b, start=0, got=[]) for b in range(B)]          # one per stream, one more per restart
    current = list(range(B))
    flushed = []
    for k, Tc in enumerate(sizes):
        f = np.minimum(rng.integers(0 if k else 1, Tc + 1, size=B), np.maximum(cut - pos, 0))   # (a stream to flush has frames)
        if G > 1:                                            # per tile: one stream without frames, one with all Tc
            first = np.arange(tiles) * G
            members = np.minimum(G, B - first)
            wide = members >= 2
            f[(first + k % members)[wide]] = 0
            f[(first + (k + 1) % members)[wide]] = Tc
            for t0, n in zip(first[wide], members[wide]):
                assert f[t0:t0 + n].min() == 0 and f[t0:t0 + n].max() == Tc
        assert (pos + f <= T).all()
        chunk = np.full((B, Tc, S), np.nan, np.float32)
        for t in range(Tc):
            rows = np.flatnonzero(f > t)
            chunk[rows, t] = source[rows, pos[rows] + t]
        out = dec.push(torch.from_numpy(chunk).to(DEV), torch.from_numpy(f))
        counts = np.array([o.numel() for o in out])
        pieces = np.split(torch.cat(out).cpu().numpy(), np.cumsum(counts)[:-1])
        for b in range(B):
            segments[current[b]]['got'].append(pieces[b])
        pos += f
        if k == len(sizes) // 2 - 1:                         # half-way: end one stream of the first, a middle and the last tile
            for t0 in sorted({0, (tiles // 2) * G, (tiles - 1) * G}):
                b = t0 + int(np.argmax(pos[t0:min(t0 + G, B)]))
                flushed.append(b)
            assert all(pos[b] > 0 for b in flushed)
            for b, rest in zip(flushed, dec.flush(items=flushed)):
                segments[current[b]]['got'].append(rest.cpu().numpy())
                segments[current[b]]['end'] = int(pos[b])
                current[b] = len(segments)
                segments.append(dict(b=b, start=int(pos[b]), got=[]))
            assert all(int(dec.frames[b]) == 0 for b in flushed)
    for b, rest in enumerate(dec.flush()):
        segments[current[b]]['got'].append(rest.cpu().numpy())
    assert len(flushed) == min(3, tiles) and len(set(pos.tolist())) > 1
    for seg in segments:
        seg.setdefault('end', int(pos[seg['b']]))
        seg['fed'] = source[seg['b'], seg['start']:seg['end']]
        seg['got'] = np.concatenate(seg['got'])
    for seg, want in zip(segments, device_whole([seg['fed'] for seg in segments], trans, init)):
        assert np.array_equal(seg['got'], want), (seg['b'], seg['start'], seg['got'], want)
    # the oracle: the first tile, the partial last tile, the tiles of the flushed streams, and 48 streams over the batch
    chosen = set(range(min(G, B))) | set(range((tiles - 1) * G, B)) | set(np.linspace(0, B - 1, 48).astype(int).tolist())
    for b in flushed:
        chosen |= set(range(b // G * G, min(b // G * G + G, B)))
    some = [seg for seg in segments if seg['b'] in chosen and len(seg['fed'])]
    assert len({seg['b'] for seg in some}) >= min(B, 32) and all(any(seg['b'] == b for seg in some) for b in flushed)
    for seg, want in zip(some, oracle_whole([seg['fed'] for seg in some], trans, init)):
        assert np.array_equal(seg['got'], want), (seg['b'], seg['start'], seg['got'], want)


@pytest.mark.parametrize('G,S', [(2, 16), (4, 15), (16, 16)])
def test_tile_neighbour_with_more_frames_leaves_full_windows_alone(G, S):
    """The forward kernel runs a tile for as many frames as its busiest stream has.  For a neighbour with fewer frames the
    slots past its own, pending + t, lie -- once pending + t reaches the capacity -- on the stream's OLDEST pending rows:
    they must not be written.  A matrix that favours staying keeps windows long; the ring is held at its first capacity
    (a stream takes no more frames than it has slots, a full one is flushed and restarts); a stream with 12 or more pending
    rows takes 0 or 1 frames while its tile neighbours take all Tc = 5.  Asserted from pending, frames and the capacity: such
    a push happened, with live rows under the slots the neighbour's frames reach."""
    B = smallest_batch(G, S)
    if B is None:
        pytest.skip(f'no batch gives {G} streams per workgroup on this device')
    B += 3
    assert tile(B, S) == G
    T, Tc, capacity = 120, 5, INITIAL_CAPACITY
    rng = np.random.default_rng(G + S)
    source, trans, init = synth.problem(B, T, S, seed=200 + G)
    trans = trans.copy()
    trans[np.arange(S), np.arange(S)] += np.float32(6.)
    dec = decoder(B, S, trans, init)
    of_tile = np.arange(B) // G
    pos = np.zeros(B, dtype=np.int64)
    segments = [dict(b=b, start=0, got=[]) for b in range(B)]          # one per stream, one more per restart
    current = list(range(B))
    covered, restarts = 0, 0
    for k in range(96):
        pending = dec.pending.numpy()
        full = np.flatnonzero(pending >= capacity).tolist()
        if full:                                             # no slot left: end the sequence, start another
            for b, rest in zip(full, dec.flush(items=full)):
                segments[current[b]]['got'].append(rest.cpu().numpy())
                segments[current[b]]['end'] = int(pos[b])
                current[b] = len(segments)
                segments.append(dict(b=b, start=int(pos[b]), got=[]))
            restarts += len(full)
            pending = dec.pending.numpy()
        room, left = capacity - pending, T - pos
        f = np.minimum(np.minimum(rng.integers(0, Tc + 1, size=B), room), left)
        held = pending >= 12
        f[held] = np.minimum(np.minimum(k % 2, room), left)[held]
        beside = (np.bincount(of_tile[held], minlength=of_tile[-1] + 1) > 0)[of_tile] & ~held
        f[beside & (room >= Tc) & (left >= Tc)] = Tc
        if not f.any() and not left.any():
            break
        busiest = np.zeros(of_tile[-1] + 1, dtype=np.int64)
        np.maximum.at(busiest, of_tile, f)
        covered += int(((f < busiest[of_tile]) & (pending + busiest[of_tile] > capacity)).sum())
        chunk = np.full((B, Tc, S), np.nan, np.float32)
        for t in range(Tc):
            rows = np.flatnonzero(f > t)
            chunk[rows, t] = source[rows, pos[rows] + t]
        out = dec.push(torch.from_numpy(chunk).to(DEV), torch.from_numpy(f))
        assert dec._capacity == capacity
        counts = np.array([o.numel() for o in out])
        pieces = np.split(torch.cat(out).cpu().numpy(), np.cumsum(counts)[:-1])
        for b in range(B):
            segments[current[b]]['got'].append(pieces[b])
        pos += f
    for b, rest in enumerate(dec.flush()):
        segments[current[b]]['got'].append(rest.cpu().numpy())
    print(f'G = {G}, B = {B}: {covered} pushes of a stream with live rows under its neighbour\'s frames, {restarts} restarts')
    assert covered >= 1
    for seg in segments:
        seg.setdefault('end', int(pos[seg['b']]))
        seg['fed'] = source[seg['b'], seg['start']:seg['end']]
        seg['got'] = np.concatenate(seg['got'])
    for seg, want in zip(segments, device_whole([seg['fed'] for seg in segments], trans, init)):
        assert np.array_equal(seg['got'], want), (seg['b'], seg['start'], seg['got'], want)
    chosen = set(np.linspace(0, B - 1, 64).astype(int).tolist())
    some = [seg for seg in segments if seg['b'] in chosen and len(seg['fed'])]
    for seg, want in zip(some, oracle_whole([seg['fed'] for seg in some], trans, init)):
        assert np.array_equal(seg['got'], want), (seg['b'], seg['start'], seg['got'], want)


# ------------------------------------------------------------------------------------------------- D2: ring growth
@pytest.mark.parametrize('S,stay,Tc,rows_wrap', [(16, 6., 5, True), (64, 8., 7, True), (257, 10., 9, False), (257, 10., 5, True)],
                         ids=['S16-rows-move', 'S64-rows-move', 'S257-by-9-pending-and-oracle-only', 'S257-by-5-rows-move'])
def test_ring_grows_with_a_wrapped_window(S, stay, Tc, rows_wrap):
    """A matrix that favours staying keeps dozens of frames pending, long after the window's first slot has moved round the
    ring.  The ring then grows from a window that does not start at slot 0 and, with the push's frames, runs past the last
    slot (asserted from frames, pending and the capacity).  `rows_wrap`: at one growth at least the rows ALREADY in the ring
    wrap as well, so that the copy to the larger ring has to move them to other slots (with 64 states that is the second
    growth, 32 -> 64; the first meets windows that end before slot 16).  With 257 states in pushes of 9 no growth meets such
    a window -- every pending row keeps its slot -- so that case cannot notice a wrong copy: it checks equal `pending` and
    the oracle only, and the pushes of 5 do what it was meant to.  (18, 36, 50 frames pending at the most with 16, 64, 257
    states.)  The host decoder runs alongside (equal `pending` after every push)."""
    B, T = 4, 400
    obs, trans, init = synth.problem(B, T, S, seed=S)
    trans = trans.copy()
    trans[np.arange(S), np.arange(S)] += np.float32(stay)
    dec, twin = decoder(B, S, trans, init), decoder(B, S, trans, init, gpu=None)
    got = [[] for _ in range(B)]
    growths, window_wraps, rows_wrapped, most = [], 0, 0, 0
    for t in range(0, T, Tc):
        capacity = dec._capacity
        first = ((dec.frames - dec.pending) % capacity).numpy()
        pending = dec.pending.numpy()
        chunk = torch.from_numpy(obs[:, t:t + Tc])
        out = dec.push(chunk.to(DEV))
        twin.push(chunk)
        assert torch.equal(dec.pending, twin.pending), (t, dec.pending, twin.pending)
        if dec._capacity > capacity:
            growths.append((capacity, dec._capacity))
            window_wraps += bool(((first != 0) & (first + pending + chunk.shape[1] > capacity)).any())
            rows_wrapped += bool(((first != 0) & (first + pending > capacity)).any())
        most = max(most, int(dec.pending.max()))
        for b in range(B):
            got[b].append(out[b].cpu())
    for b, rest in enumerate(dec.flush()):
        got[b].append(rest.cpu())
    print(f'S = {S}, pushes of {Tc}: growths {growths}, window wrapped at {window_wraps}, rows in the ring at {rows_wrapped}, '
          f'most pending {most}')
    assert growths[0] == (INITIAL_CAPACITY, 2 * INITIAL_CAPACITY) and window_wraps >= 1
    assert S == 16 or growths[1] == (2 * INITIAL_CAPACITY, 4 * INITIAL_CAPACITY)
    assert rows_wrapped >= 1 or not rows_wrap
    whole = [obs[b] for b in range(B)]
    for b, (want, other) in enumerate(zip(oracle_whole(whole, trans, init), device_whole(whole, trans, init))):
        assert np.array_equal(torch.cat(got[b]).numpy(), want), b
        assert np.array_equal(want, other), b


# -------------------------------------------------------------------------------------------------------- D3: ties
TIE_STATES = [63, 64, 65, 128, 257, 1440]


def lane_pairs(S):
    """Index pairs (i1, i2), i1 < i2 < S: two lanes of one wave whose shuffle must keep the smaller index, and -- from 65
    states -- pairs whose FIRST index sits in the higher lane (i1 % 64 > i2 % 64)."""
    pairs = [(1, 2), (5, 37), (30, 62)]
    if S > 64:
        last = 64 * ((S - 1) // 64)
        pairs += [(63, 64), (last - 1, last), (63, last), (62, 64)]
        assert all(a % 64 > b % 64 for a, b in pairs[3:])
    assert all(a < b < S for a, b in pairs)
    return pairs


def assert_first_maximum_in_a_higher_lane(seq, trans, init):
    """The input forces the tie rule across lanes: some backpointer scan has maxima i1 < i2 with i1 % 64 > i2 % 64."""
    post, _ = reference_arrays(seq, trans, init)
    for t in range(1, len(seq)):
        cand = post[t - 1][None, :] + trans
        top = cand == cand.max(axis=1, keepdims=True)
        for j in np.flatnonzero(top.sum(axis=1) >= 2)[:64]:
            where = np.flatnonzero(top[j])
            if (where[0] % 64 > where[1:] % 64).any():
                return
    raise AssertionError('no scan of this input has its first maximum in a higher lane than a later one')


@pytest.mark.parametrize('S', TIE_STATES)
@pytest.mark.parametrize('mode', ['one', 'ragged'])
def test_ties_all_zero(S, mode):
    B, T = 3, 20 if S < 1440 else 12
    zeros = np.zeros((T, S), np.float32)
    got, _ = check_streams([zeros] * B, np.zeros((S, S), np.float32), np.zeros(S, np.float32), plan(B, T, mode))
    assert all((g == 0).all() for g in got)


@pytest.mark.parametrize('S', TIE_STATES)
@pytest.mark.parametrize('mode', ['one', 'ragged'])
@pytest.mark.parametrize('levels', [7, 4])
def test_ties_quantised_scores(S, mode, levels):
    """Scores on 7 levels (0, -0.5 .. -3, as in the host test) and on 4 (0 .. -3): every scan meets many equal maxima."""
    B, T = 3, 20 if S < 1440 else 12
    step = 2 if levels == 7 else 1
    rng = np.random.default_rng(3 + S)
    obs = np.round(rng.uniform(-3, 0, size=(B, T, S)) * step).astype(np.float32) / step
    trans = np.round(rng.uniform(-3, 0, size=(S, S)) * step).astype(np.float32) / step
    init = np.zeros(S, np.float32)
    if S > 64:
        assert_first_maximum_in_a_higher_lane(clamp(obs[0]), trans, init)
    check_streams([obs[b] for b in range(B)], trans, init, plan(B, T, mode, seed=4))


@pytest.mark.parametrize('S', TIE_STATES)
@pytest.mark.parametrize('mode', ['one', 'ragged'])
def test_ties_only_two_maxima(S, mode):
    """Frame t scores two states 0 and the rest -1, the matrix is flat: every backpointer scan of frame t + 1, and the final
    state of a flush after frame t, has exactly those two maxima and must name the first.  The pairs are `lane_pairs`."""
    B, T = 3, 21
    pairs = lane_pairs(S)
    obs = np.full((B, T, S), -1, np.float32)
    want = np.zeros((B, T), np.int32)
    for b in range(B):
        for t in range(T):
            i1, i2 = pairs[(t + b) % len(pairs)]
            obs[b, t, [i1, i2]] = 0
            want[b, t] = i1
    trans, init = np.zeros((S, S), np.float32), np.zeros(S, np.float32)
    post, _ = reference_arrays(clamp(obs[0]), trans, init)
    assert all(np.flatnonzero(post[t] == post[t].max()).tolist() == list(pairs[t % len(pairs)]) for t in range(T))
    got, pos = check_streams([obs[b] for b in range(B)], trans, init, plan(B, T, mode, seed=S))
    for b in range(B):
        assert np.array_equal(got[b], want[b, :pos[b]]), (b, got[b], want[b])
    # the final state of a flush after every frame
    dec = decoder(B, S, trans, init)
    for t in range(len(pairs)):
        dec.push(torch.from_numpy(obs[:, t:t + 1]).to(DEV))
        rest = dec.flush()
        assert [r.tolist() for r in rest] == [[int(want[b, t])] for b in range(B)]


# ---------------------------------------------------------------------------------------------- D4: maximal commit
@pytest.mark.parametrize('S', [1, 2, 3, 17, 64, 65, 257])
@pytest.mark.parametrize('mode', ['one', 'ragged'])
@pytest.mark.parametrize('scores', ['dense', 'quantised'])
def test_maximal_commit(S, mode, scores):
    """After every push `pending` is what the brute-force survivor sets of the numpy recurrence leave, with a dense matrix
    and a narrow band; quantised scores keep the sets large, so that walks end on the memo shortcut."""
    B, T = 3, 40
    obs, trans, init = synth.problem(B, T, S, seed=30 + S)
    if scores == 'quantised':
        rng = np.random.default_rng(S)
        obs = np.round(rng.uniform(-2, 0, size=(B, T, S))).astype(np.float32)
        trans = np.round(rng.uniform(-2, 0, size=(S, S))).astype(np.float32)
    source = [obs[b] for b in range(B)]
    band = synth.banded_transition(S, 3) if S > 3 else trans
    for matrix in (trans, band):
        check_streams(source, matrix, init, plan(B, T, mode, seed=S), check=commit_checker(source, matrix, init, prepare=clamp))


@pytest.mark.parametrize('S', [2, 17, 257])
def test_uniform_transition_leaves_one_pending(S):
    B, T = 3, 20
    obs, _, _ = synth.problem(B, T, S, seed=40)
    dec = torbi_amd.StreamDecoder(B, S, log_probs=True, gpu=0)
    for t in range(T):
        dec.push(torch.from_numpy(obs[:, t:t + 1]).to(DEV))
        assert dec.pending.tolist() == [1] * B


# ------------------------------------------------------------------------------------------------------- D5: edges
@pytest.mark.parametrize('S,B', [(1, 5), (2, 17), (3, 1), (4, 5), (5, 17), (255, 1), (256, 5), (257, 17)])
@pytest.mark.parametrize('mode', ['one', 'ragged'])
def test_state_count_edges(S, B, mode):
    T = 20
    obs, trans, init = synth.problem(B, T, S, seed=70 + S)
    source = [obs[b] for b in range(B)]
    check_streams(source, trans, init, plan(B, T, mode, seed=S), check=commit_checker(source, trans, init, prepare=clamp))


@pytest.mark.parametrize('S', [7999, 8000])
def test_largest_state_counts(S):
    """The documented bound: 2 * 8000 words of dynamic LDS in the forward kernel (J = 4 at 8000, 1 at 7999) and the walk."""
    B, T = 2, 5
    obs, trans, init = synth.problem(B, T, S, seed=S)
    dec = decoder(B, S, trans, init)
    pushes = [(3, np.array([2, 3])), (3, np.array([3, 2]))]
    got, pos = feed(dec, [obs[b] for b in range(B)], pushes, device=DEV)
    assert pos.tolist() == [T, T]
    for b, want in enumerate(oracle_whole([obs[b] for b in range(B)], trans, init)):
        assert np.array_equal(got[b], want), (b, got[b], want)


def test_too_many_states_raise_and_leave_the_device_usable():
    S = 8001
    assert tile(1, S) == -3
    dec = torbi_amd.StreamDecoder(1, S, log_probs=True, gpu=0)
    with pytest.raises(_lib.TorbiHipError):
        dec.push(torch.zeros(1, 1, S, device=DEV))
    with pytest.raises(_lib.TorbiHipError):
        dec.flush()
    obs, trans, init = synth.problem(2, 6, 5, seed=1)
    check_streams([obs[0], obs[1]], trans, init, plan(2, 6, 'one'))


def test_pushes_without_frames():
    """A push of Tc = 0 and a push whose every stream gets 0 frames return nothing and change nothing."""
    B, T, S = 5, 12, 65
    obs, trans, init = synth.problem(B, T, S, seed=80)
    dec = decoder(B, S, trans, init)
    got = [[] for _ in range(B)]

    def nothing():
        for out in (dec.push(torch.empty(B, 0, S, device=DEV)),
                    dec.push(torch.full((B, 3, S), math.nan, device=DEV), torch.zeros(B, dtype=torch.int64))):
            assert len(out) == B and all(o.numel() == 0 and o.dtype == torch.int32 for o in out)
    nothing()                                                # on fresh streams
    assert dec.frames.tolist() == [0] * B
    for t in range(0, T, 4):
        for b, o in enumerate(dec.push(torch.from_numpy(obs[:, t:t + 4]).to(DEV))):
            got[b].append(o.cpu())
        before = (dec.frames.clone(), dec.pending.clone())
        nothing()
        assert torch.equal(dec.frames, before[0]) and torch.equal(dec.pending, before[1])
    for b, rest in enumerate(dec.flush()):
        got[b].append(rest.cpu())
    whole = [obs[b] for b in range(B)]
    for b, (want, other) in enumerate(zip(oracle_whole(whole, trans, init), device_whole(whole, trans, init))):
        assert np.array_equal(torch.cat(got[b]).numpy(), want) and np.array_equal(want, other), b


@pytest.mark.parametrize('S', [1, 3, 64, 130])
def test_single_frame_then_flush(S):
    """One frame and a flush: the first NaN of obs[0] + initial, otherwise its first maximum (at 130 states the first sits in
    a higher lane than the second); a second flush is empty."""
    B = 4
    obs, trans, init = synth.problem(B, 1, S, seed=90 + S)
    obs, init = obs.copy(), init.copy()
    if S > 1:
        nans, tied = ((70, 128), (100, 128)) if S == 130 else ((S // 2, S - 1), (S - 2, S - 1))
        obs[1, 0, list(nans)] = np.nan                       # two NaN: the first one
        obs[2, 0] = -3.
        obs[2, 0, list(tied)] = 0.                           # two maxima: the first one
        init[list(tied)] = init.max() + 1
        obs[3, 0] = np.nan                                   # a row of NaN: state 0
    row = clamp(obs[:, 0]) + init[None, :]
    want = [int(np.isnan(r).argmax()) if np.isnan(r).any() else int(r.argmax()) for r in row]
    if S > 1:
        assert want[1:] == [nans[0], tied[0], 0] and (row[2] == row[2].max()).sum() == 2
    dec = decoder(B, S, trans, init)
    out = dec.push(torch.from_numpy(obs).to(DEV))
    assert dec.flush(items=[]) == []
    if S == 1:                                               # one state: the push has returned its frame already
        assert [o.tolist() for o in out] == [[0]] * B
    else:
        assert all(o.numel() == 0 for o in out) and dec.pending.tolist() == [1] * B
        assert [r.tolist() for r in dec.flush()] == [[w] for w in want]
        for b, other in enumerate(oracle_whole([obs[b] for b in range(B)], trans, init)):
            assert other.tolist() == [want[b]], b
    assert all(r.numel() == 0 for r in dec.flush())          # flushed (twice): nothing left
    assert dec.frames.tolist() == [0] * B and dec.pending.tolist() == [0] * B


# -------------------------------------------------------------------------------------------------------- D6: C ABI
SENTINEL = -7


def abi_call(lib, name, *args):
    torch.cuda.synchronize()
    code = getattr(lib, name)(*args)
    torch.cuda.synchronize()
    assert code == 0, (name, code)


@pytest.mark.parametrize('S', [8, 7])
@pytest.mark.parametrize('violation', ['capacity', 'out_capacity', 'base_slot'])
def test_c_abi_leaves_a_stream_whose_info_does_not_fit(S, violation):
    """torbi_hip_stream_push / _flush called directly: counts_out = -1 for the stream whose info does not fit, its ring,
    memo and indices_out row byte for byte as they were, the other streams decoded.  (Only violations that stay inside the
    buffers whatever the kernels do with them: pending + frames above capacity or out_capacity, base_slot == capacity.)"""
    lib = _lib.load()
    B, Tc, bad = 3, 2, 1
    cap, out_cap = {'capacity': (4, 8), 'out_capacity': (8, 3), 'base_slot': (8, 8)}[violation]
    wrong = {'capacity': [3, 1, 2, 0], 'out_capacity': [2, 5, 2, 0], 'base_slot': [1, cap, 1, 0]}[violation]
    obs, trans, init = synth.problem(B, Tc, S, seed=S)
    nbytes = lib.torbi_hip_stream_state_bytes(B, S, cap)
    assert nbytes == 4 * (B * cap * S + B * cap + B * S)
    rng = np.random.default_rng(S)
    state = torch.from_numpy(rng.integers(1, 1 << 20, size=nbytes // 4).astype(np.int32)).to(DEV)     # small positive floats
    ring = state[:B * cap * S].view(B, cap, S)
    memo = state[B * cap * S:B * cap * (S + 1)].view(B, cap)
    out = torch.full((B, out_cap), SENTINEL, dtype=torch.int32, device=DEV)
    counts = torch.full((B,), SENTINEL, dtype=torch.int32, device=DEV)
    info = np.array([[0, 0, Tc, 1], wrong, [0, 0, Tc, 1]], np.int32)
    d_obs, d_trans, d_init = (torch.from_numpy(x).to(DEV) for x in (obs, trans, init))
    d_tt = d_trans.t().contiguous()
    d_info = torch.from_numpy(info).to(DEV)
    before = (ring[bad].clone(), memo[bad].clone())
    null = ctypes.c_void_p(0)
    abi_call(lib, 'torbi_hip_stream_push', d_obs.data_ptr(), Tc, d_info.data_ptr(), d_trans.data_ptr(),
             d_tt.data_ptr(), d_init.data_ptr(), state.data_ptr(), nbytes, cap, out.data_ptr(), out_cap, counts.data_ptr(),
             B, S, 0, null)
    got = counts.cpu().numpy()
    assert got[bad] == -1
    assert torch.equal(ring[bad], before[0]) and torch.equal(memo[bad], before[1]) and (out[bad] == SENTINEL).all()
    paths = {}
    for b in (0, 2):                                         # the other streams: the frames the brute-force rule decides
        _, bp = reference_arrays(obs[b], trans, init)
        paths[b] = reference_path(obs[b], trans, init)
        assert got[b] == decided(bp, Tc, S) + 1, (b, got)
        assert out[b, :got[b]].cpu().tolist() == paths[b][:got[b]].tolist() and (out[b, got[b]:] == SENTINEL).all()
    # flush: the two good streams return the rest; the third claims more pending frames than the ring has slots
    info = np.array([[Tc - got[0], got[0] % cap, 1, 0], [cap + 1, 0, 1, 0], [Tc - got[2], got[2] % cap, 1, 0]], np.int32)
    rest = torch.full((B, cap + 1), SENTINEL, dtype=torch.int32, device=DEV)
    counts.fill_(SENTINEL)
    d_info = torch.from_numpy(info).to(DEV)
    abi_call(lib, 'torbi_hip_stream_flush', d_info.data_ptr(), d_trans.data_ptr(), state.data_ptr(),
             nbytes, cap, rest.data_ptr(), cap + 1, counts.data_ptr(), B, S, 0, null)
    more = counts.cpu().numpy()
    assert more[bad] == -1
    assert torch.equal(ring[bad], before[0]) and torch.equal(memo[bad], before[1]) and (rest[bad] == SENTINEL).all()
    for b in (0, 2):
        assert more[b] == Tc - got[b]
        assert out[b, :got[b]].cpu().tolist() + rest[b, :more[b]].cpu().tolist() == paths[b].tolist()
    want = oracle.decode(obs, np.full(B, Tc, np.int32), trans, init)
    assert all(np.array_equal(paths[b], want[b]) for b in (0, 2))
