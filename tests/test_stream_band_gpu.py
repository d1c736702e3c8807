"""The band route of torbi_amd.StreamDecoder on the device (csrc/stream_band.hpp): every decoder here is built with
route='band' and says so, unless a test is about routing.  Outputs are compared with the device's whole-sequence decode
(other kernels), the numpy recurrence of tests/stream_cases.py on the values the decoder sees (the epsilon round trip by
torch ops on the device) and a route='dense' decoder fed the same pushes, after every push."""
import ctypes
import math
from unittest import mock

import numpy as np
import pytest
import torch

import torbi_amd
from torbi_amd import _lib, synth, viterbi
from torbi_amd.stream import INITIAL_CAPACITY
from stream_cases import plan, reference_arrays, reference_path, decided, commit_checker
from stream_lag_cases import feed_bounded, identity
from stream_band_cases import (BACKGROUNDS, REACHES, band_matrix, continuous, dead_initial, diagonals, grid_scores,
                               nonfinite_sources, tie_background, tie_counts, tie_problem)

pytestmark = pytest.mark.gpu

DEV = torch.device('cuda:0')
INSTANCES = (1, 2, 4)                    # stream_band_forward_kernel<G> as built (stream_band::kMaxGroup)


def clamp(obs):
    """log(exp(x) + tiny) by torch ops on the device."""
    x = torch.from_numpy(np.ascontiguousarray(obs, dtype=np.float32)).to(DEV)
    torch.exp_(x)
    x += torch.finfo(torch.float32).tiny
    torch.log_(x)
    return x.cpu().numpy()


def decoder(B, S, trans, init, route='band', max_lag=None, gpu=0, stated=None):
    """`stated` = (reach_left, reach_right, background): the band the decoder is told instead of what `viterbi.band_over`
    reads off the matrix.  That look takes a finite background only from a matrix whose in-band entries all lie above it
    (else it answers a band of full width), so a tie input whose in-band scores reach down to the background needs its band
    stated to meet the prefix and the suffix at all; the promise is kept, and the device's verdict is still asked."""
    where = DEV if gpu is not None else 'cpu'
    matrix = None if trans is None else torch.from_numpy(trans).to(where)
    look = viterbi.band_over if stated is None else (lambda *a, **k: tuple(stated))
    with mock.patch.object(viterbi, 'band_over', look):
        dec = torbi_amd.StreamDecoder(B, S, matrix, None if init is None else torch.from_numpy(init).to(where), log_probs=True,
                                      gpu=gpu, max_lag=max_lag, route=route)
        if gpu is not None:
            assert dec.route == route
            if route == 'band':
                assert torbi_amd.stream_route(matrix, B, S, gpu=0, log_probs=True) == 'band'
                assert stated is None or dec._band[:3] == tuple(stated)
    return dec


def band_tile(B, S, left, right):
    return _lib.load().torbi_hip_stream_band_tile(B, S, left, right, 0)


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


def feed_both(dec, other, source, pushes, check=None):
    """Push `source[b]` (frames, S) piece by piece (NaN where nothing may be read) to `dec` and, where given, to `other`,
    whose outputs, `pending` and `forced` must equal `dec`'s after every push and after the flush.  Returns the
    concatenated outputs and the frames pushed."""
    B, S = len(source), dec.states
    pos = np.zeros(B, dtype=np.int64)
    got = [[] for _ in range(B)]
    for k, (Tc, f) in enumerate(pushes):
        chunk = np.full((B, Tc, S), np.nan, np.float32)
        for b in range(B):
            chunk[b, :f[b]] = source[b][pos[b]:pos[b] + f[b]]
        chunk, counts = torch.from_numpy(chunk).to(DEV), torch.from_numpy(np.asarray(f))
        out = [o.cpu() for o in dec.push(chunk, counts)]
        if other is not None:
            twin = [o.cpu() for o in other.push(chunk if other.gpu is not None else chunk.cpu(), counts)]
            assert all(torch.equal(a, o) for a, o in zip(out, twin)), (k, out, twin)
            assert torch.equal(dec.pending, other.pending) and torch.equal(dec.forced, other.forced), k
        for b in range(B):
            got[b].append(out[b])
        pos += f
        if check is not None:
            check(dec, pos)
    rest = [r.cpu() for r in dec.flush()]
    if other is not None:
        assert all(torch.equal(a, o.cpu()) for a, o in zip(rest, other.flush()))
    for b in range(B):
        got[b].append(rest[b])
    assert (dec.frames == 0).all() and (dec.pending == 0).all()
    return [torch.cat(g).numpy() for g in got], pos


def check_streams(source, trans, init, pushes, reach=None, check=None, numpy_reference=True, dense=True, stated=None):
    """`source` through a band decoder (and a dense one beside it); every stream against the device's whole-sequence decode
    and the numpy recurrence.  `reach`: what the decoder must have found; `stated`: see `decoder`."""
    B, S = len(source), source[0].shape[1]
    dec = decoder(B, S, trans, init, stated=stated)
    if reach is not None:
        assert dec._band[:2] == tuple(reach), (dec._band[:2], reach)
    got, pos = feed_both(dec, decoder(B, S, trans, init, route='dense') if dense else None, source, pushes, check=check)
    fed = [source[b][:pos[b]] for b in range(B)]
    for b, want in enumerate(device_whole(fed, trans, init)):
        assert np.array_equal(got[b], want), ('device', b, got[b], want)
    if numpy_reference:
        with np.errstate(invalid='ignore'):
            for b in range(B):
                if pos[b]:
                    path = reference_path(clamp(fed[b]), trans, init)
                    assert np.array_equal(got[b], path), ('numpy', b, got[b], path)
    return got, pos


# ------------------------------------------------------------------------------- 1: exactness and maximal commit
SHAPES = [(1, 'one'), (5, 'ragged'), (17, 'all'), (1, 'ragged'), (5, 'all'), (17, 'one'), (1, 'all'), (5, 'one'), (17, 'ragged')]


@pytest.mark.parametrize('background', list(BACKGROUNDS))
@pytest.mark.parametrize('S', [64, 68, 252, 256, 260])
def test_band_route_is_exact_and_commits_all_it_can(S, background):
    """One wave of states, and the edge of one state per thread (252, 256, 260) x every reach x the three backgrounds; the
    batch sizes 1, 5, 17 and the push plans 'one', 'ragged', 'all' rotate over the reaches and with S, so that every pair of
    them meets every reach.  After every push `pending` is what the brute-force survivor sets leave."""
    T = 40
    bg = BACKGROUNDS[background]
    order = [64, 68, 252, 256, 260].index(S) + 3 * list(BACKGROUNDS).index(background)
    for k, (left, right) in enumerate(REACHES):
        B, mode = SHAPES[(k + order) % len(SHAPES)]
        trans = band_matrix(S, left, right, bg, seed=S + k)
        init = synth.problem(1, 1, S, seed=k)[2]
        obs = continuous(B, T, S, seed=S + 10 * k)
        source = [obs[b] for b in range(B)]
        check_streams(source, trans, init, plan(B, T, mode, seed=k), reach=(left, right),
                      check=commit_checker(source, trans, init, prepare=clamp))


# ------------------------------------------------------------------------------------------- 2: every <G> instance
def smallest_batch(G, S, left, right):
    lo, hi = 1, 1 << 16
    if band_tile(hi, S, left, right) < G:
        return None
    while lo < hi:
        mid = (lo + hi) // 2
        if band_tile(mid, S, left, right) >= G:
            hi = mid
        else:
            lo = mid + 1
    return lo if band_tile(lo, S, left, right) == G else None


def run_tiles(G, S, left, right, T):
    """Ragged pushes at a batch that runs G streams per workgroup with a partial last tile; in every push every tile has a
    stream with 0 frames and one with all Tc.  Returns the G the push ran (torbi_hip_stream_band_tile)."""
    B = smallest_batch(G, S, left, right)
    assert B is not None, f'no batch gives {G} streams per workgroup at {S} states on this device'
    B += 3
    while G > 1 and B % G == 0:
        B += 1
    ran = band_tile(B, S, left, right)
    assert ran == G and (G == 1 or B % G != 0), (B, ran)
    print(f'stream_band_forward_kernel<{G}>: B = {B}, S = {S}, reach {left}/{right}')
    rng = np.random.default_rng(100 * G + S)
    trans = band_matrix(S, left, right, BACKGROUNDS['log_tiny'], seed=G)
    init = synth.problem(1, 1, S, seed=G)[2]
    source = continuous(B, T, S, seed=G + S)
    dec = decoder(B, S, trans, init)
    assert dec._band[:2] == (left, right)
    tiles = (B + G - 1) // G
    pos = np.zeros(B, dtype=np.int64)
    got = [[] for _ in range(B)]
    sizes = []
    while sum(sizes) < T:
        sizes.append(min(int(rng.integers(1, 5)), T - sum(sizes)))
    for k, Tc in enumerate(sizes):
        f = rng.integers(0, Tc + 1, size=B)
        if G > 1:
            first = np.arange(tiles) * G
            members = np.minimum(G, B - first)
            wide = members >= 2
            f[(first + k % members)[wide]] = 0
            f[(first + (k + 1) % members)[wide]] = Tc
            for t0, n in zip(first[wide], members[wide]):
                assert f[t0:t0 + n].min() == 0 and f[t0:t0 + n].max() == Tc
        assert (pos + f <= T).all()                           # (the pushes add up to T frames: no stream runs out)
        chunk = np.full((B, Tc, S), np.nan, np.float32)
        for t in range(Tc):
            rows = np.flatnonzero(f > t)
            chunk[rows, t] = source[rows, pos[rows] + t]
        out = dec.push(torch.from_numpy(chunk).to(DEV), torch.from_numpy(f))
        counts = np.array([o.numel() for o in out])
        pieces = np.split(torch.cat(out).cpu().numpy(), np.cumsum(counts)[:-1])
        for b in range(B):
            got[b].append(pieces[b])
        pos += f
    for b, rest in enumerate(dec.flush()):
        got[b].append(rest.cpu().numpy())
    assert len(set(pos.tolist())) > 1
    fed = [source[b, :pos[b]] for b in range(B)]
    for b, want in enumerate(device_whole(fed, trans, init)):
        assert np.array_equal(np.concatenate(got[b]), want), (b, np.concatenate(got[b]), want)
    for b in sorted(set(range(min(G, B))) | set(range((tiles - 1) * G, B)) | set(np.linspace(0, B - 1, 8).astype(int).tolist())):
        if pos[b]:
            assert np.array_equal(np.concatenate(got[b]), reference_path(clamp(fed[b]), trans, init)), b
    return ran


def test_every_forward_instance_runs_with_partial_tiles_and_uneven_pushes():
    seen = {run_tiles(G, 64, 2, 5, T=14) for G in INSTANCES}
    assert seen == set(INSTANCES)


@pytest.mark.parametrize('G', [2, 4])
def test_instances_whose_rows_and_scans_pass_64_kb_of_lds(G):
    """1440 states: 72 KB of LDS at two streams per workgroup, 144 KB at four."""
    assert run_tiles(G, 1440, 11, 11, T=5) == G


# ------------------------------------------------------------------------------------------------------- 3: ties
@pytest.mark.parametrize('S', [64, 260])
@pytest.mark.parametrize('mode', ['one', 'ragged'])
def test_ties_all_zero(S, mode):
    B, T = 3, 20
    zeros = np.zeros((T, S), np.float32)
    for stated in ((2, 5, 0.), (0, 0, 0.), (31, 31, 0.)):
        got, _ = check_streams([zeros] * B, np.zeros((S, S), np.float32), np.zeros(S, np.float32), plan(B, T, mode), stated=stated)
        assert all((g == 0).all() for g in got)


@pytest.mark.parametrize('S', [64, 260])
@pytest.mark.parametrize('levels', [4, 7])
def test_ties_on_a_grid(S, levels):
    """Observations on 4 and 7 levels of the -0.25 grid, in-band scores on 8, beside every background."""
    B, T = 3, 20
    obs = grid_scores(B, T, S, levels, seed=S + levels)
    for k, (left, right) in enumerate([(2, 2), (0, 3), (5, 2), (31, 31)]):
        for name, bg in BACKGROUNDS.items():
            trans = band_matrix(S, left, right, bg, seed=k, grid=8)
            check_streams([obs[b] for b in range(B)], trans, np.zeros(S, np.float32), plan(B, T, ('one', 'ragged')[k % 2], seed=k),
                          dense=name == 'minus_inf')


@pytest.mark.parametrize('reach', [(2, 2), (0, 3), (3, 0), (2, 5), (5, 2), (31, 31)], ids=lambda r: f'{r[0]}-{r[1]}')
def test_ties_between_the_band_and_what_lies_outside_it(reach):
    """tests/test_stream_band_cpu.py's inputs: a candidate left of the band equals the in-band best and must win, the in-band
    best equals a candidate right of the band and must win (counted on the values the decoder sees)."""
    left, right = reach
    obs, trans, init = tie_problem(64, left, right, seed=7 + left)
    prefix_wins, band_wins = tie_counts(clamp(obs), trans, init, left, right, reference_arrays)
    assert prefix_wins > 0 and band_wins > 0
    check_streams([obs, obs[::-1].copy()], trans, init, plan(2, len(obs), 'ragged', seed=left),
                  stated=(left, right, float(tie_background(left, right))))


def scan_pairs(S):
    """Index pairs (i1, i2), i1 < i2 < S, that the scans join in every way: within a thread's run of states, across lanes,
    and across waves with the first index in the higher lane (a thread owns ceil(S / 256) consecutive states)."""
    pairs = [(1, 2), (5, 37), (30, 62), (0, S - 1)]
    if S > 256:
        run = (S + 255) // 256
        pairs += [(64 * run - 1, 64 * run), (63 * run, 128 * run), (128 * run - 1, 128 * run + run), (2, 3)]
    return pairs


@pytest.mark.parametrize('S', [64, 260])
@pytest.mark.parametrize('mode', ['one', 'ragged'])
def test_ties_only_two_maxima(S, mode):
    """Frame t scores two states 0 and the rest -1 under a flat matrix (stated as a band of the diagonal with background 0:
    the scans find both maxima): every state's maximum at frame t + 1, and the final state of a flush after frame t, has
    exactly those two and names the first."""
    B, T = 3, 21
    pairs = scan_pairs(S)
    assert all(a < b < S for a, b in pairs)
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
    got, pos = check_streams([obs[b] for b in range(B)], trans, init, plan(B, T, mode, seed=S), stated=(0, 0, 0.))
    for b in range(B):
        assert np.array_equal(got[b], want[b, :pos[b]]), (b, got[b], want[b])
    dec = decoder(B, S, trans, init, stated=(0, 0, 0.))
    for t in range(len(pairs)):
        dec.push(torch.from_numpy(obs[:, t:t + 1]).to(DEV))
        assert [r.tolist() for r in dec.flush()] == [[int(want[b, t])] for b in range(B)]


# ---------------------------------------------------------------------------------------------- 4: non-finite inputs
@pytest.mark.parametrize('background', ['minus_inf', 'log_tiny'])
@pytest.mark.parametrize('reach', [(2, 2), (2, 5)], ids=lambda r: f'{r[0]}-{r[1]}')
def test_nan_and_infinities(reach, background):
    """NaN at state 0 and elsewhere, +inf observations (NaN candidates beside a -inf background), rows of the round trip's
    floor; three streams flushed half-way restart from `initial` beside carried neighbours."""
    left, right = reach
    S, T = 64, 24
    trans = band_matrix(S, left, right, BACKGROUNDS[background], seed=left)
    init = synth.problem(1, 1, S, seed=1)[2]
    source = nonfinite_sources(T, S, seed=right)
    B = len(source)
    with np.errstate(invalid='ignore'):
        check_streams(source, trans, init, plan(B, T, 'ragged', seed=3), reach=reach)
        dec, other = decoder(B, S, trans, init), decoder(B, S, trans, init, route='dense')
        half, flushed = T // 2, [0, 2, 5]
        first, second = [], []
        for into, lo in ((first, 0), (second, half)):
            for t in range(lo, lo + half, 3):
                chunk = torch.from_numpy(np.stack(source)[:, t:t + 3]).to(DEV)
                out, twin = dec.push(chunk), other.push(chunk)
                assert all(torch.equal(a, o) for a, o in zip(out, twin)) and torch.equal(dec.pending, other.pending)
                into.append([o.cpu().numpy() for o in out])
            if lo == 0:
                rest = [r.cpu().numpy() for r in dec.flush(items=flushed)]
                assert all(np.array_equal(a, o.cpu().numpy()) for a, o in zip(rest, other.flush(items=flushed)))
                assert dec.frames.tolist() == [0 if b in flushed else half for b in range(B)]
        tail = [r.cpu().numpy() for r in dec.flush()]
        for b in range(B):
            head = np.concatenate([p[b] for p in first] + ([rest[flushed.index(b)]] if b in flushed else []))
            after = np.concatenate([p[b] for p in second] + [tail[b]])
            if b in flushed:
                assert np.array_equal(head, reference_path(clamp(source[b][:half]), trans, init)), b
                assert np.array_equal(after, reference_path(clamp(source[b][half:]), trans, init)), b
            else:
                assert np.array_equal(np.concatenate([head, after]), reference_path(clamp(source[b]), trans, init)), b


@pytest.mark.parametrize('background', ['minus_inf', 'log_tiny'])
@pytest.mark.parametrize('plus_inf_at', [None, 0, 5])
def test_rows_of_minus_infinity(plus_inf_at, background):
    """An initial vector of -inf: every row is -inf and every candidate ties there; with a first observation of +inf at one
    state the row is -inf with one +inf, a NaN candidate of every state whose band misses it beside a -inf background (at
    state 0: c_0 = NaN, value NaN, pointer 0)."""
    S, T, B = 64, 12, 3
    trans = band_matrix(S, 2, 5, BACKGROUNDS[background], seed=4)
    init = dead_initial(S, plus_inf_at)
    obs = continuous(B, T, S, seed=8)
    if plus_inf_at is not None:
        obs[:, 0, plus_inf_at] = np.inf
    with np.errstate(invalid='ignore'):
        post, _ = reference_arrays(clamp(obs[0]), trans, init)
        assert np.isneginf(np.delete(post[0], [] if plus_inf_at is None else [plus_inf_at])).all()
        check_streams([obs[b] for b in range(B)], trans, init, plan(B, T, 'ragged', seed=5), reach=(2, 5))


# ----------------------------------------------------------------------------------------------- 5: ring growth
def test_pointer_ring_grows_with_a_wrapped_window():
    """A matrix that favours staying keeps dozens of frames pending: the ring grows 16 -> 32 -> 64 -> ... from windows that
    do not start at slot 0 and run past the last slot, at one growth with pointer rows ALREADY in the ring wrapped (they move
    to other slots).  The host decoder runs alongside; `_state_bytes` is the formula at every capacity."""
    B, T, S, Tc = 4, 300, 64, 5
    trans = band_matrix(S, 31, 31, -20., seed=5)
    trans[np.arange(S), np.arange(S)] += np.float32(8.)
    init = np.zeros(S, np.float32)
    obs = continuous(B, T, S, seed=9)
    dec, twin = decoder(B, S, trans, init), decoder(B, S, trans, init, gpu=None)
    got = [[] for _ in range(B)]
    growths, window_wraps, rows_wrapped = [], 0, 0
    for t in range(0, T, Tc):
        capacity = dec._capacity
        assert dec._state_bytes == 4 * (B * capacity * S + B * capacity + B * S)
        first = ((dec.frames - dec.pending) % capacity).numpy()
        pending = dec.pending.numpy()
        chunk = torch.from_numpy(obs[:, t:t + Tc])
        out = dec.push(chunk.to(DEV))
        other = twin.push(chunk)
        assert all(torch.equal(a.cpu(), o) for a, o in zip(out, other)) and torch.equal(dec.pending, twin.pending), t
        if dec._capacity > capacity:
            growths.append((capacity, dec._capacity))
            window_wraps += bool(((first != 0) & (first + pending + Tc > capacity)).any())
            rows_wrapped += bool(((first != 0) & (first + pending > capacity)).any())
        for b in range(B):
            got[b].append(out[b].cpu())
    for b, rest in enumerate(dec.flush()):
        got[b].append(rest.cpu())
    print(f'growths {growths}, window wrapped at {window_wraps}, rows in the ring at {rows_wrapped}')
    assert growths[:2] == [(INITIAL_CAPACITY, 2 * INITIAL_CAPACITY), (2 * INITIAL_CAPACITY, 4 * INITIAL_CAPACITY)]
    assert window_wraps >= 2 and rows_wrapped >= 1
    for b, want in enumerate(device_whole([obs[b] for b in range(B)], trans, init)):
        assert np.array_equal(torch.cat(got[b]).numpy(), want), b


# --------------------------------------------------------------------------------------------------- 6: max_lag
@pytest.mark.parametrize('max_lag', [0, 1, 5, 15])
def test_bounded_lag_on_the_band_route(max_lag):
    """feed_bounded: every push is a span of the whole decode of the frames so far, `pending` and `forced` by brute force,
    and the host twin returns the same after every push; one-frame, ragged and whole pushes."""
    S, T = 64, 40
    for k, (B, mode, (left, right)) in enumerate([(1, 'one', (2, 2)), (5, 'ragged', (0, 3)), (17, 'all', (5, 2)), (5, 'one', (31, 31))]):
        trans = band_matrix(S, left, right, list(BACKGROUNDS.values())[k % 3], seed=k)
        init = synth.problem(1, 1, S, seed=k)[2]
        obs = continuous(B, T, S, seed=20 + k)
        dec = decoder(B, S, trans, init, max_lag=max_lag)
        feed_bounded(dec, [obs[b] for b in range(B)], trans, init, plan(B, T, mode, seed=k), prepare=clamp, device=DEV,
                     twin=decoder(B, S, trans, init, max_lag=max_lag, gpu=None))


@pytest.mark.parametrize('max_lag', [0, 1, 5, 15])
def test_bounded_lag_on_an_identity_matrix_holds_the_ring(max_lag):
    """A band of the diagonal alone: nothing is ever decided, every returned frame is forced; sixty one-frame pushes, the
    ring stays at its sixteen slots while the window goes round it."""
    B, S, T = 3, 64, 60
    eye = identity(S)
    init = synth.problem(1, 1, S, seed=2)[2]
    obs = continuous(B, T, S, seed=30)
    dec = decoder(B, S, eye, init, max_lag=max_lag)
    assert dec._band[:3] == (0, 0, -math.inf)

    def held(k, d):
        assert d.capacity == INITIAL_CAPACITY
    feed_bounded(dec, [obs[b] for b in range(B)], eye, init, plan(B, T, 'one'), prepare=clamp, device=DEV,
                 twin=decoder(B, S, eye, init, max_lag=max_lag, gpu=None), after=held)


# ------------------------------------------------------------------------------------------ 7: the workload's band
@pytest.mark.parametrize('tiny', [False, True])
def test_pitch_band_of_1440_states(tiny):
    """The reference's pitch matrix: 175 diagonals, -inf or log(tiny) outside them; one-frame and 8-frame pushes."""
    B, T, S = 2, 40, 1440
    trans = synth.banded_transition(S, 87.2, tiny=tiny)
    init = np.full(S, math.log(1. / S), np.float32)
    rng = np.random.default_rng(5)
    centre = np.clip(np.cumsum(rng.integers(-20, 21, size=(B, T)), axis=1) + 700, 0, S - 1)
    obs = (rng.normal(size=(B, T, S)) * 2 - (np.abs(np.arange(S)[None, None] - centre[..., None]) / 12.) ** 2).astype(np.float32)
    obs = np.maximum(obs, np.float32(-80.))
    source = [obs[b] for b in range(B)]
    eight = [(8, np.full(B, 8))] * (T // 8)
    for pushes in (plan(B, T, 'one'), eight):
        dec = decoder(B, S, trans, init)
        assert dec._band[:2] == (87, 87) and (dec._band[2] == -math.inf) == (not tiny)
        got, _ = feed_both(dec, decoder(B, S, trans, init, route='dense'), source, pushes)
        for b, want in enumerate(device_whole(source, trans, init)):
            assert np.array_equal(got[b], want), b
    assert np.array_equal(got[0], reference_path(clamp(obs[0]), trans, init))


# ------------------------------------------------------------------------------------------------------ 8: routing
def routes_of(trans, B=2):
    """(a decoder of route 'auto' with an initial vector of zeros, the device matrix); `stream_route` agrees with it."""
    S = trans.shape[0]
    matrix = torch.from_numpy(trans).to(DEV)
    auto = torbi_amd.StreamDecoder(B, S, matrix, torch.zeros(S, device=DEV), log_probs=True, gpu=0)
    assert torbi_amd.stream_route(matrix, B, S, gpu=0, log_probs=True) == auto.route
    return auto, matrix


def test_a_stray_entry_widens_the_band_or_sends_the_matrix_to_the_dense_route():
    """`viterbi.band_over` reads the band off the matrix, so one stray entry just outside a band is a band one diagonal
    wider, decoded exactly; a stray entry in the far corner is the background of a matrix without a band: at 260 states
    'auto' takes the dense route and 'band' raises, naming the reason."""
    S, B, T = 260, 2, 16
    trans = band_matrix(S, 2, 2, -np.inf, seed=1)
    trans[100, 103] = -1.5
    auto, _ = routes_of(trans)
    assert auto.route == 'band' and auto._band[:2] == (2, 3)
    obs = continuous(B, T, S, seed=2)
    check_streams([obs[b] for b in range(B)], trans, np.zeros(S, np.float32), plan(B, T, 'ragged'), reach=(2, 3))
    trans = band_matrix(S, 2, 2, -np.inf, seed=1)
    trans[0, S - 1] = -1.5
    auto, matrix = routes_of(trans)
    assert auto.route == 'dense'
    with pytest.raises(RuntimeError, match='band'):
        torbi_amd.StreamDecoder(B, S, matrix, log_probs=True, gpu=0, route='band')
    got, _ = feed_both(auto, None, [obs[b] for b in range(B)], plan(B, T, 'ragged'))
    for b, want in enumerate(device_whole([obs[b] for b in range(B)], trans, np.zeros(S, np.float32))):
        assert np.array_equal(got[b], want), b


def test_a_broken_promise_about_the_band_sends_auto_to_the_dense_route(monkeypatch):
    """Where the answer about the band is wrong -- here: forced to be one diagonal too narrow, the stray entry just outside
    the stated band -- the device's verdict on the private copy is 0: 'auto' decodes on the dense route, 'band' raises."""
    S, B = 64, 2
    trans = band_matrix(S, 2, 3, BACKGROUNDS['log_tiny'], seed=3)
    matrix = torch.from_numpy(trans).to(DEV)
    monkeypatch.setattr(viterbi, 'band_over', lambda *a, **k: (2, 2, float(BACKGROUNDS['log_tiny'])))
    assert torbi_amd.StreamDecoder(B, S, matrix, log_probs=True, gpu=0).route == 'dense'
    with pytest.raises(RuntimeError, match='differs from the background'):
        torbi_amd.StreamDecoder(B, S, matrix, log_probs=True, gpu=0, route='band')
    monkeypatch.undo()
    assert torbi_amd.StreamDecoder(B, S, matrix, log_probs=True, gpu=0, route='band')._band[:2] == (2, 3)


def test_a_band_wider_than_the_route_covers_takes_the_dense_route():
    S, B = 516, 2
    trans = band_matrix(S, 255, 255, -np.inf, seed=1)         # 255 + 255 + 4 > 512
    auto, matrix = routes_of(trans)
    assert auto.route == 'dense'
    with pytest.raises(RuntimeError, match='band'):
        torbi_amd.StreamDecoder(B, S, matrix, log_probs=True, gpu=0, route='band')
    for states in (62, 66):                                   # states the band kernels do not take
        small = band_matrix(states, 2, 2, -np.inf, seed=1)
        auto, matrix = routes_of(small)
        assert auto.route == 'dense'
        with pytest.raises(RuntimeError, match='band'):
            torbi_amd.StreamDecoder(B, states, matrix, log_probs=True, gpu=0, route='band')
    with pytest.raises(ValueError):
        torbi_amd.StreamDecoder(B, 64, gpu=0, route='bogus')


def test_no_matrix_decodes_as_the_dense_route_and_leaves_one_frame_pending():
    B, T, S = 3, 20, 64
    obs = continuous(B, T, S, seed=40)
    auto = torbi_amd.StreamDecoder(B, S, log_probs=True, gpu=0)
    dense = torbi_amd.StreamDecoder(B, S, log_probs=True, gpu=0, route='dense')
    assert auto.route == torbi_amd.stream_route(None, B, S, gpu=0, log_probs=True) and dense.route == 'dense'
    for t in range(T):
        chunk = torch.from_numpy(obs[:, t:t + 1]).to(DEV)
        out, want = auto.push(chunk), dense.push(chunk)
        assert all(torch.equal(a, o) for a, o in zip(out, want))
        assert auto.pending.tolist() == [1] * B and dense.pending.tolist() == [1] * B
    assert all(torch.equal(a, o) for a, o in zip(auto.flush(), dense.flush()))


# -------------------------------------------------------------------------------------------------------- 9: C ABI
SENTINEL = -7


def abi_call(lib, name, *args):
    torch.cuda.synchronize()
    code = getattr(lib, name)(*args)
    torch.cuda.synchronize()
    assert code == 0, (name, code)


def test_prepare_extracts_the_diagonals_and_judges_the_promise():
    lib = _lib.load()
    S, left, right = 64, 2, 5
    null = ctypes.c_void_p(0)
    for bg in (BACKGROUNDS['minus_inf'], BACKGROUNDS['log_tiny']):
        trans = band_matrix(S, left, right, bg, seed=6)
        diag = torch.full((left + right + 1, S), math.nan, device=DEV)
        ok = torch.full((1,), SENTINEL, dtype=torch.int32, device=DEV)
        assert lib.torbi_hip_stream_band_diagonals_bytes(S, left, right) == diag.numel() * 4

        def prepare(matrix, l=left, r=right):
            abi_call(lib, 'torbi_hip_stream_band_prepare', matrix.data_ptr(), S, l, r, ctypes.c_float(float(bg)), diag.data_ptr(),
                     ok.data_ptr(), 0, null)
            return int(ok.item())
        assert prepare(torch.from_numpy(trans).to(DEV)) == 1
        assert np.array_equal(diag.cpu().numpy(), diagonals(trans, left, right))
        for j, i in ((10, 10 + right + 1), (10, 10 - left - 1), (0, S - 1), (S - 1, 0)):       # one entry outside the band
            broken = trans.copy()
            broken[j, i] = np.float32(-1.)
            assert prepare(torch.from_numpy(broken).to(DEV)) == 0, (j, i)
        narrow = torch.from_numpy(trans).to(DEV)              # the right matrix, a band stated one diagonal too narrow
        diag = torch.full((left + right, S), math.nan, device=DEV)
        assert prepare(narrow, r=right - 1) == 0


def prepared(lib, trans, S, left, right, bg):
    """torbi_hip_stream_band_prepare on `trans` (numpy): (diagonals, the three words around the verdict).  The call gets the
    middle word; NaN diagonals and SENTINEL words before it."""
    diag = torch.full((left + right + 1, S), math.nan, device=DEV)
    ok = torch.full((3,), SENTINEL, dtype=torch.int32, device=DEV)
    matrix = torch.from_numpy(trans).to(DEV)
    abi_call(lib, 'torbi_hip_stream_band_prepare', matrix.data_ptr(), S, left, right, ctypes.c_float(float(bg)), diag.data_ptr(),
             ok[1:].data_ptr(), 0, ctypes.c_void_p(0))
    return diag.cpu().numpy(), ok.tolist()


@pytest.mark.parametrize('background', ['minus_inf', 'log_tiny'])
def test_prepare_with_a_left_reach_past_the_matrix(background):
    """reach_left = 70 at 64 states: diagonals 0 .. 6 name no column at all and are 0 throughout, no row has a column left of
    its band, and the promise holds."""
    lib = _lib.load()
    S, left, right, bg = 64, 70, 3, BACKGROUNDS[background]
    trans = band_matrix(S, left, right, bg, seed=7)
    diag, ok = prepared(lib, trans, S, left, right, bg)
    assert ok == [SENTINEL, 1, SENTINEL]
    assert np.array_equal(diag, diagonals(trans, left, right))
    assert not diag[:left - (S - 1)].any() and diag[left - (S - 1)].any()


@pytest.mark.parametrize('background', ['minus_inf', 'log_tiny'])
def test_prepare_with_more_diagonals_than_threads(background):
    """W = 502 diagonals for the 256 threads of a row's workgroup, 576 states: the diagonal loop strides, and so does the
    loop over the row."""
    lib = _lib.load()
    S, left, right, bg = 576, 250, 251, BACKGROUNDS[background]
    trans = band_matrix(S, left, right, bg, seed=8)
    diag, ok = prepared(lib, trans, S, left, right, bg)
    assert ok == [SENTINEL, 1, SENTINEL]
    assert np.array_equal(diag, diagonals(trans, left, right))
    broken = trans.copy()
    broken[10, 10 + right + 1] = np.float32(-1.)
    assert prepared(lib, broken, S, left, right, bg)[1] == [SENTINEL, 0, SENTINEL]


@pytest.mark.parametrize('background', ['minus_inf', 'log_tiny'])
def test_prepare_copies_nan_and_plus_inf_inside_the_band_and_writes_one_word(background):
    """The streaming route has no matrix alarm: a NaN and a +inf inside the band arrive in the diagonals by their bits, the
    promise holds, and the verdict is the only word written beside the diagonals."""
    lib = _lib.load()
    S, left, right, bg = 64, 2, 5, BACKGROUNDS[background]
    trans = band_matrix(S, left, right, bg, seed=9)
    trans[10, 11] = np.nan
    trans[20, 19] = np.inf
    diag, ok = prepared(lib, trans, S, left, right, bg)
    assert ok == [SENTINEL, 1, SENTINEL]
    want = diagonals(trans, left, right)
    assert np.isnan(want[left + 1, 10]) and np.isposinf(want[left - 1, 20])
    assert np.array_equal(diag.view(np.int32), want.view(np.int32))


@pytest.mark.parametrize('violation', ['capacity', 'out_capacity', 'base_slot'])
def test_c_abi_leaves_a_stream_whose_info_does_not_fit(violation):
    """torbi_hip_stream_band_push / _flush called directly: counts_out = -1 for the stream whose info does not fit, its
    pointer ring, memo, carried row and indices_out row byte for byte as they were, the other streams decoded."""
    lib = _lib.load()
    B, Tc, bad, S, left, right = 3, 2, 1, 64, 2, 5
    bg = BACKGROUNDS['log_tiny']
    cap, out_cap = {'capacity': (4, 8), 'out_capacity': (8, 3), 'base_slot': (8, 8)}[violation]
    wrong = {'capacity': [3, 1, 2, 0], 'out_capacity': [2, 5, 2, 0], 'base_slot': [1, cap, 1, 0]}[violation]
    obs = continuous(B, Tc, S, seed=3)
    trans, init = band_matrix(S, left, right, bg, seed=2), synth.problem(1, 1, S, seed=4)[2]
    nbytes = lib.torbi_hip_stream_state_bytes(B, S, cap)
    assert nbytes == 4 * (B * cap * S + B * cap + B * S)
    rng = np.random.default_rng(S)
    state = torch.from_numpy(rng.integers(1, 1 << 20, size=nbytes // 4).astype(np.int32)).to(DEV)
    ring = state[:B * cap * S].view(B, cap, S)
    memo = state[B * cap * S:B * cap * (S + 1)].view(B, cap)
    carried = state[B * cap * (S + 1):].view(B, S)
    out = torch.full((B, out_cap), SENTINEL, dtype=torch.int32, device=DEV)
    counts = torch.full((B,), SENTINEL, dtype=torch.int32, device=DEV)
    d_obs, d_trans, d_init = (torch.from_numpy(x).to(DEV) for x in (obs, trans, init))
    diag = torch.empty((left + right + 1, S), device=DEV)
    ok = torch.zeros(1, dtype=torch.int32, device=DEV)
    null = ctypes.c_void_p(0)
    abi_call(lib, 'torbi_hip_stream_band_prepare', d_trans.data_ptr(), S, left, right, ctypes.c_float(float(bg)), diag.data_ptr(),
             ok.data_ptr(), 0, null)
    assert int(ok.item()) == 1
    d_info = torch.from_numpy(np.array([[0, 0, Tc, 1], wrong, [0, 0, Tc, 1]], np.int32)).to(DEV)
    before = (ring[bad].clone(), memo[bad].clone(), carried[bad].clone())

    def untouched(rows):
        return (torch.equal(ring[bad], before[0]) and torch.equal(memo[bad], before[1]) and torch.equal(carried[bad], before[2])
                and bool((rows[bad] == SENTINEL).all()))
    abi_call(lib, 'torbi_hip_stream_band_push', d_obs.data_ptr(), Tc, d_info.data_ptr(), diag.data_ptr(), d_init.data_ptr(), left,
             right, ctypes.c_float(float(bg)), state.data_ptr(), nbytes, cap, out.data_ptr(), out_cap, counts.data_ptr(), -1, null,
             B, S, 0, null)
    got = counts.cpu().numpy()
    assert got[bad] == -1 and untouched(out)
    paths = {}
    for b in (0, 2):
        _, bp = reference_arrays(obs[b], trans, init)
        paths[b] = reference_path(obs[b], trans, init)
        assert got[b] == decided(bp, Tc, S) + 1, (b, got)
        assert out[b, :got[b]].cpu().tolist() == paths[b][:got[b]].tolist() and (out[b, got[b]:] == SENTINEL).all()
    info = np.array([[Tc - got[0], got[0] % cap, 1, 0], [cap + 1, 0, 1, 0], [Tc - got[2], got[2] % cap, 1, 0]], np.int32)
    rest = torch.full((B, cap + 1), SENTINEL, dtype=torch.int32, device=DEV)
    counts.fill_(SENTINEL)
    d_info = torch.from_numpy(info).to(DEV)
    abi_call(lib, 'torbi_hip_stream_band_flush', d_info.data_ptr(), state.data_ptr(), nbytes, cap, rest.data_ptr(), cap + 1,
             counts.data_ptr(), B, S, 0, null)
    more = counts.cpu().numpy()
    assert more[bad] == -1 and untouched(rest)
    for b in (0, 2):
        assert more[b] == Tc - got[b]
        assert out[b, :got[b]].cpu().tolist() + rest[b, :more[b]].cpu().tolist() == paths[b].tolist()
