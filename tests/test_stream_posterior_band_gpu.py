"""The band route of torbi_amd.StreamPosteriors on an MI355X (csrc/stream_posterior_band.hpp): the prefix property after every
push against the float64 route `state_posteriors(prefix, gpu=None)`, every tile size, the pitch matrix and the edges of the
coverage, bit-identity across chunkings, tiles, neighbours, stale state and the ring, agreement with the dense device route
and with `forward_backward_banded`, the non-finite rules, the per-stream predicate, the promise and the absence of host
synchronisation.

Bounds (tests/test_posterior_gpu.py::check, POSTERIOR.md): max |gamma - ref| <= 1e-4, |sum_j gamma - 1| <= 1e-4,
|L - ref| <= 1e-6 |ref| + 4e-6 n'; 2e-4 between two device routes; NaN exactly where the reference has NaN."""
import math

import numpy as np
import pytest
import torch

import torbi_amd
from torbi_amd import _lib, synth
from stream_posterior_cases import DEVICE_GAMMA, Feeder, cpu, problem, ragged_plan, reference, same
from stream_posterior_band_cases import BACKGROUNDS, EUNSUPPORTED, MAX_STATES, TILES, TINY, band_problem, bits

pytestmark = pytest.mark.gpu

DEV = torch.device('cuda:0')
BETWEEN_ROUTES = 2e-4
STATES = [1, 5, 37, 64, 65, 257]
BATCHES = [1, 5, 17]
LAGS = [0, 1, 4, 8]
REACHES = [(0, 0), (1, 2), (5, 2), (3, 0)]


def tile(B, S, left, right):
    return _lib.load().torbi_hip_stream_smooth_band_tile(B, S, left, right, 0)


def decoder(B, S, trans, init, lag, log_probs=True, **kw):
    sp = torbi_amd.StreamPosteriors(B, S, trans, init, log_probs=log_probs, gpu=0, lag=lag, **kw)
    assert sp.route == ('band' if kw else 'dense')
    return sp


def feeder(B, T, S, left, right, background, log_probs, lag, seed, **kw):
    obs, trans, init, band = band_problem(B, T, S, left, right, background, log_probs, seed)
    return Feeder(decoder(B, S, trans, init, lag, log_probs, route='band', band=band), obs, trans, init, log_probs, DEVICE_GAMMA, **kw)


# ---- 1. the prefix property after every push ---------------------------------------------------------------------------

@pytest.mark.parametrize('lag', LAGS)
@pytest.mark.parametrize('B', BATCHES)
@pytest.mark.parametrize('S', STATES)
def test_prefix_property_after_every_push(S, B, lag):
    T = 24
    k = (STATES.index(S) * len(BATCHES) + BATCHES.index(B)) * len(LAGS) + LAGS.index(lag)
    (left, right), background, log_probs = REACHES[(k + k // 4) % 4], BACKGROUNDS[k % 3], (k // 3) % 2 == 0
    fd = feeder(B, T, S, left, right, background, log_probs, lag, seed=100 * S + 10 * B + lag)
    plan = ragged_plan(B, T, seed=S + B + lag)
    assert len(plan) >= 6 and any(Tc == 0 for Tc, _ in plan) and any(Tc == 7 for Tc, _ in plan)
    for Tc, f in plan:
        if B >= 2:
            assert (f == 0).any() and (f == Tc).any()
        fd.push(Tc, f)
    fd.flush()
    print(f'S={S} B={B} lag={lag} reach {left}/{right} background {background} log_probs={log_probs}: {fd.worst}')


@pytest.mark.parametrize('log_probs', [True, False])
@pytest.mark.parametrize('background', BACKGROUNDS)
def test_prefix_property_on_a_band_the_matrix_edges_clip(background, log_probs):
    B, T, S, lag = 5, 24, 37, 4                                    # 36 / 36: the whole matrix is the band, 73 diagonals of it
    fd = feeder(B, T, S, 36, 36, background, log_probs, lag, seed=37)
    for Tc, f in ragged_plan(B, T, seed=37):
        fd.push(Tc, f)
    fd.flush()
    print(f'S=37 reach 36/36 background {background} log_probs={log_probs}: {fd.worst}')


# ---- 2. every tile size ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('S', [64, 63])
@pytest.mark.parametrize('G,B', TILES[1:])                       # (G = 1: every case above)
def test_every_tile_with_a_partial_last_one(G, B, S):
    left, right = 1, 2
    assert tile(B, S, left, right) == G and B % G != 0 and tile(B - 1, S, left, right) == G // 2
    fd = feeder(B, 9, S, left, right, BACKGROUNDS[G % 3], True, lag=2, seed=G + S, record=False)
    rng = np.random.default_rng(G)
    for k, Tc in enumerate((3, 1, 5)):
        f = rng.integers(0, Tc + 1, size=B)
        f[k], f[B - 1 - k] = 0, Tc                                 # the last, partial tile takes frames too
        fd.push(Tc, f)
    fd.flush()
    print(f'G={G} B={B} S={S}: {fd.worst}')


# ---- 3. the pitch matrix and the edges of the coverage -----------------------------------------------------------------

@pytest.mark.parametrize('tiny', [False, True])
def test_the_pitch_matrix_through_the_planner_and_as_a_stated_band(tiny):
    B, T, S = 2, 12, 1440
    obs, _, init = problem(B, T, S, 'none', True, seed=14)
    trans = torch.from_numpy(synth.banded_transition(S, 12, tiny=tiny))          # 23 diagonals
    runs = []
    for kw in (dict(route='band'), dict(route='band', band=(11, 11, TINY if tiny else -math.inf))):
        fd = Feeder(decoder(B, S, trans, init, 3, **kw), obs, trans, init, True, DEVICE_GAMMA)
        got = []
        for Tc, f in [(5, [5, 2]), (1, [0, 1]), (6, [6, 6])]:
            got += [bits(r) for r in fd.push(Tc, f)] + [bits(fd.sp.filtered()), bits(fd.sp.log_likelihood)]
        rest, final = fd.flush()
        runs.append(got + [bits(r) for r in rest] + [bits(final)])
        print(f'1440 states, tiny={tiny}, {kw}: {fd.worst}')
    assert len(runs[0]) == len(runs[1]) and all(np.array_equal(x, y) for x, y in zip(*runs))


def test_the_largest_state_count_with_the_widest_band():
    B, T, S, left, right = 1, 6, MAX_STATES, 31, 32
    fd = feeder(B, T, S, left, right, -20., True, lag=2, seed=40)
    assert tile(B, S, left, right) == 1
    fd.push(4)
    fd.push(2)
    fd.flush()
    print(f'{S} states, reach {left}/{right}: {fd.worst}')


@pytest.mark.parametrize('S,left,right', [(MAX_STATES + 1, 31, 32), (1440, 32, 32), (MAX_STATES, 32, 32)])
def test_one_step_beyond_each_edge_is_unsupported(S, left, right):
    lib = _lib.load()
    assert tile(1, S, left, right) == EUNSUPPORTED
    with pytest.raises(RuntimeError, match='torbi_hip_stream_smooth_band_covers turns down'):
        torbi_amd.StreamPosteriors(1, S, None, None, log_probs=True, gpu=0, lag=1, route='band', band=(left, right, -3.))
    trans = torch.zeros((8, 8), device=DEV)                         # (turned down before anything is read)
    diag = torch.zeros(lib.torbi_hip_stream_smooth_band_diagonals_size(S, left, right) // 4, device=DEV)
    ok = torch.full((1,), 7, dtype=torch.int32, device=DEV)
    _, index, stream = _lib.launch(DEV)
    assert lib.torbi_hip_stream_smooth_band_prepare(trans.data_ptr(), S, left, right, -3., diag.data_ptr(), ok.data_ptr(), index,
                                                    stream) == EUNSUPPORTED
    torch.cuda.synchronize()
    assert ok.item() == 7 and not diag.any()


# ---- 4. bit identity ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('S,background', [(64, -math.inf), (65, -3.)])
def test_chunking_does_not_change_a_bit(S, background):
    B, T, lag = 3, 23, 4
    obs, trans, init, band = band_problem(B, T, S, 5, 2, background, True, seed=S)
    runs = []
    for cuts in ([1] * 23, [5, 5, 5, 5, 3], [23]):
        fd = Feeder(decoder(B, S, trans, init, lag, route='band', band=band), obs, trans, init, True, DEVICE_GAMMA)
        for Tc in cuts:
            fd.push(Tc, check=False)
        score = bits(fd.sp.log_likelihood)
        now = bits(fd.sp.filtered())
        rest, final = fd.flush(check=False)
        assert all(r.shape[0] == lag for r in rest)                # frames 19 .. 22
        runs.append((score, now, [bits(r) for r in rest], bits(final), {(b, t, n): row.view(np.uint32) for b, t, n, row in fd.returned}))
    for other in runs[1:]:
        assert np.array_equal(runs[0][0], other[0]) and np.array_equal(runs[0][1], other[1]) and np.array_equal(runs[0][3], other[3])
        for b in range(B):
            assert np.array_equal(runs[0][2][b], other[2][b])
    shared = sorted(set(runs[0][4]) & set(runs[1][4]))
    assert [(t, n) for b, t, n in shared if b == 0] == [(0, 5), (5, 10), (10, 15), (15, 20), (18, 23), (19, 23), (20, 23),
                                                         (21, 23), (22, 23)]
    for key in shared:
        assert np.array_equal(runs[0][4][key], runs[1][4][key]), key
    for key in set(runs[1][4]) & set(runs[2][4]):                  # (frames 0 .. 18 at n' = 23 where both return them)
        assert np.array_equal(runs[1][4][key], runs[2][4][key]), key


@pytest.mark.parametrize('S,background', [(64, -20.), (65, -math.inf)])
def test_neighbours_and_tiles_do_not_change_a_bit(S, background):
    T, lag, left, right = 11, 3, 1, 2
    batches = (1, 17, 511, 1021, 2041)
    obs, trans, init, band = band_problem(batches[-1], T, S, left, right, background, True, seed=9 + S)
    cuts = (4, 1, 6)
    runs = []
    for B in batches:
        sp = decoder(B, S, trans, init, lag, route='band', band=band)
        got = []
        for at, Tc in zip(np.cumsum((0,) + cuts), cuts):
            rows = sp.push(obs[:B, at:at + Tc].to(DEV))
            got += [bits(rows[0]), bits(sp.filtered()[0]), bits(sp.log_likelihood[0])]
        rest, final = sp.flush()
        runs.append(got + [bits(rest[0]), bits(final[0])])
    assert [tile(B, S, left, right) for B in batches] == [1, 1, 2, 4, 8]
    for other in runs[1:]:
        assert len(other) == len(runs[0]) and all(np.array_equal(x, y) for x, y in zip(runs[0], other))


def test_a_stale_state_does_not_change_a_bit():
    B, S, T, lag = 5, 64, 12, 2
    obs, trans, init, band = band_problem(B, T, S, 3, 0, -20., True, seed=11)
    runs = []
    for fill in ('zero', 'ff', 'nan'):
        sp = decoder(B, S, trans, init, lag, route='band', band=band)
        if fill == 'zero':
            sp._state.zero_()
        elif fill == 'ff':
            sp._state.fill_(0xFF)
        else:
            sp._state.view(torch.float32).fill_(math.nan)
        got = []
        for at, Tc, f in [(0, 5, [5, 0, 3, 5, 1]), (5, 7, None)]:
            rows = sp.push(obs[:, at:at + Tc].to(DEV), None if f is None else torch.tensor(f))
            got += [bits(r) for r in rows] + [bits(sp.filtered()), bits(sp.log_likelihood)]
        rest, final = sp.flush()
        runs.append(got + [bits(r) for r in rest] + [bits(final)])
    for other in runs[1:]:
        assert all(np.array_equal(x, y) for x, y in zip(runs[0], other))
    assert not np.isnan(runs[0][-1].view(np.float32)).any()


def test_flushing_one_stream_leaves_its_neighbours_bits():
    B, S, T, lag = 3, 65, 14, 3
    obs, trans, init, band = band_problem(B, T, S, 1, 2, -3., True, seed=12)
    runs = []
    for flushed in (True, False):
        fd = Feeder(decoder(B, S, trans, init, lag, route='band', band=band), obs, trans, init, True, DEVICE_GAMMA)
        fd.push(4)
        fd.push(2, [2, 1, 2])
        if flushed:
            rest, _ = fd.flush(items=[1])
            assert rest[0].shape[0] == 3
            fd.restart(1, problem(1, 8, S, 'none', True, seed=120)[0][0])
        later = [fd.push(5, check=flushed), fd.push(3, [3, 3, 0], check=flushed)]
        rest, final = fd.flush(check=flushed)
        runs.append([bits(r[b]) for r in later + [rest] for b in (0, 2)] + [bits(final)[[0, 2]]])
    assert all(np.array_equal(x, y) for x, y in zip(*runs))


def test_the_ring_wraps_and_grows():
    B, S, lag, T = 3, 65, 8, 100
    fd = feeder(B, T, S, 5, 2, -math.inf, True, lag, seed=10)
    for k in range(60):
        fd.push(1, None if k % 7 else [1, 0, 1])
        assert fd.sp.capacity == 16                               # held while the window wraps (60 frames, 16 slots)
    fd.push(40)
    assert fd.sp.capacity == 64 <= torbi_amd.StreamPosteriors.round_capacity(lag + 40)
    fd.flush()
    print(f'ring: {fd.worst}')


def test_the_ring_does_not_change_a_bit():
    # sixty one-frame pushes through 16 slots, then the ring grows to 64: the bits of a decoder that had 64 slots all along
    B, S, lag, T = 2, 64, 8, 100
    obs, trans, init, band = band_problem(B, T, S, 1, 2, -20., True, seed=21)
    runs = []
    for roomy in (False, True):
        fd = Feeder(decoder(B, S, trans, init, lag, route='band', band=band), obs, trans, init, True, DEVICE_GAMMA)
        if roomy:
            fd.sp._grow(64)
        for _ in range(60):
            fd.push(1, check=False)
        assert fd.sp.capacity == (64 if roomy else 16)
        fd.push(40, check=False)
        assert fd.sp.capacity == 64
        score, now = bits(fd.sp.log_likelihood), bits(fd.sp.filtered())
        rest, final = fd.flush(check=False)
        runs.append([score, now, bits(final)] + [bits(r) for r in rest] + [row.view(np.uint32) for _, _, _, row in fd.returned])
    assert len(runs[0]) == len(runs[1]) == 3 + B + B * 100 and all(np.array_equal(x, y) for x, y in zip(*runs))


# ---- 5. against the other device routes ----------------------------------------------------------------------------------

@pytest.mark.parametrize('B,S,background', [(5, 65, -math.inf), (17, 64, -3.)])
def test_against_the_dense_device_route_on_the_same_pushes(B, S, background):
    T, lag = 20, 4
    obs, trans, init, band = band_problem(B, T, S, 5, 2, background, True, seed=B * S)
    fds = [Feeder(decoder(B, S, trans, init, lag, **kw), obs, trans, init, True, DEVICE_GAMMA)
           for kw in (dict(), dict(route='band', band=band))]
    worst = 0.
    for Tc, f in ragged_plan(B, T, seed=B):
        dense, banded = (fd.push(Tc, f, check=False) for fd in fds)
        for b in range(B):
            worst = max(worst, same(cpu(banded[b]), cpu(dense[b]), BETWEEN_ROUTES, f'stream {b} against the dense route'))
        worst = max(worst, same(cpu(fds[1].sp.filtered()), cpu(fds[0].sp.filtered()), BETWEEN_ROUTES, 'filtered'))
    (dense, _), (banded, _) = (fd.flush(check=False) for fd in fds)
    for b in range(B):
        worst = max(worst, same(cpu(banded[b]), cpu(dense[b]), BETWEEN_ROUTES, f'stream {b} at the flush'))
    print(f'B={B} S={S} background {background}: band against dense {worst}')


@pytest.mark.parametrize('B,S,background', [(5, 65, -20.), (17, 64, -math.inf)])
def test_against_forward_backward_banded_at_the_flush(B, S, background):
    T, left, right = 20, 5, 2
    obs, trans, init, band = band_problem(B, T, S, left, right, background, True, seed=B + S)
    sp = decoder(B, S, trans, init, T, route='band', band=band)    # a lag of T: every row leaves at the flush
    n = np.array([T - (3 * b) % 7 for b in range(B)])
    for at in (0, 7, 14):
        rows = sp.push(obs[:, at:at + 7].to(DEV), torch.from_numpy(np.clip(n - at, 0, 7)))
        assert all(r.shape[0] == 0 for r in rows)
    rest, final = sp.flush()
    g, L = torbi_amd.forward_backward_banded(obs.to(DEV), torch.from_numpy(n).to(DEV), trans.to(DEV), init.to(DEV), left, right,
                                             background)
    worst = 0.
    for b in range(B):
        assert rest[b].shape[0] == n[b]
        worst = max(worst, same(cpu(rest[b]), cpu(g[b, :n[b]]), BETWEEN_ROUTES, f'stream {b} against forward_backward_banded'))
    same(cpu(final), cpu(L), 2 * (1e-6 * np.abs(cpu(L)) + 4e-6 * n), 'log-likelihood against forward_backward_banded')
    print(f'B={B} S={S} background {background}: band against forward_backward_banded {worst}')


# ---- 6. non-finite rules -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize('poison', [math.nan, math.inf])
def test_a_non_finite_observation_poisons_its_stream_alone_until_the_flush(poison):
    B, S, T, t0, lag = 5, 64, 16, 5, 2
    clean, trans, init, band = band_problem(B, T, S, 1, 2, -20., True, seed=13)
    runs = []
    for poisoned in (True, False):
        obs = clean.clone()
        if poisoned:
            obs[1, t0, 37] = poison
        fd = Feeder(decoder(B, S, trans, init, lag, route='band', band=band), obs, trans, init, True, DEVICE_GAMMA)
        got = [fd.push(4)]
        for Tc in (3, 1, 4):
            rows = fd.push(Tc)
            got.append(rows)
            if poisoned:
                assert np.isnan(cpu(rows[1])).all() and rows[1].shape[0] == Tc
                assert np.isnan(cpu(fd.sp.log_likelihood)).tolist() == [False, True, False, False, False]
                assert np.isnan(cpu(fd.sp.filtered())[1]).all()
        rest, final = fd.flush(items=[1])
        assert np.isnan(cpu(rest[0])).all() == poisoned and math.isnan(float(final[0])) == poisoned
        fd.restart(1, problem(1, 4, S, 'none', True, seed=130)[0][0])
        got.append(fd.push(4))                                    # clean after the flush: checked against the reference
        assert not np.isnan(cpu(got[-1][1])).any() and not np.isnan(cpu(fd.sp.log_likelihood)).any()
        runs.append([bits(rows[b]) for rows in got for b in (0, 2, 3, 4)])
    assert all(np.array_equal(x, y) for x, y in zip(*runs))       # the other streams: the same bits with and without it


def test_an_initial_without_mass_gives_minus_infinity_and_nan_rows_until_the_flush():
    S, T = 65, 10
    obs, trans, _, band = band_problem(2, T, S, 1, 2, -math.inf, True, seed=8)
    init = torch.full((S,), -math.inf)
    fd = Feeder(decoder(2, S, trans, init, 1, route='band', band=band), obs, trans, init, True, DEVICE_GAMMA)
    for Tc in (2, 3, 1):
        rows = fd.push(Tc)
        assert all(np.isnan(cpu(r)).all() and r.shape[0] > 0 for r in rows)
        assert (cpu(fd.sp.log_likelihood) == -math.inf).all()
    _, final = fd.flush()
    assert (cpu(final) == -math.inf).all()
    fd.init = problem(1, 1, S, 'none', True, seed=80)[2]            # clean after it: the same decoder with an initial that has mass
    fd.sp.initial.copy_(fd.init)
    fd.restart(0, obs[0, 6:])
    fd.restart(1, obs[1, 6:])
    rows = fd.push(4)
    assert not any(np.isnan(cpu(r)).any() for r in rows) and np.isfinite(cpu(fd.sp.log_likelihood)).all()


@pytest.mark.parametrize('background', [-math.inf, -3.])
def test_a_nan_inside_the_band_reaches_every_stream_that_takes_a_second_frame(background):
    B, S, T = 4, 64, 6
    obs, trans, init, band = band_problem(B, T, S, 1, 2, background, True, seed=17)
    trans[20, 21] = math.nan                                       # [next 20][prev 21]: inside the band
    sp = decoder(B, S, trans, init, 1, route='band', band=band)
    rows = sp.push(obs[:, :3].to(DEV), torch.tensor([3, 1, 0, 2]))
    assert [r.shape[0] for r in rows] == [2, 0, 0, 1]
    assert np.isnan(cpu(rows[0])).all() and np.isnan(cpu(rows[3])).all()
    assert np.isnan(cpu(sp.log_likelihood)).tolist() == [True, False, False, True]
    assert np.isnan(cpu(sp.filtered())).all(axis=1).tolist() == [True, False, False, True]
    assert not np.isnan(cpu(sp.filtered())[1]).any()
    rows = sp.push(obs[:, 3:4].to(DEV))                              # the second frame of stream 1, the first of stream 2
    assert np.isnan(cpu(rows[1])).all() and rows[1].shape[0] == 1 and rows[2].shape[0] == 0
    assert np.isnan(cpu(sp.log_likelihood)).tolist() == [True, True, False, True]


def test_a_stream_whose_info_does_not_fit_is_left_alone():
    lib = _lib.load()
    B, S, lag, Tc, out_cap = 7, 65, 1, 2, 3
    obs, trans, init, band = band_problem(B, 6, S, 5, 2, -20., True, seed=15)
    sp = decoder(B, S, trans, init, lag, route='band', band=band)
    sp.push(obs[:, :4].to(DEV))                                   # every stream: 4 frames, 1 pending, base 3
    cap, chunk = sp.capacity, obs[:, 4:6].to(DEV).contiguous()
    left, right, background, diagonals = sp._band
    fits = [1, 3, Tc, 0]
    # pending, base_slot, frames, fresh: a negative pending, a slot outside the ring, more frames than the push holds, a fresh
    # stream with a pending row, more frames than the ring has room for
    table = [fits, [-1, 3, Tc, 0], [1, cap, Tc, 0], [1, 3, Tc + 1, 0], [1, 3, Tc, 1], [cap - 1, 3, Tc, 0], fits]
    info = torch.tensor(table, dtype=torch.int32, device=DEV)
    want, _ = reference(obs, np.full(B, 6), trans, init, True)
    _, index, stream = _lib.launch(DEV)

    def call(counts, info=info, out_cap=out_cap):
        state = sp._state.clone()
        out = torch.full((B, out_cap, S), 7., device=DEV)
        code = lib.torbi_hip_stream_smooth_band_push(
            chunk.data_ptr(), Tc, info.data_ptr(), diagonals.data_ptr(), left, right, background, sp.initial.data_ptr(),
            state.data_ptr(), state.numel(), cap, out.data_ptr(), out_cap, None if counts is None else counts.data_ptr(), lag,
            B, S, index, stream)
        assert code == 0
        torch.cuda.synchronize()
        return state, out

    counts = torch.full((B,), 99, dtype=torch.int32, device=DEV)
    state, out = call(counts)
    assert counts.tolist() == [2, -1, -1, -1, -1, -1, 2]
    old, new = sp._rings(), sp._rings(state)
    for b in (1, 2, 3, 4, 5):                                      # state bytes and output rows byte-identical
        assert torch.equal(sp._state[8 * b:8 * b + 8], state[8 * b:8 * b + 8])
        assert all(np.array_equal(bits(x[b]), bits(y[b])) for x, y in zip(old, new))
        assert (out[b] == 7.).all()
    for b in (0, 6):                                               # the others are processed: rows 3 and 4 of 6 frames
        same(cpu(out[b, :2]), want[b, 3:5], DEVICE_GAMMA, f'stream {b}')
        assert (out[b, 2] == 7.).all()
    state2, out2 = call(None)                                      # a NULL counts_out is accepted
    assert torch.equal(state, state2) and torch.equal(out, out2)
    # more rows to return than the output holds: every stream, state and output untouched
    state, out = call(counts, out_cap=1)
    assert counts.tolist() == [-1] * B and torch.equal(state, sp._state) and (out == 7.).all()
    # a flush whose rows do not fit the output: -1 and nothing written; the others return their pending row
    marks = torch.tensor([[1, 3, 1, 0], [out_cap + 1, 3, 1, 0], [1, 3, 0, 0]] + [[1, 3, 1, 0]] * 4, dtype=torch.int32, device=DEV)
    out = torch.full((B, out_cap, S), 7., device=DEV)
    before = sp._state.clone()
    assert lib.torbi_hip_stream_smooth_band_flush(marks.data_ptr(), diagonals.data_ptr(), left, right, background, sp._state.data_ptr(),
                                                  sp._state.numel(), cap, out.data_ptr(), out_cap, counts.data_ptr(), B, S, index,
                                                  stream) == 0
    torch.cuda.synchronize()
    assert counts.tolist() == [1, -1, 0, 1, 1, 1, 1] and (out[1] == 7.).all() and (out[2] == 7.).all()
    assert torch.equal(before, sp._state)                          # a flush writes no state
    full, _ = reference(obs, np.full(B, 4), trans, init, True)
    same(cpu(out[0, 0]), full[0, 3], DEVICE_GAMMA, 'flushed row')


# ---- 7. the promise ----------------------------------------------------------------------------------------------------

def test_a_stated_band_narrower_than_the_matrix_s_raises_from_the_constructor():
    S = 65
    _, trans, init, band = band_problem(1, 1, S, 5, 2, -20., True, seed=18)
    for narrow in [(4, 2, -20.), (5, 1, -20.), (0, 0, -20.)]:
        with pytest.raises(RuntimeError, match='differs from the background'):
            torbi_amd.StreamPosteriors(1, S, trans, init, log_probs=True, gpu=0, route='band', band=narrow)
    with pytest.raises(RuntimeError, match='differs from the background'):                 # the band is right, the value is not
        torbi_amd.StreamPosteriors(1, S, trans, init, log_probs=True, gpu=0, route='auto', band=(5, 2, -20.5))
    for wider in [band, (6, 3, -20.), (31, 32, -20.)]:               # a wider band keeps the promise
        assert torbi_amd.StreamPosteriors(1, S, trans, init, log_probs=True, gpu=0, route='band', band=wider).route == 'band'


def test_a_dense_matrix_raises_under_band_and_goes_dense_under_auto():
    S = 128                                                         # (64 dense states would be a band of 64 entries per row)
    _, trans, init = problem(1, 1, S, 'dense', True, seed=19)
    with pytest.raises(RuntimeError, match=r"StreamPosteriors\(route='band'\): .*(does not hold one value|turns down)"):
        torbi_amd.StreamPosteriors(2, S, trans, init, log_probs=True, gpu=0, route='band')
    sp = torbi_amd.StreamPosteriors(2, S, trans, init, log_probs=True, gpu=0, route='auto')
    assert sp.route == 'dense' and torbi_amd.stream_posterior_route(trans, 2, S, gpu=0, log_probs=True) == 'dense'
    assert torbi_amd.StreamPosteriors(2, S, trans, init, log_probs=True, gpu=0).route == 'dense'
    assert torbi_amd.stream_posterior_route(None, 2, S, gpu=0) == 'dense'


def test_auto_takes_the_band_exactly_where_the_table_of_measured_classes_says():
    from torbi_amd import stream_posterior
    S = 1440
    trans = torch.from_numpy(synth.banded_transition(S, 12))
    # measured faster (STREAM.md): 1, 8 and 512 streams at 23 diagonals of 1440 states; nothing beyond was measured
    for B, want in [(1, 'band'), (8, 'band'), (512, 'band'), (513, 'dense'), (4096, 'dense')]:
        assert stream_posterior._band_pays(B, S, 11, 11) == (want == 'band')
        assert torbi_amd.stream_posterior_route(trans, B, S, gpu=0, log_probs=True) == want
        if B <= 8:
            assert torbi_amd.StreamPosteriors(B, S, trans, None, log_probs=True, gpu=0, route='auto').route == want
    assert torbi_amd.StreamPosteriors(1, S, trans, None, log_probs=True, gpu=0).route == 'dense'       # (the default route)
    # a band that holds a larger share of a row than the one that was measured stays dense
    assert not stream_posterior._band_pays(1, S, 12, 11) and not stream_posterior._band_pays(1, 64, 1, 2)
    assert stream_posterior._band_pays(1, 2880, 22, 23) and stream_posterior._band_pays(1, 4096, 31, 32)


# ---- 8. no host synchronisation ------------------------------------------------------------------------------------------

def test_a_push_does_not_synchronise_the_host():
    B, S = 5, 64
    obs, trans, init, band = band_problem(B, 12, S, 1, 2, -20., True, seed=16)
    sp = decoder(B, S, trans, init, 2, route='band', band=band)
    chunks = [obs[:, :5].to(DEV), obs[:, 5:12].to(DEV)]
    frames = torch.tensor([5, 0, 3, 5, 1])
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode('error')
    try:
        rows = sp.push(chunks[0], frames)
        rows += sp.push(chunks[1])
        now, score = sp.filtered(), sp.log_likelihood
        rest, final = sp.flush()
    finally:
        torch.cuda.set_sync_debug_mode('default')
    assert [r.shape[0] for r in rows] == [3, 0, 1, 3, 0, 7, 5, 7, 7, 6] and not np.isnan(cpu(final)).any()
