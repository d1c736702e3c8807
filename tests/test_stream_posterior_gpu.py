"""torbi_amd.StreamPosteriors on an MI355X (csrc/stream_posterior.hpp): the prefix property after every push against the
float64 route `state_posteriors(prefix, gpu=None)`, bit-identity across chunkings, tiles, neighbours and stale state, the
ring, the non-finite rules, the bound on S and the C entry points' per-stream predicate.

Bounds (tests/test_posterior_gpu.py::check, POSTERIOR.md): max |gamma - ref| <= 1e-4, |sum_j gamma - 1| <= 1e-4,
|L - ref| <= 1e-6 |ref| + 4e-6 n'; NaN exactly where the reference has NaN."""
import math

import numpy as np
import pytest
import torch

import torbi_amd
from torbi_amd import _lib, synth
from stream_posterior_cases import DEVICE_GAMMA, Feeder, cpu, problem, ragged_plan, reference, same

pytestmark = pytest.mark.gpu

DEV = torch.device('cuda:0')
MAX_STATES = 8000                       # include/torbi_hip.h: TORBI_HIP_ERANGE above
KINDS = [('dense', True), ('band', False), ('none', True), ('dense', False), ('band', True), ('none', False)]


def tile(B, S):
    return _lib.load().torbi_hip_stream_posterior_tile(B, S, 0)


def decoder(B, S, trans, init, lag, log_probs=True):
    return torbi_amd.StreamPosteriors(B, S, trans, init, log_probs=log_probs, gpu=0, lag=lag)


def feeder(B, S, kind, log_probs, lag, T, seed, **kw):
    obs, trans, init = problem(B, T, S, kind, log_probs, seed)
    return Feeder(decoder(B, S, trans, init, lag, log_probs), obs, trans, init, log_probs, DEVICE_GAMMA, **kw)


def bits(t):
    return cpu(t).view(np.uint32)


# ---- 6. the prefix property after every push ---------------------------------------------------------------------------

@pytest.mark.parametrize('lag', [0, 1, 4, 8])
@pytest.mark.parametrize('B', [1, 5, 17])
@pytest.mark.parametrize('S', [1, 3, 63, 64, 65, 257])           # 64: four states per thread; the others one
def test_prefix_property_after_every_push(S, B, lag):
    T = 24
    kind, log_probs = KINDS[(S + B + lag) % len(KINDS)]
    fd = feeder(B, S, kind, log_probs, lag, T, seed=100 * S + 10 * B + lag)
    assert tile(B, S) == 1
    for Tc, f in ragged_plan(B, T, seed=S + B + lag):
        fd.push(Tc, f)
    fd.flush()
    print(f'S={S} B={B} lag={lag} {kind} log_probs={log_probs}: {fd.worst}')


@pytest.mark.parametrize('S', [64, 63])
@pytest.mark.parametrize('G,B', [(2, 511), (4, 1021), (8, 2041), (16, 4081)])     # (G = 1: every case above)
def test_every_tile_with_a_partial_last_one(G, B, S):
    assert tile(B, S) == G and B % G != 0 and tile(B - 1, S) == G // 2
    fd = feeder(B, S, 'dense', True, lag=2, T=9, seed=G + S, record=False)
    rng = np.random.default_rng(G)
    for k, Tc in enumerate((3, 1, 5)):
        f = rng.integers(0, Tc + 1, size=B)
        f[k], f[B - 1 - k] = 0, Tc                                 # the last, partial tile takes frames too
        fd.push(Tc, f)
    fd.flush()
    print(f'G={G} B={B} S={S}: {fd.worst}')


@pytest.mark.parametrize('tiny', [False, True])
def test_the_pitch_matrix_at_1440_states(tiny):
    B, T, S = 2, 12, 1440
    obs, _, init = problem(B, T, S, 'none', True, seed=14)
    trans = torch.from_numpy(synth.banded_transition(S, 12, tiny=tiny))
    fd = Feeder(decoder(B, S, trans, init, lag=3), obs, trans, init, True, DEVICE_GAMMA)
    for Tc, f in [(5, [5, 2]), (1, [0, 1]), (6, [6, 6])]:
        fd.push(Tc, f)
    fd.flush()
    print(f'1440 states, tiny={tiny}: {fd.worst}')


# ---- 7. against the device's offline route -----------------------------------------------------------------------------

@pytest.mark.parametrize('B,S', [(5, 65), (17, 64)])
def test_against_the_offline_device_route(B, S):
    T, lag = 20, 4
    fd = feeder(B, S, 'dense', True, lag, T, seed=B * S)
    trans, init = fd.trans.to(DEV), fd.init.to(DEV)
    for Tc, f in ragged_plan(B, T, seed=B):
        base, n0 = fd.base.copy(), fd.n.copy()
        rows = fd.push(Tc, f, check=False)
        n = n0 + f
        if not any(r.shape[0] for r in rows):
            continue
        g, _ = torbi_amd.forward_backward(fd.obs[:, :n.max()].to(DEV), torch.from_numpy(np.maximum(n, 1)).to(DEV), trans, init)
        for b in range(B):
            k = rows[b].shape[0]
            same(cpu(rows[b]), cpu(g[b, base[b]:base[b] + k]), 2e-4, f'stream {b} against forward_backward')


# ---- 8. chunking does not change a bit ---------------------------------------------------------------------------------

@pytest.mark.parametrize('S', [64, 65])
def test_chunking_does_not_change_a_bit(S):
    B, T, lag = 3, 23, 4
    obs, trans, init = problem(B, T, S, 'dense', True, seed=S)
    runs = []
    for cuts in ([1] * 23, [5, 5, 5, 5, 3], [23]):
        fd = Feeder(decoder(B, S, trans, init, lag), obs, trans, init, True, DEVICE_GAMMA)
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


# ---- 9. neighbours do not change a bit -----------------------------------------------------------------------------------

@pytest.mark.parametrize('S', [64, 65])
def test_neighbours_and_tiles_do_not_change_a_bit(S):
    T, lag = 11, 3
    obs, trans, init = problem(4081, T, S, 'dense', True, seed=9 + S)
    cuts = (4, 1, 6)
    runs = []
    for B in (1, 17, 33, 1021, 4081):
        sp = decoder(B, S, trans, init, lag)
        got = []
        for at, Tc in zip(np.cumsum((0,) + cuts), cuts):
            rows = sp.push(obs[:B, at:at + Tc].to(DEV))
            got += [bits(rows[0]), bits(sp.filtered()[0]), bits(sp.log_likelihood[0])]
        rest, final = sp.flush()
        runs.append(got + [bits(rest[0]), bits(final[0])])
    assert [tile(B, S) for B in (1, 17, 33, 1021, 4081)] == [1, 1, 1, 4, 16]
    for other in runs[1:]:
        assert len(other) == len(runs[0]) and all(np.array_equal(x, y) for x, y in zip(runs[0], other))


# ---- 10. the ring ------------------------------------------------------------------------------------------------------

def test_the_ring_wraps_and_grows():
    B, S, lag, T = 3, 65, 8, 100
    fd = feeder(B, S, 'dense', True, lag, T, seed=10)
    for k in range(60):
        fd.push(1, None if k % 7 else [1, 0, 1])
        assert fd.sp.capacity == 16                               # held while the window wraps (60 frames, 16 slots)
    fd.push(40)
    assert fd.sp.capacity == 64 <= torbi_amd.StreamPosteriors.round_capacity(lag + 40)
    fd.flush()
    print(f'ring: {fd.worst}')


# ---- 11. stale state ---------------------------------------------------------------------------------------------------

def test_a_stale_state_does_not_change_a_bit():
    B, S, T, lag = 5, 64, 12, 2
    obs, trans, init = problem(B, T, S, 'dense', True, seed=11)
    runs = []
    for fill in ('zero', 'ff', 'nan'):
        sp = decoder(B, S, trans, init, lag)
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


# ---- 12. flushing one stream beside carried neighbours -----------------------------------------------------------------

def test_flushing_one_stream_leaves_its_neighbours_bits():
    B, S, T, lag = 3, 65, 14, 3
    obs, trans, init = problem(B, T, S, 'dense', True, seed=12)
    runs = []
    for flushed in (True, False):
        fd = Feeder(decoder(B, S, trans, init, lag), obs, trans, init, True, DEVICE_GAMMA)
        fd.push(4)
        fd.push(2, [2, 1, 2])
        if flushed:
            rest, _ = fd.flush(items=[1])
            assert rest[0].shape[0] == 3
            fd.restart(1, problem(1, 8, S, 'dense', True, seed=120)[0][0])
        later = [fd.push(5, check=flushed), fd.push(3, [3, 3, 0], check=flushed)]
        rest, final = fd.flush(check=flushed)
        runs.append([bits(r[b]) for r in later + [rest] for b in (0, 2)] + [bits(final)[[0, 2]]])
    assert all(np.array_equal(x, y) for x, y in zip(*runs))


@pytest.mark.parametrize('route', ['dense', 'band'])
def test_flushing_no_stream_returns_nothing_and_changes_nothing(route):
    """`flush(items=[])` is the host route's ([], empty) on both device routes, and the flush after it returns the bits of an
    object that was fed the same pushes without it."""
    B, S, model = (2, 4, dict(lag=1)) if route == 'dense' else (2, 8, dict(lag=1, route='band', band=(1, 1, -math.inf)))
    obs, trans, init = problem(B, 2, S, route, True, seed=17)     # ('band': tridiagonal, -inf outside reach 1/1)
    runs = []
    for empty_flush in (True, False):
        sp = torbi_amd.StreamPosteriors(B, S, trans, init, log_probs=True, gpu=0, **model)
        assert sp.route == route
        for t in range(2):
            sp.push(obs[:, t:t + 1].to(DEV))
        if empty_flush:
            before = (sp.pending.tolist(), sp.frames.tolist(), bits(sp.log_likelihood))
            rest, final = sp.flush(items=[])
            assert rest == [] and final.dtype == torch.float32 and tuple(final.shape) == (0,) and final.device == DEV
            assert (sp.pending.tolist(), sp.frames.tolist()) == before[:2] == ([1, 1], [2, 2])
            assert np.array_equal(bits(sp.log_likelihood), before[2])
        rest, final = sp.flush()
        runs.append([bits(r) for r in rest] + [bits(final)])
    assert all(r.shape == (1, S) for r in runs[0][:B]) and not np.isnan(runs[0][-1].view(np.float32)).any()
    assert all(np.array_equal(x, y) for x, y in zip(*runs))


# ---- 13. non-finite inputs ---------------------------------------------------------------------------------------------

def test_a_nan_observation_poisons_its_stream_alone_until_the_flush():
    B, S, T, t0, lag = 5, 64, 16, 5, 2
    clean, trans, init = problem(B, T, S, 'dense', True, seed=13)
    runs = []
    for poisoned in (True, False):
        obs = clean.clone()
        if poisoned:
            obs[1, t0, 37] = math.nan
        fd = Feeder(decoder(B, S, trans, init, lag), obs, trans, init, True, DEVICE_GAMMA)
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
        fd.restart(1, problem(1, 4, S, 'dense', True, seed=130)[0][0])
        got.append(fd.push(4))                                    # clean after the flush: checked against the reference
        assert not np.isnan(cpu(got[-1][1])).any() and not np.isnan(cpu(fd.sp.log_likelihood)).any()
        runs.append([bits(rows[b]) for rows in got for b in (0, 2, 3, 4)])
    assert all(np.array_equal(x, y) for x, y in zip(*runs))       # the other streams: the same bits with and without the NaN


def test_an_initial_without_mass_gives_minus_infinity_and_nan_rows():
    S, T = 65, 6
    obs, trans, _ = problem(2, T, S, 'band', True, seed=8)
    init = torch.full((S,), -math.inf)
    fd = Feeder(decoder(2, S, trans, init, lag=1), obs, trans, init, True, DEVICE_GAMMA)
    for Tc in (2, 3, 1):
        rows = fd.push(Tc)
        assert all(np.isnan(cpu(r)).all() and r.shape[0] > 0 for r in rows)
        assert (cpu(fd.sp.log_likelihood) == -math.inf).all()
    _, final = fd.flush()
    assert (cpu(final) == -math.inf).all()


# ---- 14. the bound on S ------------------------------------------------------------------------------------------------

def test_the_largest_state_count_and_the_one_above_it():
    S = MAX_STATES
    gen = torch.Generator().manual_seed(14)
    trans = torch.rand((S, S), generator=gen) + 0.05
    trans = torch.log(trans / trans.sum(0, keepdim=True))
    obs = torch.rand((1, 2, S), generator=gen) ** 3 + 1e-3
    obs = torch.log(obs / obs.sum(-1, keepdim=True))
    init = torch.log(torch.full((S,), 1. / S))
    assert tile(1, S) == 1 and tile(1, S + 1) == -3
    fd = Feeder(decoder(1, S, trans, init, lag=1), obs, trans, init, True, DEVICE_GAMMA)
    fd.push(2)
    fd.flush()
    print(f'{S} states: {fd.worst}')
    del fd, trans
    sp = torbi_amd.StreamPosteriors(1, S + 1, None, None, log_probs=True, gpu=0, lag=1)
    with pytest.raises(_lib.TorbiHipError, match='code -3'):       # TORBI_HIP_ERANGE, before any launch
        sp.push(torch.zeros((1, 2, S + 1), device=DEV))
    assert sp.frames.tolist() == [0]


# ---- 15. the C entry points --------------------------------------------------------------------------------------------

def test_a_stream_whose_info_does_not_fit_is_left_alone():
    lib = _lib.load()
    B, S, lag, Tc, out_cap = 6, 65, 1, 2, 3
    obs, trans, init = problem(B, 6, S, 'dense', True, seed=15)
    sp = decoder(B, S, trans, init, lag)
    sp.push(obs[:, :4].to(DEV))                                   # every stream: 4 frames, 1 pending, base 3
    cap, chunk = sp.capacity, obs[:, 4:6].to(DEV).contiguous()
    fits = [1, 3, Tc, 0]
    table = [fits, [-1, 3, Tc, 0], [1, cap, Tc, 0], [1, 3, Tc + 1, 0], [1, 3, Tc, 1], fits]     # pending, base_slot, frames, fresh
    info = torch.tensor(table, dtype=torch.int32, device=DEV)
    want, _ = reference(obs, np.full(B, 6), trans, init, True)
    _, index, stream = _lib.launch(DEV)

    def call(counts):
        state = sp._state.clone()
        out = torch.full((B, out_cap, S), 7., device=DEV)
        code = lib.torbi_hip_stream_posterior_push(
            chunk.data_ptr(), Tc, info.data_ptr(), sp._expa.data_ptr(), sp._expa_t.data_ptr(), sp.initial.data_ptr(),
            state.data_ptr(), state.numel(), cap, out.data_ptr(), out_cap, None if counts is None else counts.data_ptr(), lag,
            B, S, index, stream)
        assert code == 0
        torch.cuda.synchronize()
        return state, out

    counts = torch.full((B,), 99, dtype=torch.int32, device=DEV)
    state, out = call(counts)
    assert counts.tolist() == [2, -1, -1, -1, -1, 2]
    old, new = sp._rings(), sp._rings(state)
    for b in (1, 2, 3, 4):                                         # state bytes and output rows byte-identical
        assert torch.equal(sp._state[8 * b:8 * b + 8], state[8 * b:8 * b + 8])
        assert all(np.array_equal(bits(x[b]), bits(y[b])) for x, y in zip(old, new))
        assert (out[b] == 7.).all()
    for b in (0, 5):                                               # the others are processed: rows 3 and 4 of 6 frames
        same(cpu(out[b, :2]), want[b, 3:5], DEVICE_GAMMA, f'stream {b}')
        assert (out[b, 2] == 7.).all()
    state2, out2 = call(None)                                      # a NULL counts_out is accepted
    assert torch.equal(state, state2) and torch.equal(out, out2)
    # a flush whose rows do not fit the output: -1 and nothing written; the others return their pending row
    marks = torch.tensor([[1, 3, 1, 0], [out_cap + 1, 3, 1, 0], [1, 3, 0, 0]] + [[1, 3, 1, 0]] * 3, dtype=torch.int32, device=DEV)
    out = torch.full((B, out_cap, S), 7., device=DEV)
    before = sp._state.clone()
    assert lib.torbi_hip_stream_posterior_flush(marks.data_ptr(), sp._expa.data_ptr(), sp._state.data_ptr(), sp._state.numel(), cap,
                                                out.data_ptr(), out_cap, counts.data_ptr(), B, S, index, stream) == 0
    torch.cuda.synchronize()
    assert counts.tolist() == [1, -1, 0, 1, 1, 1] and (out[1] == 7.).all() and (out[2] == 7.).all()
    assert torch.equal(before, sp._state)                          # a flush writes no state
    full, _ = reference(obs, np.full(B, 4), trans, init, True)
    same(cpu(out[0, 0]), full[0, 3], DEVICE_GAMMA, 'flushed row')


def test_a_push_does_not_synchronise_the_host():
    B, S = 5, 64
    obs, trans, init = problem(B, 12, S, 'dense', True, seed=16)
    sp = decoder(B, S, trans, init, lag=2)
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
