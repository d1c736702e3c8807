"""No route writes outside the workspace it asked for, and every route still computes what its own tests expect.

Each case hands the call exactly the bytes its size query names -- cut out of an allocation filled with 0xC3 that has 65536
more bytes on either side (tests/workspace_cases.py) -- checks the result against the reference the route's own tests use
(the oracle for decodes; the float64 host recurrence at the tolerances of test_posterior_gpu.py, test_posterior_band_gpu.py
and test_counts_gpu.py; the host route bit for bit for k-best), then that the bytes in front of the workspace and behind it
still hold 0xC3, and that the call took the route the case is about (the other models' entry points are their routes).  The
decode shapes are the smallest that select each layout of csrc/torbi_hip.hip and each of their optional regions.

The decodes are also run over what a pooled workspace holds: zeros and 0xFF (NaN as a float, -1 as an int) must give the same
indices, and so must a workspace that has just served other data of the same shape -- then a smaller shape decodes in it.
The decode workspace is 256-byte aligned by contract (tests/test_workspace_alignment_cpu.py), so its base is never odd here;
tests/test_workspace_contract_gpu.py puts the other routes through odd bases, stale bytes and dirty predecessors."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import oracle
import torbi_amd
from torbi_amd import _lib, inputs, synth, viterbi

import test_counts_gpu as counts_cases
import test_k_best_gpu as k_best_cases
import test_posterior_band_gpu as band_cases
import test_posterior_gpu as posterior_cases
from workspace_cases import DEV, assert_guards_intact, guarded

pytestmark = pytest.mark.gpu

FILL = 0xC3


def problem(B, T, S):
    obs, trans, init = synth.problem(B, T, S, seed=B + T + S)
    frames = np.clip(synth.lengths(B, 1, T, seed=S), 1, T).astype(np.int32)
    frames[0] = T
    return obs, frames, trans, init


def to_dev(*arrays):
    return [torch.as_tensor(np.ascontiguousarray(a)).to(DEV) for a in arrays]


def resident_instance(kernel):
    """(CLUSTER, NI) of a resident::resident_forward_kernel<KW, MAXP, PIPE, KR, CLUSTER, NI, REPAIR> name"""
    args = kernel[kernel.index('<') + 1:kernel.rindex('>')].split(', ')
    return args[4] == 'true', int(args[5])


# (case, (B, T, S), path named, route expected, what the forward kernel's name has to say)
DECODES = [
    ('wavefront', (3, 5, 5), 'auto', 'small', lambda k: k.startswith('small::decode')),
    ('workgroup_with_arrive_words', (3, 5, 100), 'auto', 'small', lambda k: k.startswith('small::block_value_kernel')),
    ('generic', (3, 5, 70), 'dense', 'generic', lambda k: k.startswith('step_rows_kernel')),
    ('held_with_chase_maps', (2, 130, 100), 'held', 'held', lambda k: k == 'held::held_forward_kernel'),
    ('rows', (3, 5, 64), 'pruned', 'rows', lambda k: k == 'rowscan::step_rows_sorted_kernel'),
    ('dense', (32, 4, 64), 'dense', 'dense', lambda k: k.startswith('dense::step_dense_kernel')),
    ('whole_tiles', (40, 5, 64), 'resident', 'resident', lambda k: resident_instance(k) == (False, 16)),
    ('cluster', (17, 5, 64), 'cluster', 'cluster', lambda k: resident_instance(k) == (True, 16)),
    ('cluster_8_item_tiles', (9, 4, 2052), 'cluster', 'cluster', lambda k: resident_instance(k) == (True, 8)),
    ('length_histogram', (8193, 2, 64), 'resident', 'resident', lambda k: resident_instance(k) == (False, 16)),
]


@functools.lru_cache(maxsize=None)
def decode_problem(shape, other=0):
    """(inputs, the oracle's indices, its final posterior rows) of a decode case, computed once; `other`: other data."""
    B, T, S = shape
    obs, frames, trans, init = problem(B, T, S)
    if other:
        obs = synth.scores(synth.STREAM_OBSERVATION, (B, T, S), B + T + S + other)
        frames = np.clip(synth.lengths(B, 1, T, seed=S + other), 1, T).astype(np.int32)
    want, want_rows = oracle.decode(obs, frames, trans, init, num_threads=oracle.max_threads(), return_posterior=True)
    return (obs, frames, trans, init), want, want_rows


def decode_in(ws, case, shape, path, route, kernel_ok, other=0):
    """One decode of a DECODES case in `ws`, with everything test_decode_stays_inside_its_workspace asserts about it."""
    B, T, S = shape
    (obs, frames, trans, init), want, want_rows = decode_problem(shape, other)
    assert viterbi.forward_path(B, S, path=path) == route
    profile = []
    got = torbi_amd.decode(*to_dev(obs, frames, trans, init), workspace=ws, path=path, _profile=profile)
    np.testing.assert_array_equal(got.cpu().numpy(), want)
    assert_guards_intact(ws)
    assert viterbi.ROUTES[int(profile[3])] == route, viterbi.ROUTES[int(profile[3])]
    assert kernel_ok(viterbi.last_forward_kernel()), viterbi.last_forward_kernel()
    if case in ('dense', 'cluster'):
        # the read-back entry points find their regions through the same layouts (and the route record behind them)
        rows = viterbi.read_posterior(ws, torch.as_tensor(frames), B, T, S).cpu().numpy()
        assert np.array_equal(rows.view(np.uint32), want_rows.view(np.uint32))
        stats = viterbi.scan_stats(ws, B, T, S)
        assert stats is not None
        if case == 'cluster':
            assert int(stats.cpu()[127]) == 0       # no cluster gave up waiting
        assert_guards_intact(ws)
    if case == 'cluster_8_item_tiles':
        assert int(viterbi.scan_stats(ws, B, T, S).cpu()[127]) == 0
    return got


def smaller_decode(shape):
    """Fewer items and fewer frames at the same state count: a shape whose workspace fits the case's."""
    B, T, S = shape
    return max(1, B - 1 - B // 4), max(1, T - 1), S


@pytest.mark.parametrize('case,shape,path,route,kernel_ok', DECODES, ids=[d[0] for d in DECODES])
def test_decode_stays_inside_its_workspace(case, shape, path, route, kernel_ok):
    decode_in(guarded(viterbi.workspace_bytes(*shape), fill=FILL), case, shape, path, route, kernel_ok)


@pytest.mark.parametrize('case,shape,path,route,kernel_ok', DECODES, ids=[d[0] for d in DECODES])
def test_decode_does_not_depend_on_stale_bytes(case, shape, path, route, kernel_ok):
    """Zeros and 0xFF in every byte of the workspace: the same indices (the oracle's), the same route and kernel."""
    got = [decode_in(guarded(viterbi.workspace_bytes(*shape), fill=fill), case, shape, path, route, kernel_ok)
           for fill in (0x00, 0xFF)]
    assert torch.equal(got[0], got[1])


@pytest.mark.parametrize('case,shape,path,route,kernel_ok', DECODES, ids=[d[0] for d in DECODES])
def test_decode_after_another_decode_in_the_same_workspace(case, shape, path, route, kernel_ok):
    """Other data of the same shape first -- it leaves its arrive words, chase maps, exchange granules and route record --,
    then the case (for the cluster cases: still no cluster that gave up waiting), then a smaller shape, whose layout lies over
    what the two left."""
    ws = guarded(viterbi.workspace_bytes(*shape), fill=0xFF)
    first = decode_in(ws, case, shape, path, route, kernel_ok, other=1)
    second = decode_in(ws, case, shape, path, route, kernel_ok)
    assert not torch.equal(first, second)
    B, T, S = smaller_decode(shape)
    assert viterbi.workspace_bytes(B, T, S) <= ws.numel()
    obs, frames, trans, init = problem(B, T, S)
    want = oracle.decode(obs, frames, trans, init, num_threads=oracle.max_threads())
    got = torbi_amd.decode(*to_dev(obs, frames, trans, init), workspace=ws, path=path)
    np.testing.assert_array_equal(got.cpu().numpy(), want)
    assert_guards_intact(ws)


def test_decode_workspace_one_byte_short_raises():
    B, T, S = 3, 5, 70
    obs, frames, trans, init = problem(B, T, S)
    need = viterbi.workspace_bytes(B, T, S)
    ws = guarded(need, fill=FILL)
    with pytest.raises(RuntimeError, match='workspace'):
        torbi_amd.decode(*to_dev(obs, frames, trans, init), workspace=ws[:need - 1], path='dense')
    torch.cuda.synchronize()
    assert bool((ws == FILL).all())                 # nothing was launched
    assert_guards_intact(ws)


def band_problem(other=0):
    """The band route's problem, set up as test_gpu_parity.py::test_band_kernel_matches_the_oracle sets it up."""
    B, T, S, left, right = 17, 9, 360, 10, 3
    obs, _, init = synth.problem(B, T, S, seed=B + S + other)
    idx = np.arange(S)
    d = idx[None, :] - idx[:, None]
    trans = np.where((d >= -left) & (d <= right), synth.problem(1, 1, S, seed=S)[1], -np.inf).astype(np.float32)
    trans[S // 3] = -np.inf
    frames = np.clip(synth.lengths(B, 1, T, seed=3 + other), 1, T).astype(np.int32)
    frames[0] = T
    return obs, frames, trans, init


def band_decode_in(ws, form, other=0):
    obs, frames, trans, init = band_problem(other)
    want = oracle.decode(obs, frames, trans, init, num_threads=oracle.max_threads())
    profile = []
    got = torbi_amd.decode(*to_dev(obs, frames, trans, init), workspace=ws, path='band', _profile=profile)
    np.testing.assert_array_equal(got.cpu().numpy(), want)
    assert_guards_intact(ws)
    assert viterbi.ROUTES[int(profile[3])] == 'band', viterbi.ROUTES[int(profile[3])]
    assert ('band_tile_kernel' in viterbi.last_forward_kernel()) == (form == 'tile'), viterbi.last_forward_kernel()
    return got


@pytest.mark.parametrize('form', ['split', 'tile'])
def test_band_decode_stays_inside_its_workspace(form, monkeypatch):
    """The band route's two forms."""
    monkeypatch.setenv('TORBI_HIP_BAND_FORM', form)
    band_decode_in(guarded(viterbi.workspace_bytes(17, 9, 360), fill=FILL), form)


@pytest.mark.parametrize('form', ['split', 'tile'])
def test_band_decode_over_stale_bytes_and_after_another_decode(form, monkeypatch):
    """Zeros, 0xFF, and the workspace that has just decoded other data (the split form's exchange granules and words)."""
    monkeypatch.setenv('TORBI_HIP_BAND_FORM', form)
    need = viterbi.workspace_bytes(17, 9, 360)
    zeros = band_decode_in(guarded(need, fill=0x00), form)
    ws = guarded(need, fill=0xFF)
    assert torch.equal(band_decode_in(ws, form), zeros)
    assert not torch.equal(band_decode_in(ws, form, other=1), zeros)
    assert torch.equal(band_decode_in(ws, form), zeros)


def test_kept_preparation_of_exactly_the_stated_size():
    """torbi_hip_viterbi_decode_batches_prepared with a caller's buffer of exactly torbi_hip_preparation_bytes(S): filled by the
    first call, reused (and left as it is) by the second; nothing behind it or behind the workspace is written."""
    lib = _lib.load()
    B, T, S = 40, 5, 64
    obs, frames, trans, init = problem(B, T, S)
    want = oracle.decode(obs, frames, trans, init, num_threads=oracle.max_threads())
    d_obs, d_frames, d_trans, d_init = to_dev(obs, frames, trans, init)
    kept_bytes = int(lib.torbi_hip_preparation_bytes(S))
    kept = guarded(kept_bytes, fill=FILL)
    assert kept.data_ptr() % 256 == 0
    _, index, stream = _lib.launch(DEV)
    filled = ctypes.c_int(0)
    held = None
    for reuse in (0, 1):
        ws = guarded(viterbi.workspace_bytes(B, T, S), fill=FILL)       # (a workspace per call: what the kept buffer is for)
        out = torch.full((B, T), -1, dtype=torch.int32, device=DEV)
        table = (_lib.Batch * 1)(_lib.Batch(d_obs.data_ptr(), d_frames.data_ptr(), out.data_ptr(), ws.data_ptr(), ws.numel(),
                                            B, T))
        phases = (ctypes.c_float * 6)()
        _lib.check(lib.torbi_hip_viterbi_decode_batches_prepared(
            table, 1, d_trans.data_ptr(), d_init.data_ptr(), S, index, stream, viterbi._path_flag('resident') | reuse, phases,
            kept.data_ptr(), kept_bytes, ctypes.byref(filled)), 'torbi_hip_viterbi_decode_batches_prepared')
        np.testing.assert_array_equal(out.cpu().numpy(), want)
        assert_guards_intact(ws)
        assert_guards_intact(kept)
        assert filled.value == 1 and viterbi.ROUTES[int(phases[3])] == 'resident'
        if reuse:
            assert torch.equal(kept, held)
        else:
            held = kept.clone()
            assert bool((held != FILL).any())           # the preparation went into the caller's buffer


OTHER = (3, 6, 70)


def test_forward_backward_stays_inside_its_workspace():
    B, T, S = OTHER
    obs, frames, trans, init = problem(B, T, S)
    want = posterior_cases.host(obs, frames, trans, init)
    ws = guarded(torbi_amd.forward_backward_workspace_bytes(B, T, S), fill=FILL)
    transition, _, initial = inputs.model(torch.as_tensor(trans), torch.as_tensor(init), True, S, DEV)      # as state_posteriors
    g, L = torbi_amd.forward_backward(inputs.observation(torch.as_tensor(obs), True, DEV), torch.as_tensor(frames).to(DEV),
                                      transition, initial, workspace=ws)
    posterior_cases.check((g.cpu().numpy().astype(np.float64), L.cpu().numpy().astype(np.float64)), want, frames)
    assert_guards_intact(ws)


def test_forward_backward_counts_stays_inside_its_workspace():
    B, T, S = OTHER
    obs, frames, trans, init = problem(B, T, S)
    rX, rI, _ = counts_cases.host(obs, frames, trans, init)
    ws = guarded(torbi_amd.training.expected_counts_workspace_bytes(B, T, S), fill=FILL)
    post, L, X, I = torbi_amd.forward_backward_counts(*to_dev(obs, frames, trans, init), workspace=ws)
    counts_cases.check_counts(X, I, rX, rI, frames, T)
    assert_guards_intact(ws)
    post2, L2 = torbi_amd.forward_backward(*to_dev(obs, frames, trans, init))       # (the dense route's, bit for bit)
    assert torch.equal(post, post2) and torch.equal(L, L2)


def test_forward_backward_banded_stays_inside_its_workspace():
    case = OTHER + (2, 1, band_cases.NINF)
    obs, frames, trans, init = band_cases.problem(*case)
    ws = guarded(torbi_amd.forward_backward_banded_workspace_bytes(*case[:5]), fill=FILL)
    got = band_cases.banded(obs, frames, trans, init, *case[3:], workspace=ws)
    band_cases.check(got, band_cases.reference(*case), frames)
    assert_guards_intact(ws)


def test_k_best_stays_inside_its_workspace():
    B, T, S = OTHER
    k = 3
    obs, frames, trans, init = problem(B, T, S)
    ws = guarded(torbi_amd.k_best.decode_k_best_workspace_bytes(B, T, S, k), fill=FILL)
    k_best_cases.same(k_best_cases.device(obs, frames, trans, init, k, workspace=ws), k_best_cases.host(obs, frames, trans, init, k))
    assert_guards_intact(ws)
