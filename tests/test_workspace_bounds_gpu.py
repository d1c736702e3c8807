"""No route writes behind the workspace it asked for, and every route still computes what its own tests expect.

Each case hands the call exactly the bytes its size query names -- the front of an allocation filled with 0xC3 that is
65536 bytes longer -- checks the result against the reference the route's own tests use (the oracle for decodes; the
float64 host recurrence at the tolerances of test_posterior_gpu.py, test_posterior_band_gpu.py and test_counts_gpu.py; the host
route bit for bit for k-best), then that the 65536 bytes behind the workspace still hold 0xC3, and that the call took the
route the case is about (the other models' entry points are their routes).  The decode shapes are the smallest that select
each layout of csrc/torbi_hip.hip and each of their optional regions."""
import ctypes

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

pytestmark = pytest.mark.gpu

DEV = torch.device('cuda:0')
GUARD = 65536
FILL = 0xC3


def guarded(need):
    """(the whole allocation, its first `need` bytes: same base, so the same alignment)"""
    whole = torch.full((need + GUARD,), FILL, dtype=torch.uint8, device=DEV)
    return whole, whole[:need]


def assert_guard_intact(whole):
    torch.cuda.synchronize()
    touched = torch.nonzero(whole[-GUARD:] != FILL).flatten()
    assert touched.numel() == 0, f'{touched.numel()} bytes written behind the workspace, the first {int(touched[0])} bytes in'


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


@pytest.mark.parametrize('case,shape,path,route,kernel_ok', DECODES, ids=[d[0] for d in DECODES])
def test_decode_stays_inside_its_workspace(case, shape, path, route, kernel_ok):
    B, T, S = shape
    obs, frames, trans, init = problem(B, T, S)
    want, want_rows = oracle.decode(obs, frames, trans, init, num_threads=oracle.max_threads(), return_posterior=True)
    whole, ws = guarded(viterbi.workspace_bytes(B, T, S))
    assert viterbi.forward_path(B, S, path=path) == route
    profile = []
    got = torbi_amd.decode(*to_dev(obs, frames, trans, init), workspace=ws, path=path, _profile=profile)
    np.testing.assert_array_equal(got.cpu().numpy(), want)
    assert_guard_intact(whole)
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
        assert_guard_intact(whole)


@pytest.mark.parametrize('form', ['split', 'tile'])
def test_band_decode_stays_inside_its_workspace(form, monkeypatch):
    """The band route's two forms, set up as test_gpu_parity.py::test_band_kernel_matches_the_oracle sets them up."""
    B, T, S, left, right = 17, 9, 360, 10, 3
    monkeypatch.setenv('TORBI_HIP_BAND_FORM', form)
    obs, _, init = synth.problem(B, T, S, seed=B + S)
    idx = np.arange(S)
    d = idx[None, :] - idx[:, None]
    trans = np.where((d >= -left) & (d <= right), synth.problem(1, 1, S, seed=S)[1], -np.inf).astype(np.float32)
    trans[S // 3] = -np.inf
    frames = np.clip(synth.lengths(B, 1, T, seed=3), 1, T).astype(np.int32)
    frames[0] = T
    want = oracle.decode(obs, frames, trans, init, num_threads=oracle.max_threads())
    whole, ws = guarded(viterbi.workspace_bytes(B, T, S))
    profile = []
    got = torbi_amd.decode(*to_dev(obs, frames, trans, init), workspace=ws, path='band', _profile=profile)
    np.testing.assert_array_equal(got.cpu().numpy(), want)
    assert_guard_intact(whole)
    assert viterbi.ROUTES[int(profile[3])] == 'band', viterbi.ROUTES[int(profile[3])]
    assert ('band_tile_kernel' in viterbi.last_forward_kernel()) == (form == 'tile'), viterbi.last_forward_kernel()


def test_kept_preparation_of_exactly_the_stated_size():
    """torbi_hip_viterbi_decode_batches_prepared with a caller's buffer of exactly torbi_hip_preparation_bytes(S): filled by the
    first call, reused (and left as it is) by the second; nothing behind it or behind the workspace is written."""
    lib = _lib.load()
    B, T, S = 40, 5, 64
    obs, frames, trans, init = problem(B, T, S)
    want = oracle.decode(obs, frames, trans, init, num_threads=oracle.max_threads())
    d_obs, d_frames, d_trans, d_init = to_dev(obs, frames, trans, init)
    kept_bytes = int(lib.torbi_hip_preparation_bytes(S))
    kept_whole, kept = guarded(kept_bytes)
    assert kept.data_ptr() % 256 == 0
    _, index, stream = _lib.launch(DEV)
    filled = ctypes.c_int(0)
    held = None
    for reuse in (0, 1):
        whole, ws = guarded(viterbi.workspace_bytes(B, T, S))       # (a workspace per call: what the kept buffer is for)
        out = torch.full((B, T), -1, dtype=torch.int32, device=DEV)
        table = (_lib.Batch * 1)(_lib.Batch(d_obs.data_ptr(), d_frames.data_ptr(), out.data_ptr(), ws.data_ptr(), ws.numel(),
                                            B, T))
        phases = (ctypes.c_float * 6)()
        _lib.check(lib.torbi_hip_viterbi_decode_batches_prepared(
            table, 1, d_trans.data_ptr(), d_init.data_ptr(), S, index, stream, viterbi._path_flag('resident') | reuse, phases,
            kept.data_ptr(), kept_bytes, ctypes.byref(filled)), 'torbi_hip_viterbi_decode_batches_prepared')
        np.testing.assert_array_equal(out.cpu().numpy(), want)
        assert_guard_intact(whole)
        assert_guard_intact(kept_whole)
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
    whole, ws = guarded(torbi_amd.forward_backward_workspace_bytes(B, T, S))
    transition, _, initial = inputs.model(torch.as_tensor(trans), torch.as_tensor(init), True, S, DEV)      # as state_posteriors
    g, L = torbi_amd.forward_backward(inputs.observation(torch.as_tensor(obs), True, DEV), torch.as_tensor(frames).to(DEV),
                                      transition, initial, workspace=ws)
    posterior_cases.check((g.cpu().numpy().astype(np.float64), L.cpu().numpy().astype(np.float64)), want, frames)
    assert_guard_intact(whole)


def test_forward_backward_counts_stays_inside_its_workspace():
    B, T, S = OTHER
    obs, frames, trans, init = problem(B, T, S)
    rX, rI, _ = counts_cases.host(obs, frames, trans, init)
    whole, ws = guarded(torbi_amd.training.expected_counts_workspace_bytes(B, T, S))
    post, L, X, I = torbi_amd.forward_backward_counts(*to_dev(obs, frames, trans, init), workspace=ws)
    counts_cases.check_counts(X, I, rX, rI, frames, T)
    assert_guard_intact(whole)
    post2, L2 = torbi_amd.forward_backward(*to_dev(obs, frames, trans, init))       # (the dense route's, bit for bit)
    assert torch.equal(post, post2) and torch.equal(L, L2)


def test_forward_backward_banded_stays_inside_its_workspace():
    case = OTHER + (2, 1, band_cases.NINF)
    obs, frames, trans, init = band_cases.problem(*case)
    whole, ws = guarded(torbi_amd.forward_backward_banded_workspace_bytes(*case[:5]))
    got = band_cases.banded(obs, frames, trans, init, *case[3:], workspace=ws)
    band_cases.check(got, band_cases.reference(*case), frames)
    assert_guard_intact(whole)


def test_k_best_stays_inside_its_workspace():
    B, T, S = OTHER
    k = 3
    obs, frames, trans, init = problem(B, T, S)
    whole, ws = guarded(torbi_amd.k_best.decode_k_best_workspace_bytes(B, T, S, k))
    k_best_cases.same(k_best_cases.device(obs, frames, trans, init, k, workspace=ws), k_best_cases.host(obs, frames, trans, init, k))
    assert_guard_intact(whole)
