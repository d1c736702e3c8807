"""The pruned scan's closed-row mask (csrc/resident_forward.hpp: kMask) switches the lanes of rows whose
maxima are final off for the blocks behind a termination test, and changes no result: on the smallest shapes at which a mask
can go wrong the decoded indices are the oracle's, the final posterior rows are, bit for bit, those of the dense route, and the
launch reports the instance the shape has to run."""
import numpy as np
import pytest
import torch

import oracle
import torbi_amd
from torbi_amd import synth, viterbi
from conftest import CachedOracle

pytestmark = pytest.mark.gpu

SWITCH = 'TORBI_HIP_WHOLE_TILE_WAVES'
HEADLINE = 'resident::resident_forward_kernel<16, 6, true, 1, false, 16, false>'
TWELVE = 'resident::resident_forward_kernel<12, 6, true, 1, false, 16, false>'

_oracle = CachedOracle(oracle)
_cases = {}


def _build(name):
    """Two tiles, the second with one live item.  (inputs, waves forced, the instance that has to run)"""
    B, T = 17, 6
    frames = np.full(B, T, np.int32)
    if name == 'headline':          # 73 row groups: lanes past S in the last one, closed from a pass's first test on
        S = 1156
        obs, trans, init = synth.problem(B, T, S, seed=61)
    elif name == 'ties':            # integer scores: bound and maximum meet exactly, a quad closes at equality
        S = 1440
        obs, trans, init = [np.round(x).astype(np.float32) for x in synth.problem(B, T, S, seed=63)]
    elif name == 'short_lists':     # 59 finite entries a row, -inf behind: a pass ends at the list's end with quads masked
        S = 1440
        obs, _, init = synth.problem(B, T, S, seed=65)
        trans = synth.banded_transition(S, 30)
    elif name == 'ragged':          # ended items have thr = -inf: their pairs are closed from the first test on
        S = 1156
        obs, trans, init = synth.problem(B, T, S, seed=67)
        frames = np.array([1, 3, 6], np.int32)[np.arange(B) % 3]
    elif name.startswith('twelve_'):            # the twelve-wave instance below 1153 states
        B, T, S = 17, 8, int(name[7:])
        obs, trans, init = synth.problem(B, T, S, seed=69)
        frames = np.full(B, T, np.int32)
        return (obs, frames, np.ascontiguousarray(trans, dtype=np.float32), init), None, TWELVE
    else:
        raise KeyError(name)
    return (obs, frames, np.ascontiguousarray(trans, dtype=np.float32), init), '16', HEADLINE


def _reference(obs, frames, trans, init, what):
    """The oracle's indices and the dense route's final posterior rows."""
    B, T, S = obs.shape
    want = _oracle.decode(obs, frames, trans, init, num_threads=oracle.max_threads())
    dev = torch.device('cuda:0')
    args = [torch.tensor(x, device=dev) for x in (obs, frames, trans, init)]
    space = torch.empty(viterbi.workspace_bytes(B, T, S), dtype=torch.uint8, device=dev)
    try:
        dense = torbi_amd.decode(*args, workspace=space, path='dense')
        rows = viterbi.read_posterior(space, args[1], B, T, S, path='dense').cpu().numpy()
        torch.cuda.synchronize()
    finally:
        torbi_amd.reset_path_state()
    np.testing.assert_array_equal(dense.cpu().numpy(), want, err_msg=f'{what}: the dense route itself')
    return want, rows


def case(name):
    """Inputs and references of a case: computed once, shared, read-only."""
    if name not in _cases:
        inputs, waves, expected = _build(name)
        want, rows = _reference(*inputs, name)
        for array in inputs + (want, rows):
            array.setflags(write=False)
        _cases[name] = (inputs, want, rows, waves, expected)
    return _cases[name]


@pytest.mark.parametrize('name', ['headline', 'ties', 'short_lists', 'ragged', 'twelve_96', 'twelve_400'])
def test_masked_scans_leave_the_oracles_paths_and_the_dense_routes_rows(name, monkeypatch):
    (obs, frames, trans, init), want, rows, waves, expected = case(name)
    B, T, S = obs.shape
    dev = torch.device('cuda:0')
    args = [torch.tensor(x, device=dev) for x in (obs, frames, trans, init)]
    space = torch.empty(viterbi.workspace_bytes(B, T, S), dtype=torch.uint8, device=dev)
    if waves is None:
        monkeypatch.delenv(SWITCH, raising=False)
    else:
        monkeypatch.setenv(SWITCH, waves)
    try:
        viterbi._depth_record(args[2], S)[0] = 0.0          # a scan depth on record: the one-seed instance
        got = torbi_amd.decode(*args, workspace=space, path='resident')
        torch.cuda.synchronize()
        assert viterbi.last_forward_kernel() == expected
        np.testing.assert_array_equal(got.cpu().numpy(), want, err_msg=name)
        post = viterbi.read_posterior(space, args[1], B, T, S, path='resident').cpu().numpy()
        assert np.array_equal(post.view(np.uint32), rows.view(np.uint32)), f'{name}: final posterior rows'
    finally:
        torbi_amd.reset_path_state()


def test_a_masked_launch_group_of_three_unequal_batches_is_exact(monkeypatch):
    S, T = 1156, 6
    _, trans, init = synth.problem(1, 1, S, seed=71)
    trans = np.ascontiguousarray(trans, dtype=np.float32)
    batches = []
    for k, B in enumerate((5, 33, 18)):
        obs, _, _ = synth.problem(B, T, S, seed=73 + k)
        frames = (1 + (np.arange(B) * 5 + k) % T).astype(np.int32)
        batches.append((obs, frames) + _reference(obs, frames, trans, init, f'batch {k}'))
    dev = torch.device('cuda:0')
    d_trans, d_init = torch.tensor(trans, device=dev), torch.tensor(init, device=dev)
    d_obs = [torch.tensor(b[0], device=dev) for b in batches]
    d_frames = [torch.tensor(b[1], device=dev) for b in batches]
    spaces = [torch.empty(viterbi.workspace_bytes(b[0].shape[0], T, S), dtype=torch.uint8, device=dev) for b in batches]
    monkeypatch.setenv(SWITCH, '16')
    try:
        viterbi._depth_record(d_trans, S)[0] = 0.0
        got = viterbi.decode_batches(d_obs, d_frames, d_trans, d_init, workspaces=spaces, path='resident')
        torch.cuda.synchronize()
        assert viterbi.last_forward_kernel() == HEADLINE
        for k, (obs, frames, want, rows) in enumerate(batches):
            np.testing.assert_array_equal(got[k].cpu().numpy(), want, err_msg=f'batch {k}')
            post = viterbi.read_posterior(spaces[k], d_frames[k], obs.shape[0], T, S, path='resident').cpu().numpy()
            assert np.array_equal(post.view(np.uint32), rows.view(np.uint32)), f'batch {k}: final posterior rows'
    finally:
        torbi_amd.reset_path_state()
