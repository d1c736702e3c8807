"""The pruned scan's read-ahead, early block-boundary requests and wave priorities (csrc/resident_forward.hpp: consume(),
prio_level()) change when a posterior read is requested and which wave issues first,
never a result: on the smallest shapes that reach the places a read-ahead can go wrong, the decoded indices are the
oracle's and the final posterior rows are, bit for bit, those of the dense route -- whole tiles, clusters and a launch group."""
import numpy as np
import pytest
import torch

import oracle
import torbi_amd
from torbi_amd import synth, viterbi
from conftest import CachedOracle

pytestmark = pytest.mark.gpu

_oracle = CachedOracle(oracle)
_cases = {}


def _halves(*arrays):
    """Every score a multiple of 0.5: many candidates are exactly equal and the first maximum has to win."""
    return [(np.round(x * 2) / 2).astype(np.float32) for x in arrays]


def _build(name):
    if name in ('four_blocks', 'four_blocks_ties'):      # lists of exactly four blocks: shorter than read-ahead plus horizon
        B, T, S = 17, 8, 64
        obs, trans, init = synth.problem(B, T, S, seed=21)
        frames = np.full(B, T, np.int32)
    elif name == 'not_a_multiple_of_16':                 # lanes past S and padding entries are read ahead
        B, T, S = 17, 8, 100
        obs, trans, init = synth.problem(B, T, S, seed=23)
        frames = np.full(B, T, np.int32)
    elif name.startswith('frames_'):                     # no scan, one scan, the horizon's first real timestep
        B, T, S = 17, int(name[7:]), 100
        obs, trans, init = synth.problem(B, T, S, seed=25)
        frames = np.full(B, T, np.int32)
    elif name in ('ragged_tile', 'ragged_tile_ties'):    # items end inside the launch: their thr goes to -inf mid-way
        B, T, S = 40, 24, 272
        obs, trans, init = synth.problem(B, T, S, seed=27)
        frames = (1 + np.arange(B) % T).astype(np.int32)
    elif name == 'minus_inf_tail':                       # scans stop inside the first two blocks: the second pair of the
        B, T, S = 20, 10, 272                            # block behind them is requested and never evaluated
        obs, _, init = synth.problem(B, T, S, seed=29)
        trans, frames = synth.banded_transition(S, 5), np.full(B, T, np.int32)
    elif name == 'eight_item_tiles':                     # G = 2: eight entries per lane
        B, T, S = 24, 6, 2080
        obs, trans, init = synth.problem(B, T, S, seed=31)
        frames = np.resize(np.array([6, 1, 4, 6, 2, 3, 6, 5], np.int32), B)
    else:
        raise KeyError(name)
    if name.endswith('_ties'):
        obs, trans, init = _halves(obs, trans, init)
    return obs, frames, np.ascontiguousarray(trans, dtype=np.float32), init


NAMES = ['four_blocks', 'four_blocks_ties', 'not_a_multiple_of_16', 'frames_1', 'frames_2', 'frames_3', 'ragged_tile',
         'ragged_tile_ties', 'minus_inf_tail', 'eight_item_tiles']


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
    """Inputs, the oracle's indices and the dense route's final posterior rows of a case: computed once, shared by every
    test that needs them, never written to again."""
    if name not in _cases:
        obs, frames, trans, init = _build(name)
        want, rows = _reference(obs, frames, trans, init, name)
        for array in (obs, frames, trans, init, want, rows):
            array.setflags(write=False)
        _cases[name] = (obs, frames, trans, init, want, rows)
    return _cases[name]


def _decode_and_compare(name, path, seeds=None):
    obs, frames, trans, init, want, rows = case(name)
    B, T, S = obs.shape
    dev = torch.device('cuda:0')
    args = [torch.tensor(x, device=dev) for x in (obs, frames, trans, init)]
    space = torch.empty(viterbi.workspace_bytes(B, T, S), dtype=torch.uint8, device=dev)
    if seeds is not None:               # a scan depth on record: shallow -> one seed per item, deep -> three
        viterbi._depth_record(args[2], S)[0] = 0.0 if seeds == 1 else float(S)
    for again in range(2):              # (the second decode finds the first one's lists and statistics in place)
        got = torbi_amd.decode(*args, workspace=space, path=path)
        torch.cuda.synchronize()
        kernel = viterbi.last_forward_kernel()
        assert kernel.startswith('resident::resident_forward_kernel<'), kernel
        assert kernel.endswith(f', {"true" if path == "cluster" else "false"}, {8 if S > 2048 else 16}, false>'), kernel
        if seeds is not None:
            assert f', true, {seeds}, ' in kernel, kernel
        np.testing.assert_array_equal(got.cpu().numpy(), want, err_msg=f'{name} on {path}, decode {again}')
        post = viterbi.read_posterior(space, args[1], B, T, S, path=path).cpu().numpy()
        assert np.array_equal(post.view(np.uint32), rows.view(np.uint32)), f'{name} on {path}: final posterior rows'
        if path == 'cluster':
            assert int(viterbi.scan_stats(space, B, T, S, path='resident').cpu()[127]) == 0, 'a cluster member gave up waiting'


@pytest.mark.parametrize('path', ['resident', 'cluster'])
@pytest.mark.parametrize('name', NAMES)
def test_every_depth_leaves_the_oracles_paths_and_the_dense_routes_rows(name, path):
    try:
        _decode_and_compare(name, path)
    finally:
        torbi_amd.reset_path_state()


@pytest.mark.parametrize('seeds', [1, 3])
@pytest.mark.parametrize('name', ['ragged_tile', 'eight_item_tiles'])
def test_one_and_three_seed_instances_are_exact_at_the_depth_their_registers_gave_them(name, seeds):
    try:
        _decode_and_compare(name, 'resident', seeds=seeds)
    finally:
        torbi_amd.reset_path_state()


def test_a_launch_group_of_unequal_batches_is_exact_with_waves_of_one_and_two_passes():
    """Three batches of unequal size in ONE whole-tile launch: 272 states are 17 row groups over twelve waves, so waves 0-4
    make two passes per timestep and the others one -- the wave priorities (prio_level) differ inside a workgroup."""
    S, T = 272, 12
    _, trans, init = synth.problem(1, 1, S, seed=33)
    trans = np.ascontiguousarray(trans, dtype=np.float32)
    batches = []
    for k, B in enumerate((5, 33, 18)):
        obs, _, _ = synth.problem(B, T, S, seed=35 + k)
        frames = (1 + (np.arange(B) * 5 + k) % T).astype(np.int32)
        batches.append((obs, frames) + _reference(obs, frames, trans, init, f'batch {k}'))
    dev = torch.device('cuda:0')
    d_trans, d_init = torch.tensor(trans, device=dev), torch.tensor(init, device=dev)
    d_obs = [torch.tensor(b[0], device=dev) for b in batches]
    d_frames = [torch.tensor(b[1], device=dev) for b in batches]
    spaces = [torch.empty(viterbi.workspace_bytes(b[0].shape[0], T, S), dtype=torch.uint8, device=dev) for b in batches]
    try:
        prof = []
        got = viterbi.decode_batches(d_obs, d_frames, d_trans, d_init, workspaces=spaces, path='resident', _profile=prof)
        torch.cuda.synchronize()
        assert int(prof[2]) == 1, f'{int(prof[2])} forward launches'
        kernel = viterbi.last_forward_kernel()
        assert kernel.startswith('resident::resident_forward_kernel<12, 6, true, ') and kernel.endswith(', false, 16, false>'), kernel
        for k, (obs, frames, want, rows) in enumerate(batches):
            np.testing.assert_array_equal(got[k].cpu().numpy(), want, err_msg=f'batch {k}')
            post = viterbi.read_posterior(spaces[k], d_frames[k], obs.shape[0], T, S, path='resident').cpu().numpy()
            assert np.array_equal(post.view(np.uint32), rows.view(np.uint32)), f'batch {k}: final posterior rows'
    finally:
        torbi_amd.reset_path_state()
