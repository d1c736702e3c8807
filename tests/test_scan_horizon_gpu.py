"""The pruned scan's test horizon, one-slot test and top-list filter (csrc/resident_forward.hpp: horizon[],
more(), last4[]) change which termination tests a wave pass evaluates and which outputs get a list
key, never a result: on the smallest shapes at which a horizon taken from the previous timestep can go wrong, the decoded
indices are the oracle's and the final posterior rows are, bit for bit, those of the dense route -- whole tiles and clusters."""
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


def _alternating(B, T, S):
    """Observation rows that alternate between all-equal values (nothing is pruned behind them: the scan walks deep) and one
    state far above the rest (depth 1): the horizon a deep timestep leaves overshoots the next scan, which has to stop at its
    first test, and the timestep after that is deep again.  Items differ in their peak states and start on either kind."""
    obs = np.zeros((B, T, S), np.float32)
    peak = synth.hash_u24(11, 0, B * T, seed=S).reshape(B, T) % S
    for b in range(B):
        for t in range(T):
            if (t + b // 16) % 2:
                obs[b, t] = -30.0
                obs[b, t, peak[b, t]] = 0.0
            else:
                obs[b, t] = -1.5
    return obs


def _build(name):
    if name == 'collapse':          # depth collapses and recovers; 5 list blocks, three tiles (the last with one item)
        B, T, S = 33, 16, 80
        _, trans, init = synth.problem(1, 1, S, seed=3)
        obs, frames = _alternating(B, T, S), np.full(B, T, np.int32)
    elif name == 'short_lists':     # lists shorter than any horizon: Sp = 64, four blocks
        B, T, S = 17, 8, 64
        obs, trans, init = synth.problem(B, T, S, seed=5)
        frames = np.full(B, T, np.int32)
    elif name == 'minus_inf_tails':  # most of every list is -inf
        B, T, S = 20, 10, 96
        obs, _, init = synth.problem(B, T, S, seed=7)
        trans, frames = synth.banded_transition(S, 6), np.full(B, T, np.int32)
    elif name == 'ragged':          # items end inside the launch: thr = -inf for them, slots made of ended items only
        B, T, S = 33, 12, 80
        obs, trans, init = synth.problem(B, T, S, seed=9)
        frames = (1 + np.arange(B) % T).astype(np.int32)
    elif name == 'eight_item_tiles':
        B, T, S = 9, 5, 2080
        obs, trans, init = synth.problem(B, T, S, seed=13)
        frames = np.array([5, 1, 4, 5, 2, 3, 5, 5, 4], np.int32)
    elif name == 'ties':            # many outputs equal the last entry of a top list
        B, T, S = 33, 16, 80
        obs, trans, init = synth.problem(B, T, S, seed=17)
        obs = np.round(obs / 4).astype(np.float32)
        frames = np.full(B, T, np.int32)
    else:
        raise KeyError(name)
    return obs, frames, np.ascontiguousarray(trans, dtype=np.float32), init


NAMES = ['collapse', 'short_lists', 'minus_inf_tails', 'ragged', 'eight_item_tiles', 'ties']


def case(name):
    """Inputs, the oracle's indices and the dense route's final posterior rows of a case: computed once, shared by both
    paths, never written to again."""
    if name not in _cases:
        obs, frames, trans, init = _build(name)
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
        np.testing.assert_array_equal(dense.cpu().numpy(), want, err_msg=f'{name}: the dense route itself')
        for array in (obs, frames, trans, init, want, rows):
            array.setflags(write=False)
        _cases[name] = (obs, frames, trans, init, want, rows)
    return _cases[name]


@pytest.mark.parametrize('path', ['resident', 'cluster'])
@pytest.mark.parametrize('name', NAMES)
def test_every_horizon_leaves_the_oracles_paths_and_the_dense_routes_rows(name, path):
    obs, frames, trans, init, want, rows = case(name)
    B, T, S = obs.shape
    dev = torch.device('cuda:0')
    args = [torch.tensor(x, device=dev) for x in (obs, frames, trans, init)]
    space = torch.empty(viterbi.workspace_bytes(B, T, S), dtype=torch.uint8, device=dev)
    try:
        for again in range(2):          # (the second decode finds the first one's lists and statistics in place)
            got = torbi_amd.decode(*args, workspace=space, path=path)
            torch.cuda.synchronize()
            kernel = viterbi.last_forward_kernel()
            assert kernel.startswith('resident::resident_forward_kernel<'), kernel
            assert kernel.endswith(f', {"true" if path == "cluster" else "false"}, {8 if S > 2048 else 16}, false>'), kernel
            np.testing.assert_array_equal(got.cpu().numpy(), want, err_msg=f'{name} on {path}, decode {again}')
            post = viterbi.read_posterior(space, args[1], B, T, S, path=path).cpu().numpy()
            assert np.array_equal(post.view(np.uint32), rows.view(np.uint32)), f'{name} on {path}: final posterior rows'
            if path == 'cluster':
                assert int(viterbi.scan_stats(space, B, T, S, path='resident').cpu()[127]) == 0, 'a cluster member gave up waiting'
    finally:
        torbi_amd.reset_path_state()
