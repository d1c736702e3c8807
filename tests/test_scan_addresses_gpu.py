"""The pruned scan takes its observation and history addresses from a table of the tile items' element offsets in the LDS
(csrc/resident_forward.hpp: sbase) plus a per-timestep scalar and the lane's state, and changes no result: on the smallest
shapes at which a wrong base can hide the decoded indices are the oracle's, the final posterior rows are, bit for bit, those of
the dense route, and the launch reports the instance the shape has to run."""
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
THREE_SEEDS = 'resident::resident_forward_kernel<12, 8, true, 3, false, 16, false>'
# three tiles on 256 compute units: sixteen members a tile.  90 row groups of 16 next-states -> a share of 6, one pass of
# twelve waves (the form that requests the next timestep's observations ahead); 65 row groups of 32 -> a share of 5 on eight waves
CLUSTER_16 = 'resident::resident_forward_kernel<12, 1, true, 1, true, 16, false>'
CLUSTER_8 = 'resident::resident_forward_kernel<8, 1, true, 1, true, 8, false>'

_oracle = CachedOracle(oracle)
_cases = {}


def _build(name):
    """(inputs, decode path, waves forced, scan depth on record as a share of S, the instance that has to run)"""
    if name == 'tail_tile':         # two tiles, the second with ONE live item: fifteen slots take a valid item's base and store
        B, T, S = 17, 6, 1156       # nothing; 73 row groups: the lanes of the last one lie past S
        obs, trans, init = synth.problem(B, T, S, seed=81)
        frames = np.full(B, T, np.int32)
        plan = ('resident', '16', 0.0, HEADLINE)
    elif name == 'permuted':        # lengths 1, 3, 6 in turn: `order` is not the identity, a slot's base is that of order[...]
        B, T, S = 35, 6, 1156
        obs, trans, init = synth.problem(B, T, S, seed=83)
        frames = np.array([1, 3, 6], np.int32)[np.arange(B) % 3]
        plan = ('resident', '16', 0.0, HEADLINE)
    elif name.startswith('twelve_'):            # the twelve-wave instance below 1153 states
        B, T, S = 17, 8, int(name[7:])
        obs, trans, init = synth.problem(B, T, S, seed=85)
        frames = np.full(B, T, np.int32)
        plan = ('resident', None, 0.0, TWELVE)
    elif name == 'three_seeds':     # a deep scan on record: three seeds per item, which stay on twelve waves
        B, T, S = 17, 6, 1156
        obs, trans, init = synth.problem(B, T, S, seed=87)
        frames = np.full(B, T, np.int32)
        plan = ('resident', None, 1.0, THREE_SEEDS)
    elif name == 'cluster_16':      # one pass a member: the observations of t + 1 are loaded at kernel entry and behind row t
        B, T, S = 40, 6, 1440
        obs, trans, init = synth.problem(B, T, S, seed=89)
        frames = np.array([6, 2, 5], np.int32)[np.arange(B) % 3]
        plan = ('cluster', None, 0.0, CLUSTER_16)
    elif name == 'cluster_8':       # 8-item tiles: two lanes per next-state, items 4g .. 4g + 3 of eight
        B, T, S = 24, 5, 2064
        obs, trans, init = synth.problem(B, T, S, seed=91)
        frames = np.array([5, 1, 4], np.int32)[np.arange(B) % 3]
        plan = ('cluster', None, 0.0, CLUSTER_8)
    else:
        raise KeyError(name)
    return (obs, frames, np.ascontiguousarray(trans, dtype=np.float32), init), plan


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
        inputs, plan = _build(name)
        want, rows = _reference(*inputs, name)
        for array in inputs + (want, rows):
            array.setflags(write=False)
        _cases[name] = (inputs, want, rows, plan)
    return _cases[name]


def _switch(monkeypatch, waves):
    if waves is None:
        monkeypatch.delenv(SWITCH, raising=False)
    else:
        monkeypatch.setenv(SWITCH, waves)


@pytest.mark.parametrize('name', ['tail_tile', 'permuted', 'twelve_96', 'twelve_400', 'three_seeds', 'cluster_16', 'cluster_8'])
def test_table_addressed_scans_leave_the_oracles_paths_and_the_dense_routes_rows(name, monkeypatch):
    (obs, frames, trans, init), want, rows, (path, waves, depth, expected) = case(name)
    B, T, S = obs.shape
    dev = torch.device('cuda:0')
    args = [torch.tensor(x, device=dev) for x in (obs, frames, trans, init)]
    space = torch.empty(viterbi.workspace_bytes(B, T, S), dtype=torch.uint8, device=dev)
    _switch(monkeypatch, waves)
    try:
        viterbi._depth_record(args[2], S)[0] = depth * S          # a scan depth on record: shallow -> one seed, deep -> three
        got = torbi_amd.decode(*args, workspace=space, path=path)
        torch.cuda.synchronize()
        assert viterbi.last_forward_kernel() == expected
        if path == 'cluster':       # (a cluster that gave up is decoded again by the repair launch: that would hide its instance)
            assert int(viterbi.scan_stats(space, B, T, S).cpu()[127]) == 0, f'{name}: workgroups gave up waiting'
        np.testing.assert_array_equal(got.cpu().numpy(), want, err_msg=name)
        post = viterbi.read_posterior(space, args[1], B, T, S, path=path).cpu().numpy()
        assert np.array_equal(post.view(np.uint32), rows.view(np.uint32)), f'{name}: final posterior rows'
    finally:
        torbi_amd.reset_path_state()


def test_a_launch_group_of_batches_of_unequal_length_takes_every_tiles_own_table(monkeypatch):
    """group_unequal_T: three batches of (17, T = 6), (5, T = 9) and (33, T = 4) in ONE forward launch -- a tile's bases are
    multiples of ITS batch's T * S, into its batch's observations and history."""
    S = 1156
    _, trans, init = synth.problem(1, 1, S, seed=93)
    trans = np.ascontiguousarray(trans, dtype=np.float32)
    batches = []
    for k, (B, T) in enumerate(((17, 6), (5, 9), (33, 4))):
        obs, _, _ = synth.problem(B, T, S, seed=95 + k)
        frames = (1 + (np.arange(B) * 5 + k) % T).astype(np.int32)
        batches.append((obs, frames) + _reference(obs, frames, trans, init, f'batch {k}'))
    dev = torch.device('cuda:0')
    d_trans, d_init = torch.tensor(trans, device=dev), torch.tensor(init, device=dev)
    d_obs = [torch.tensor(b[0], device=dev) for b in batches]
    d_frames = [torch.tensor(b[1], device=dev) for b in batches]
    spaces = [torch.empty(viterbi.workspace_bytes(b[0].shape[0], b[0].shape[1], S), dtype=torch.uint8, device=dev)
              for b in batches]
    monkeypatch.setenv(SWITCH, '16')
    try:
        viterbi._depth_record(d_trans, S)[0] = 0.0
        got = viterbi.decode_batches(d_obs, d_frames, d_trans, d_init, workspaces=spaces, path='resident')
        torch.cuda.synchronize()
        assert viterbi.last_forward_kernel() == HEADLINE
        for k, (obs, frames, want, rows) in enumerate(batches):
            B, T = obs.shape[:2]
            np.testing.assert_array_equal(got[k].cpu().numpy(), want, err_msg=f'batch {k}')
            post = viterbi.read_posterior(spaces[k], d_frames[k], B, T, S, path='resident').cpu().numpy()
            assert np.array_equal(post.view(np.uint32), rows.view(np.uint32)), f'batch {k}: final posterior rows'
    finally:
        torbi_amd.reset_path_state()


def test_items_whose_byte_offsets_lie_above_four_gigabytes_are_decoded_exactly(monkeypatch):
    """far_items: 2^17 + 17 items x 64 frames x 128 states, 4.3 GB of observations and as much history -- the last seventeen
    items' element offsets are past 2^30, their byte offsets past 2^32.  (Not 2^18 + 17 items of 64 states, the same bytes: a
    launch group holds at most 16384 tiles = 2^18 items, csrc/torbi_hip.hip kMaxGroupTiles, and a batch above that is not
    decoded by the time-resident kernel at all.)  Items are independent: the first 32 and the last 33 are compared with the
    oracle and with the dense route's rows on those items alone; every index of every item lies inside [0, S)."""
    B, T, S = (1 << 17) + 17, 64, 128
    dev = torch.device('cuda:0')
    trans = viterbi.fill_synthetic((S, S), synth.STREAM_TRANSITION, device=dev)
    init = viterbi.fill_synthetic((S,), synth.STREAM_INITIAL, device=dev)
    obs = viterbi.fill_synthetic((B, T, S), synth.STREAM_OBSERVATION, seed=97, device=dev)
    assert (B - 17) * T * S * 4 >= 1 << 32          # (the last seventeen items)
    frames = (T - torch.arange(B, device=dev) % 3).to(torch.int32)          # 64, 63, 62 in turn: `order` is not the identity
    pick = torch.cat([torch.arange(32), torch.arange(B - 33, B)]).to(dev)
    sub = [obs[pick].cpu().numpy(), frames[pick].cpu().numpy(), trans.cpu().numpy(), init.cpu().numpy()]
    want, rows = _reference(*sub, 'far_items')
    space = torch.empty(viterbi.workspace_bytes(B, T, S), dtype=torch.uint8, device=dev)
    monkeypatch.delenv(SWITCH, raising=False)
    try:
        viterbi._depth_record(trans, S)[0] = 0.0
        got = torbi_amd.decode(obs, frames, trans, init, workspace=space, path='resident')
        torch.cuda.synchronize()
        assert viterbi.last_forward_kernel() == TWELVE
        assert int(got.min()) >= 0 and int(got.max()) < S
        np.testing.assert_array_equal(got[pick].cpu().numpy(), want)
        post = viterbi.read_posterior(space, frames, B, T, S, path='resident')[pick].cpu().numpy()
        assert np.array_equal(post.view(np.uint32), rows.view(np.uint32)), 'far_items: final posterior rows'
    finally:
        torbi_amd.reset_path_state()
