"""Waves per workgroup of the whole-tile, one-seed forward instance at 73 .. 96 row groups (csrc/torbi_hip.hip:
whole_tile_waves, TORBI_HIP_WHOLE_TILE_WAVES).  More waves with fewer passes each change which wave scans which row group and
nothing else: on the smallest shapes that reach every pass count the indices are the oracle's, the final posterior rows are,
bit for bit, those of the dense route, and the launch reports the instance the rule names."""
import numpy as np
import pytest
import torch

import oracle
import torbi_amd
from torbi_amd import synth, viterbi
from conftest import CachedOracle

pytestmark = pytest.mark.gpu

WAVES = 16                  # what the rule takes once a launch's tiles fill more than half the compute units
NEW = f'resident::resident_forward_kernel<{WAVES}, 6, true, 1, false, 16, false>'
TWELVE = 'resident::resident_forward_kernel<12, 8, true, 1, false, 16, false>'
TWELVE_THREE_SEEDS = 'resident::resident_forward_kernel<12, 8, true, 3, false, 16, false>'
SWITCH = 'TORBI_HIP_WHOLE_TILE_WAVES'

_oracle = CachedOracle(oracle)
_cases = {}


def _build(name):
    if name.startswith('states_'):          # 1156: 73 row groups, 1440: 90, 1536: 96, 1530: lanes past S in the last one
        B, T, S = 17, 7, int(name[7:])
        obs, trans, init = synth.problem(B, T, S, seed=41)
    elif name == 'ties':                    # every score a multiple of 0.5: the first maximum has to win
        B, T, S = 17, 7, 1440
        obs, trans, init = [(np.round(x * 2) / 2).astype(np.float32) for x in synth.problem(B, T, S, seed=43)]
    elif name == 'short_scans':             # scans stop inside the first two blocks
        B, T, S = 17, 7, 1440
        obs, _, init = synth.problem(B, T, S, seed=45)
        trans = synth.banded_transition(S, 5)
    elif name == 'rule':                    # one tile more than half the compute units
        cus = torch.cuda.get_device_properties(0).multi_processor_count
        B, T, S = 16 * (cus // 2 + 1), 3, 1156
        obs, trans, init = synth.problem(B, T, S, seed=47)
    else:
        raise KeyError(name)
    frames = (1 + np.arange(B) % T).astype(np.int32)
    return obs, frames, np.ascontiguousarray(trans, dtype=np.float32), init


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
    """Inputs, the oracle's indices and the dense route's final posterior rows of a case: computed once, shared, read-only."""
    if name not in _cases:
        obs, frames, trans, init = _build(name)
        want, rows = _reference(obs, frames, trans, init, name)
        for array in (obs, frames, trans, init, want, rows):
            array.setflags(write=False)
        _cases[name] = (obs, frames, trans, init, want, rows)
    return _cases[name]


def _decode_and_compare(name, expected, seeds=1):
    obs, frames, trans, init, want, rows = case(name)
    B, T, S = obs.shape
    dev = torch.device('cuda:0')
    args = [torch.tensor(x, device=dev) for x in (obs, frames, trans, init)]
    space = torch.empty(viterbi.workspace_bytes(B, T, S), dtype=torch.uint8, device=dev)
    viterbi._depth_record(args[2], S)[0] = 0.0 if seeds == 1 else float(S)      # a scan depth on record: one seed / three
    got = torbi_amd.decode(*args, workspace=space, path='resident')
    torch.cuda.synchronize()
    assert viterbi.last_forward_kernel() == expected
    np.testing.assert_array_equal(got.cpu().numpy(), want, err_msg=name)
    post = viterbi.read_posterior(space, args[1], B, T, S, path='resident').cpu().numpy()
    assert np.array_equal(post.view(np.uint32), rows.view(np.uint32)), f'{name}: final posterior rows'


@pytest.mark.parametrize('name', ['states_1156', 'states_1440', 'states_1536', 'states_1530', 'ties', 'short_scans'])
def test_forced_waves_leave_the_oracles_paths_and_the_dense_routes_rows(name, monkeypatch):
    """Two tiles (one full, one of a single item), ragged lengths.  Sixteen waves: 73 row groups are five and four passes a
    wave, 90 six and five, 96 six for every wave."""
    monkeypatch.setenv(SWITCH, str(WAVES))
    try:
        _decode_and_compare(name, NEW)
    finally:
        torbi_amd.reset_path_state()


def test_a_forced_launch_group_of_unequal_batches_is_one_launch_and_exact(monkeypatch):
    S, T = 1156, 8
    _, trans, init = synth.problem(1, 1, S, seed=49)
    trans = np.ascontiguousarray(trans, dtype=np.float32)
    batches = []
    for k, B in enumerate((5, 33, 18)):
        obs, _, _ = synth.problem(B, T, S, seed=51 + k)
        frames = (1 + (np.arange(B) * 5 + k) % T).astype(np.int32)
        batches.append((obs, frames) + _reference(obs, frames, trans, init, f'batch {k}'))
    dev = torch.device('cuda:0')
    d_trans, d_init = torch.tensor(trans, device=dev), torch.tensor(init, device=dev)
    d_obs = [torch.tensor(b[0], device=dev) for b in batches]
    d_frames = [torch.tensor(b[1], device=dev) for b in batches]
    spaces = [torch.empty(viterbi.workspace_bytes(b[0].shape[0], T, S), dtype=torch.uint8, device=dev) for b in batches]
    monkeypatch.setenv(SWITCH, str(WAVES))
    try:
        viterbi._depth_record(d_trans, S)[0] = 0.0
        prof = []
        got = viterbi.decode_batches(d_obs, d_frames, d_trans, d_init, workspaces=spaces, path='resident', _profile=prof)
        torch.cuda.synchronize()
        assert int(prof[2]) == 1, f'{int(prof[2])} forward launches'
        assert viterbi.last_forward_kernel() == NEW
        for k, (obs, frames, want, rows) in enumerate(batches):
            np.testing.assert_array_equal(got[k].cpu().numpy(), want, err_msg=f'batch {k}')
            post = viterbi.read_posterior(spaces[k], d_frames[k], obs.shape[0], T, S, path='resident').cpu().numpy()
            assert np.array_equal(post.view(np.uint32), rows.view(np.uint32)), f'batch {k}: final posterior rows'
    finally:
        torbi_amd.reset_path_state()


@pytest.mark.parametrize('name, switch, seeds, expected', [
    ('rule', None, 1, NEW),                         # tiles fill more than half the units: the rule on its own
    ('rule', None, 3, TWELVE_THREE_SEEDS),          # three seeds spill at sixteen waves: twelve
    ('states_1156', None, 1, TWELVE),               # two tiles: twelve
    ('rule', '12', 1, TWELVE),                      # the switch names twelve whatever the tile count
])
def test_the_rule_and_the_switch_name_the_instance(name, switch, seeds, expected, monkeypatch):
    if switch is None:
        monkeypatch.delenv(SWITCH, raising=False)
    else:
        monkeypatch.setenv(SWITCH, switch)
    try:
        _decode_and_compare(name, expected, seeds=seeds)
    finally:
        torbi_amd.reset_path_state()
