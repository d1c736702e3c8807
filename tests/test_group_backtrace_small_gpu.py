"""The backtrace over the sorted rows with its streamed first argmax (csrc/lazy_backtrace.hpp, GatherWalker::first_state): the
launch group's whole-path kernel, the segment and stitch kernels of few paths, and two launch groups issued back to back on
two streams -- indices against the oracle, the forward kernel by name."""
import numpy as np
import pytest
import torch

import oracle
import torbi_amd
from torbi_amd import synth, viterbi
from conftest import CachedOracle

pytestmark = pytest.mark.gpu

_oracle = CachedOracle(oracle)
_problems = {}

# (items, frames, states): NQ = 6, 2, 8 and 16 float4 of a posterior row per lane; 4096 states decode in 8-item tiles
SHAPES = [(40, 37, 1440), (24, 9, 512), (24, 9, 2048), (12, 9, 4096)]


def problem(B, T, S, ties):
    """`B` different items with ragged lengths (T, 1, 2, about T / 2, T - 1 in turn) and the oracle's paths for them, computed
    once per shape and never written to again.  `ties`: every score a multiple of 0.5, so that equal maxima reach the first
    argmax of a final row (first_state) and of a path step (step) and the lowest state has to win."""
    key = (B, T, S, ties)
    if key not in _problems:
        obs, trans, init = synth.problem(B, T, S, seed=S + T)
        if ties:
            obs, trans, init = (np.round(x * 2) / 2 for x in (obs, trans, init))
        frames = np.resize(np.array([T, 1, 2, max(1, T // 2), T - 1], np.int32), B)
        want = _oracle.decode(obs, frames, trans, init, num_threads=oracle.max_threads())
        for array in (obs, trans, init, frames, want):
            array.setflags(write=False)
        _problems[key] = (obs, frames, trans, init, want)
    return _problems[key]


def batches_of(B, count):
    """Which items the batches of a group hold: the same items in different order and number, so that the tiles of the group
    differ and every batch is checked against the one set of oracle paths."""
    return [np.roll(np.arange(B), 7 * k)[:B - 3 * k] for k in range(count)]


def forward_instance(S):
    """The whole-tile instance launch_whole_tiles names for a few tiles at S states: 16 items per tile up to 2048 states, 8
    above; only the tile size is pinned here (tests/test_instance_arms_gpu.py pins every argument)."""
    return f', {8 if S > 2048 else 16}, false>'


@pytest.mark.parametrize('segments', [None, '1'], ids=['segments', 'whole-paths'])
@pytest.mark.parametrize('ties', [False, True], ids=['plain', 'ties'])
@pytest.mark.parametrize('count', [2, 3])
@pytest.mark.parametrize('shape', SHAPES, ids=['x'.join(map(str, s)) for s in SHAPES])
def test_launch_groups_walk_the_oracles_paths_from_the_streamed_first_argmax(shape, count, ties, segments, monkeypatch):
    """decode_batches of two and of three ragged batches on the time-resident kernel.  A group this small walks every path in
    speculative segments (group_segment_gather_kernel, group_stitch_gather_kernel); with TORBI_HIP_BACKTRACE_SEGMENTS=1 it
    walks whole paths as a full launch group does (group_backtrace_gather_kernel).  Both start from
    GatherWalker::first_state, at every NQ."""
    B, T, S = shape
    obs, frames, trans, init, want = problem(B, T, S, ties)
    dev = torch.device('cuda:0')
    if segments is None:
        monkeypatch.delenv('TORBI_HIP_BACKTRACE_SEGMENTS', raising=False)
    else:
        monkeypatch.setenv('TORBI_HIP_BACKTRACE_SEGMENTS', segments)
    d_obs, d_frames = torch.tensor(obs, device=dev), torch.tensor(frames, device=dev)
    picks = batches_of(B, count)
    try:
        got = torbi_amd.decode_batches([d_obs[torch.tensor(p, device=dev)] for p in picks],
                                       [d_frames[torch.tensor(p, device=dev)] for p in picks],
                                       torch.tensor(trans, device=dev), torch.tensor(init, device=dev), path='resident')
        torch.cuda.synchronize()
        kernel = viterbi.last_forward_kernel()
    finally:
        torbi_amd.reset_path_state()
    assert kernel.startswith('resident::resident_forward_kernel<') and kernel.endswith(forward_instance(S)), kernel
    for k, (p, g) in enumerate(zip(picks, got)):
        np.testing.assert_array_equal(g.cpu().numpy(), want[p], err_msg=f'batch {k} of {count}, {shape}, ties={ties}')


@pytest.mark.parametrize('ties', [False, True], ids=['plain', 'ties'])
def test_one_batch_walks_the_oracles_paths_in_segments(ties, monkeypatch):
    """One batch of 40 x 37 x 1440 on the time-resident kernel: the segment and stitch kernels of a single call, on the same
    walker."""
    B, T, S = SHAPES[0]
    obs, frames, trans, init, want = problem(B, T, S, ties)
    dev = torch.device('cuda:0')
    monkeypatch.delenv('TORBI_HIP_BACKTRACE_SEGMENTS', raising=False)
    try:
        got = torbi_amd.decode(torch.tensor(obs, device=dev), torch.tensor(frames, device=dev), torch.tensor(trans, device=dev),
                               torch.tensor(init, device=dev), path='resident')
        torch.cuda.synchronize()
        kernel = viterbi.last_forward_kernel()
    finally:
        torbi_amd.reset_path_state()
    assert kernel.startswith('resident::resident_forward_kernel<') and kernel.endswith(forward_instance(S)), kernel
    np.testing.assert_array_equal(got.cpu().numpy(), want, err_msg=f'ties={ties}')


@pytest.mark.parametrize('ties', [False, True], ids=['plain', 'ties'])
def test_two_full_chip_groups_back_to_back_on_two_streams_equal_the_oracle(ties):
    """Two launch groups of two 2064 x 3 x 1440 batches (258 tiles a group: more workgroups than compute units) through
    DecodePipeline(depth=2, group=2), forced to the time-resident kernel: the second group's forward launch is queued on the
    other stream while the first group's runs, and the first group's backtrace -- 4128 whole paths, small enough in registers
    to run beside that forward launch -- must still find the first group's complete history.  Every batch of both groups
    equals the oracle."""
    B, T, S, distinct = 2064, 3, 1440, 40
    obs, _, trans, init, _ = problem(distinct, 37, S, ties)
    obs = np.ascontiguousarray(obs[:, :T])
    frames = np.resize(np.array([3, 1, 2], np.int32), distinct)
    want = _oracle.decode(obs, frames, trans, init, num_threads=oracle.max_threads())
    dev = torch.device('cuda:0')
    d_obs, d_frames = torch.tensor(obs, device=dev), torch.tensor(frames, device=dev)
    d_trans, d_init = torch.tensor(trans, device=dev), torch.tensor(init, device=dev)
    items = [(np.arange(B) + 11 * k) % distinct for k in range(4)]
    inputs = [(d_obs[torch.tensor(i, device=dev)], d_frames[torch.tensor(i, device=dev)]) for i in items]
    torch.cuda.synchronize()
    try:
        pipe = torbi_amd.DecodePipeline(dev, depth=2, group=2, reuse_preparation=False, path='resident')
        pipe.reserve(B, T, S)
        got = [pipe.decode(o, f, d_trans, d_init) for o, f in inputs]
        pipe.synchronize()
        kernel = viterbi.last_forward_kernel()
    finally:
        torbi_amd.reset_path_state()
    assert kernel.startswith('resident::resident_forward_kernel<') and kernel.endswith(forward_instance(S)), kernel
    for k, (i, g) in enumerate(zip(items, got)):
        np.testing.assert_array_equal(g.cpu().numpy(), want[i], err_msg=f'batch {k} (group {k // 2}), ties={ties}')
