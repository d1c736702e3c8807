"""What a launch group's preparation leaves behind (csrc/resident_forward.hpp order_items_kernel / order_tiles_kernel, which
rank from lengths staged in the LDS; csrc/pruned_forward.hpp arrange_blocks_kernel, which arranges a list block staged in
the LDS): the items' and the tiles' order, entry for entry, against the rule the kernels' comments state, and the decode
that runs on the arranged lists against the oracle."""
import numpy as np
import pytest
import torch

import oracle
import torbi_amd
from torbi_amd import synth, viterbi
from conftest import CachedOracle

pytestmark = pytest.mark.gpu

_oracle = CachedOracle(oracle)
_tables = {}

DISTINCT, T = 24, 6
STATES = [64, 1156, 1440, 2080]        # 2080: 8-item tiles and arrange_blocks_kernel<8>; 1156: no multiple of 16
MAX_GROUP_TILES = 16384                # kMaxGroupTiles (csrc/torbi_hip.hip): words of the tile map


def table(S):
    """The oracle's path of every (item, length) pair of DISTINCT items and lengths 1 .. T: [item][length - 1][T], once per
    state count and read-only."""
    if S not in _tables:
        obs, trans, init = synth.problem(DISTINCT, T, S, seed=S)
        pairs = np.repeat(np.arange(DISTINCT), T)
        lengths = np.tile(np.arange(1, T + 1, dtype=np.int32), DISTINCT)
        want = _oracle.decode(obs[pairs], lengths, trans, init, num_threads=oracle.max_threads()).reshape(DISTINCT, T, T)
        for array in (obs, trans, init, want):
            array.setflags(write=False)
        _tables[S] = (obs, trans, init, want)
    return _tables[S]


def groups(kind):
    """[(items, lengths)] per batch.  `ragged`: batches of 1, 17, 512 and 600 items with lengths all over 1 .. T (600 items: three
    blocks of order_items_kernel, the last one part full).  `equal`: three batches with the SAME lengths, few different
    values: items tie within a batch and tiles tie across batches, and the item number / tile number has to decide."""
    if kind == 'ragged':
        sizes = [1, 17, 512, 600]
        return [((np.arange(B) + 5 * k) % DISTINCT, synth.lengths(B, 1, T, seed=k)) for k, B in enumerate(sizes)]
    lengths = np.resize(np.array([T, 2, T, T, 1, 2], np.int32), 100)
    return [((np.arange(100) + 5 * k) % DISTINCT, lengths.copy()) for k in range(3)]


def expected_orders(batches, items_per_tile, shortest_first):
    """order[] of every batch and the group's tile map, as the kernels' comments rule: items by descending length, ties by item
    number; tiles by descending length of their longest item, ties by tile number across the group; both reversed when the
    shortest go first."""
    orders, tile_lengths, tile_names = [], [], []
    for k, (_, lengths) in enumerate(batches):
        B = len(lengths)
        order = np.lexsort((np.arange(B), -lengths.astype(np.int64)))
        if shortest_first:
            order = order[::-1]
        orders.append(order.astype(np.int32))
        for j in range((B + items_per_tile - 1) // items_per_tile):
            tile_lengths.append(int(lengths[order[items_per_tile * j:items_per_tile * (j + 1)]].max()))
            tile_names.append((k << 20) | j)
    ranked = np.lexsort((np.arange(len(tile_names)), -np.array(tile_lengths, np.int64)))
    if shortest_first:
        ranked = ranked[::-1]
    return orders, np.array(tile_names, np.int32)[ranked]


def words(workspace, offset, count):
    return workspace[offset:offset + 4 * count].view(torch.int32).cpu().numpy()


@pytest.mark.parametrize('shortest_first', [False, True], ids=['longest-first', 'shortest-first'])
@pytest.mark.parametrize('kind', ['ragged', 'equal'])
@pytest.mark.parametrize('S', STATES)
def test_a_groups_items_and_tiles_are_ranked_by_the_rule_and_decode_to_the_oracle(S, kind, shortest_first, monkeypatch):
    """One decode_batches call on the time-resident kernel per group.  The item order of every batch and the tile map of the
    group are read back from the workspaces (history first, then the tile map, the statistics and the order: carve_resident)
    and must equal the stated ranking entry for entry -- a decode does not depend on the order, so the oracle alone would not
    see a wrong one --, and the indices must equal the oracle's, which needs every list block arranged without losing or
    doubling an entry.  Whole paths (TORBI_HIP_BACKTRACE_SEGMENTS=1): the segment walk reuses the tile map's words."""
    obs, trans, init, want = table(S)
    batches = groups(kind)
    dev = torch.device('cuda:0')
    monkeypatch.setenv('TORBI_HIP_BACKTRACE_SEGMENTS', '1')
    d_obs = torch.tensor(obs, device=dev)
    spaces = [torch.zeros(viterbi.workspace_bytes(len(f), T, S), dtype=torch.uint8, device=dev) for _, f in batches]
    try:
        got = torbi_amd.decode_batches([d_obs[torch.tensor(i, device=dev)] for i, _ in batches],
                                       [torch.tensor(f, device=dev) for _, f in batches], torch.tensor(trans, device=dev),
                                       torch.tensor(init, device=dev), workspaces=spaces, path='resident',
                                       shortest_first=shortest_first)
        torch.cuda.synchronize()
    finally:
        torbi_amd.reset_path_state()
    items_per_tile = 8 if S > 2048 else 16
    orders, tile_map = expected_orders(batches, items_per_tile, shortest_first)

    def history_bytes(B):
        return (B * T * S * 4 + 255) // 256 * 256
    for k, ((_, f), ws, order) in enumerate(zip(batches, spaces, orders)):
        at = history_bytes(len(f)) + 4 * MAX_GROUP_TILES + 512
        np.testing.assert_array_equal(words(ws, at, len(f)), order, err_msg=f'order[] of batch {k}, {S} states, {kind}')
    np.testing.assert_array_equal(words(spaces[0], history_bytes(len(batches[0][1])), len(tile_map)), tile_map,
                                  err_msg=f'tile map, {S} states, {kind}')
    for k, ((i, f), g) in enumerate(zip(batches, got)):
        np.testing.assert_array_equal(g.cpu().numpy(), want[i, f - 1], err_msg=f'batch {k}, {S} states, {kind}')
