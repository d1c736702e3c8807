"""Record what every byte query of the C ABI answers into tests/golden/workspace_bytes.json
(tests/test_workspace_bytes_cpu.py replays the file against the library of the tree it runs in).

Run it on the commit whose answers are to be kept, after that commit's build():

    python tests/golden/generate_workspace_bytes.py

The grid crosses every condition of the layouts: B 16 | 17 (held-matrix regions, row scan), 31 | 32 (dense plan),
1024 | 1025 (`arrive` words), 8192 | 8193 (length histogram); T 128 | 129 | 130 (chase maps and their chunk count); S 1 | 2,
63 | 64 | 65, 256 | 257, 2048 | 2049, 4096 | 4097 (small-state kernels, time-resident, 8-item tiles, the routes' limits), 2052
(a multiple of 4 above 2048: band route with 8-item tiles), 192 and 1440.  The decode query branches on T, so it keeps the whole
T axis at the batch sizes next to a T condition and two values elsewhere; the others are linear in T and keep one or two.
The band counts add B 511 | 512 | 513 (one plane per item up to 512 planes), sampling both values of `uniform` and the ends
of the range of draws (the size does not depend on them), and the band queries a reach of 300 / 5, which clamps at S - 1 for
every state count up to 257.
"""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, 'tests', 'golden', 'workspace_bytes.json')

BATCHES = (1, 3, 16, 17, 31, 32, 1024, 1025, 8192, 8193)
FRAMES = (1, 2, 128, 129, 130, 500)
STATES = (1, 2, 63, 64, 65, 192, 256, 257, 1440, 2048, 2049, 2052, 4096, 4097)
CAPACITIES = (1, 64)
RANKS = (1, 3, 32)
REACHES = ((0, 0), (10, 3), (87, 87))
WIDE = REACHES + ((300, 5),)
DRAWS = (1, 4096)


def grid():
    """function name -> list of argument tuples"""
    g = {}
    g['torbi_hip_workspace_bytes'] = [(B, T, S) for B in BATCHES for S in STATES
                                      for T in (FRAMES if B in (16, 8193) else (2, 130))]
    g['torbi_hip_preparation_bytes'] = [(S,) for S in STATES]
    g['torbi_hip_stream_state_bytes'] = [(B, S, c) for B in BATCHES for S in (1, 63, 257, 4097) for c in CAPACITIES]
    g['torbi_hip_forward_backward_workspace_bytes'] = (
        [(B, 129, S) for B in (1, 17, 32, 8193) for S in STATES] + [(17, 2, S) for S in STATES])
    g['torbi_hip_forward_backward_band_workspace_bytes'] = (
        [(B, 129, S, l, r) for B in (1, 17, 8193) for S in STATES for (l, r) in REACHES]
        + [(17, 2, S, 10, 3) for S in STATES])
    g['torbi_hip_k_best_workspace_bytes'] = (
        [(B, 130, S, k) for B in (1, 17, 8193) for S in STATES for k in RANKS]
        + [(B, 1, S, 3) for B in (1, 17, 8193) for S in STATES])
    # the queries that stand on the ones above: the counts (the layout of forward_backward), the band counts (planes behind the
    # band layout: one per item below 512 items, 512 from there on), band k-best (diagonals in place of the matrix, a verdict
    # word), sampling (filter rows behind forward_backward's layout or the band's; the uniform route's row sums alone) and
    # the streaming band route's diagonals.  WIDE holds reaches that clamp at S - 1 for the smaller state counts.
    g['torbi_hip_forward_backward_counts_workspace_bytes'] = (
        [(B, 129, S) for B in (1, 17, 32, 8193) for S in STATES] + [(17, 2, S) for S in STATES])
    g['torbi_hip_forward_backward_counts_band_workspace_bytes'] = (
        [(B, 129, S, l, r) for B in (1, 17, 511, 512, 513, 8193) for S in STATES for (l, r) in WIDE]
        + [(17, 2, S, 10, 3) for S in STATES])
    g['torbi_hip_k_best_band_workspace_bytes'] = (
        [(B, 130, S, k, l, r) for B in (1, 17, 8193) for S in STATES for k in RANKS for (l, r) in WIDE]
        + [(17, 1, S, 3, 10, 3) for S in STATES])
    g['torbi_hip_sample_workspace_bytes'] = (
        [(B, 129, S, N, u) for B in (1, 17, 32, 8193) for S in STATES for N in DRAWS for u in (0, 1)]
        + [(17, 2, S, 5, u) for S in STATES for u in (0, 1)])
    g['torbi_hip_sample_band_workspace_bytes'] = (
        [(B, 129, S, N, l, r) for B in (1, 17, 8193) for S in STATES for N in DRAWS for (l, r) in WIDE]
        + [(17, 2, S, 5, 10, 3) for S in STATES])
    g['torbi_hip_stream_band_diagonals_bytes'] = [(S, l, r) for S in STATES for (l, r) in WIDE]
    return g


def main():
    from torbi_amd import _lib
    lib = _lib.load()
    units = lib.torbi_hip_compute_units(0) if lib.torbi_hip_device_count() > 0 else 256
    commit = subprocess.check_output(['git', 'rev-parse', 'HEAD'], cwd=ROOT, text=True).strip()
    lines = ['{', f' "commit": "{commit}",', f' "compute_units": {units},']
    total = 0
    names = list(grid().items())
    for n, (name, cases) in enumerate(names):
        rows = [json.dumps(list(args) + [int(getattr(lib, name)(*args))]) for args in cases]
        total += len(rows)
        lines.append(f' "{name}": [\n  ' + ',\n  '.join(rows) + '\n ]' + (',' if n + 1 < len(names) else ''))
    lines.append('}')
    with open(OUT, 'w') as f:
        f.write('\n'.join(lines) + '\n')
    json.load(open(OUT))
    print(f'wrote {total} entries of commit {commit[:7]} ({units} compute units) to {OUT}')


if __name__ == '__main__':
    main()
