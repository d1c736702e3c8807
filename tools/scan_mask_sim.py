"""CPU simulation of the pruned scan's closed-row mask (csrc/resident_forward.hpp, kMask): how much of a wave pass's posterior reads belongs to
rows that are already closed.

Built on scan_horizon_sim.pass_depths (the exact recurrence on one tile of 16 items; per wave pass -- 16 next-states x 16
items -- which pairs each termination test finds closed).  A pass walks max(1, previous walk - slack) blocks before its first
evaluated test and tests behind every block from there on; a row (the lane quad of one next-state) is closed once a test
finds all 16 of its items closed, rows past the last state from the first test on.  For every slack:
  * the share of the (quad, block) posterior reads of a pass that belong to rows closed at an earlier test of that pass --
    what the mask takes off the LDS,
  * the share of the 16-lane phases of those reads (four quads: next-states LANE_ROW[4k .. 4k + 3] of the row group, the
    kernel's lane order) in which no quad is open,
  * blocks walked per pass.
Three kinds of rows, as scan_horizon_sim: the benchmark's, peaked rows with the dense matrix, peaked rows with the banded
pitch matrix.

    python tools/scan_mask_sim.py [--states 1440] [--frames 13] [--skip 2] [--seeds 1] > profiles/scan_mask_sim.txt
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from torbi_amd import synth  # noqa: E402
from scan_horizon_sim import ITEMS, ROWS, pass_depths, peaked_rows  # noqa: E402

# next-state (within its row group) of lane quad q = lane >> 2: the nibbles of 0xFBAE9DC873261540, lowest first
LANE_ROW = [(0xFBAE9DC873261540 >> (4 * q)) & 15 for q in range(16)]
PHASES = np.array(LANE_ROW).reshape(4, 4)       # a ds_read_b128 goes through the LDS 16 lanes = 4 quads at a time


def masked_reads(closed, depth, slack):
    """(reads, reads of closed rows, phases, phases without an open quad, blocks walked, passes) with a horizon of `slack`."""
    T1, nrg = depth.shape
    reads = shut = phases = empty = walked = 0
    prev = depth[0].copy()
    for t in range(1, T1):          # (the first timestep kept only sets the horizons, as in scan_horizon_sim.report)
        first = np.maximum(1, prev - slack)
        walk = np.maximum(first, depth[t])
        for rg in range(nrg):
            rows_closed = closed[t][:, rg].all(axis=0)          # (ROWS, tests): every item of the row closed at test n
            reads += ROWS * walk[rg]
            phases += len(PHASES) * walk[rg]
            for n in range(first[rg], walk[rg]):                # block n + 1 runs under the mask of the test behind block n
                row = rows_closed[:, n - 1]
                shut += row.sum()
                empty += row[PHASES].all(axis=1).sum()
        walked += walk.sum()
        prev = walk
    return reads, shut, phases, empty, walked, (T1 - 1) * nrg


def report(name, obs, trans, init, KR, slacks, skip):
    closed, depth = pass_depths(obs, trans, init, KR)
    closed, depth = closed[skip:], depth[skip:]
    print(f'== {name}: {trans.shape[0]} states, {depth.shape[0] - 1} timesteps x {depth.shape[1]} row groups, {KR} seed(s) per item')
    for slack in slacks:
        reads, shut, phases, empty, walked, passes = masked_reads(closed, depth, slack)
        print(f'slack {slack}: reads for closed rows {100 * shut / reads:.1f} % of {reads} (quad, block) reads, '
              f'phases with no open quad {100 * empty / phases:.1f} %, blocks walked {walked / passes:.2f} a pass')


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--states', type=int, default=1440)
    ap.add_argument('--frames', type=int, default=13, help='timesteps 1 .. frames - 1 are simulated')
    ap.add_argument('--seeds', type=int, default=1, help='explicit candidates per item (KR of the kernel instance)')
    ap.add_argument('--skip', type=int, default=2, help='timesteps left out in front (the transient behind row 0)')
    ap.add_argument('--slacks', type=int, nargs='+', default=[2, 3, 4])
    ap.add_argument('--half-width', type=float, default=87.2, help='of the banded pitch matrix')
    args = ap.parse_args()
    S, T = args.states, args.frames
    obs, trans, init = synth.problem(ITEMS, T, S, seed=0)
    report('benchmark rows, dense matrix', obs, trans, init, args.seeds, args.slacks, args.skip)
    peaks = peaked_rows(T, S, seed=1)
    report('peaked rows, dense matrix', peaks, trans, init, args.seeds, args.slacks, args.skip)
    band = synth.banded_transition(S, args.half_width)
    report('peaked rows, banded pitch matrix', peaks, band, np.full(S, -np.log(S), np.float32), args.seeds, args.slacks, args.skip)


if __name__ == '__main__':
    main()
