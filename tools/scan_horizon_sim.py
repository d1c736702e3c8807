"""CPU simulation of the pruned scan's termination tests (csrc/resident_forward.hpp): which of them decide anything.

One tile of 16 items runs the exact recurrence for a few timesteps; for every wave pass (a row group of 16 next-states x 16
items, 256 pairs in lock step) it records after how many 16-entry list blocks the kernel's bound closes every pair, and from
that
  * the distribution of blocks per wave pass and of the change of a row group's depth from one timestep to the next,
  * the share of the termination tests that ONE item slot settles (slot = item nblk & 3 of every lane: items it, it + 4,
    it + 8, it + 12 of the sixteen rows, 64 pairs): some pair of the slot is open, the wave goes on whatever the rest say,
  * for a test horizon of max(1, previous walk - slack) blocks: blocks walked past the lock-step depth (overshoot), tests left.
Three kinds of rows: the benchmark's (synth.problem, dense matrix), peaked rows with the dense matrix, peaked rows with the
banded pitch matrix (scans two or three blocks deep: the horizon must cost nothing there).

    python tools/scan_horizon_sim.py [--states 1440] [--frames 9] [--skip 2] [--seeds 1] > profiles/scan_horizon_sim.txt
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from torbi_amd import synth  # noqa: E402

BLK, ITEMS, ROWS = 16, 16, 16


def peaked_rows(T, S, seed, width=12.0, step=20):
    """log-softmax rows with one peak whose centre wanders by up to `step` states a frame."""
    rng = np.random.default_rng(seed)
    centre = np.clip(np.cumsum(rng.integers(-step, step + 1, size=(ITEMS, T)), axis=1) + rng.integers(0, S, size=(ITEMS, 1)), 0, S - 1)
    logits = rng.standard_normal((ITEMS, T, S)).astype(np.float32) * 2
    logits -= (np.abs(np.arange(S)[None, None, :] - centre[:, :, None]).astype(np.float32) / np.float32(width)) ** 2
    m = logits.max(2, keepdims=True)
    lse = m + np.log(np.exp(logits - m).sum(2, keepdims=True))
    return np.maximum(logits - lse, np.log(np.finfo(np.float32).tiny)).astype(np.float32)


def pass_depths(obs, trans, init, KR):
    """closed[t - 1][rg] = (tests, ITEMS, ROWS) bool per row group: test n (behind block n + 1) finds the pair closed; and the
    lock-step depth of every wave pass, [T - 1][row groups]."""
    S = trans.shape[0]
    Sp = (S + BLK - 1) // BLK * BLK
    nb = Sp // BLK
    order = np.argsort(-trans, axis=1, kind='stable')
    ts = np.full((S, Sp), -np.inf, np.float32)
    ts[:, :S] = np.take_along_axis(trans, order, axis=1)
    order = np.concatenate([order, np.zeros((S, Sp - S), order.dtype)], axis=1)
    head = np.concatenate([ts[:, BLK::BLK], np.full((S, 1), -np.inf, np.float32)], axis=1)      # (S, nb): first entry of block n + 1
    nrg = (S + ROWS - 1) // ROWS
    post = (obs[:, 0] + init[None, :]).astype(np.float32)
    closed_all, depth_all = [], []
    with np.errstate(invalid='ignore'):
        for t in range(1, obs.shape[1]):
            srt = np.argsort(-post, axis=1, kind='stable')
            nxt = np.empty_like(post)
            closed = np.zeros((ITEMS, S, nb), bool)
            for b in range(ITEMS):
                p = post[b]
                seeds, thr = srt[b, :KR], p[srt[b, KR]]
                best0 = (p[seeds][None, :] + trans[:, seeds]).max(1) if KR else np.full(S, -np.inf, np.float32)
                cand = (p[order] + ts).reshape(S, nb, BLK).max(2)                   # block maxima, (S, nb)
                run = np.maximum(np.maximum.accumulate(cand, axis=1), best0[:, None])
                closed[b] = ~(head + thr > run)
                closed[b, :, nb - 1] = True                                         # the list ends
                nxt[b] = obs[b, t] + run[:, nb - 1]
            depth = closed.argmax(axis=2) + 1                                       # (ITEMS, S) blocks a pair needs
            pad = nrg * ROWS - S
            depth = np.concatenate([depth, np.ones((ITEMS, pad), depth.dtype)], axis=1)
            closed = np.concatenate([closed, np.ones((ITEMS, pad, nb), bool)], axis=1)
            closed_all.append(closed.reshape(ITEMS, nrg, ROWS, nb))
            depth_all.append(depth.reshape(ITEMS, nrg, ROWS).max(axis=(0, 2)))
            post = nxt
    return closed_all, np.array(depth_all)


def report(name, obs, trans, init, KR, slacks, skip):
    closed, depth = pass_depths(obs, trans, init, KR)
    closed, depth = closed[skip:], depth[skip:]       # (row 0 is observation + initial: the first scans run deeper)
    T1, nrg = depth.shape
    nb = closed[0].shape[3]
    print(f'== {name}: {trans.shape[0]} states, {nb} blocks a row, {T1} timesteps (from {skip + 1}) x {nrg} row groups = {T1 * nrg} wave passes, '
          f'{KR} seed(s) per item')
    hist = np.bincount(depth.ravel(), minlength=nb + 1)
    print(f'blocks per wave pass: mean {depth.mean():.2f}, min {depth.min()}, max {depth.max()};  '
          + ' '.join(f'{d}:{n}' for d, n in enumerate(hist) if n))
    if T1 > 1:
        change = (depth[1:] - depth[:-1]).ravel()
        lo, hi = change.min(), change.max()
        print('change of a row group\'s depth, timestep to timestep: '
              + ' '.join(f'{c:+d}:{n}' for c, n in zip(range(lo, hi + 1), np.bincount(change - lo)) if n))

    def slot_settles(t, rg, n):
        """test behind block n of pass (t, rg): is a pair of item slot n & 3 still open?"""
        return not closed[t][(n & 3)::4, rg, :, n - 1].all()

    # the shipped scan: a full test behind every block
    tests = settled = 0
    for t in range(T1):
        for rg in range(nrg):
            for n in range(1, depth[t, rg] + 1):
                tests += 1
                settled += slot_settles(t, rg, n)
    print(f'test behind every block: {tests} tests, {tests / depth.size:.2f} a pass; one slot settles {settled} '
          f'({100 * settled / tests:.1f} %), the full test is needed {(tests - settled) / depth.size:.2f} times a pass')
    # (the horizon starts at 1 at the first timestep kept, as the kernel's does at t = 1; that timestep, whose every test is
    # evaluated, is left out of the sums: the launch has hundreds of timesteps behind it)
    for slack in slacks:
        prev = depth[0].copy()
        walked = tests = settled = 0
        for t in range(1, T1):
            first = np.maximum(1, prev - slack)
            walk = np.maximum(first, depth[t])
            for rg in range(nrg):
                for n in range(first[rg], walk[rg] + 1):
                    tests += 1
                    settled += slot_settles(t, rg, n)
            walked += walk.sum()
            prev = walk
        over = walked - depth[1:].sum()
        print(f'horizon, slack {slack}: blocks walked {walked} ({100 * over / walked:.2f} % overshoot), tests {tests / depth[1:].size:.2f} a pass, '
              f'one slot settles {100 * settled / tests:.1f} % of them, full tests {(tests - settled) / depth[1:].size:.2f} a pass')


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--states', type=int, default=1440)
    ap.add_argument('--frames', type=int, default=9, help='timesteps 1 .. frames - 1 are simulated')
    ap.add_argument('--seeds', type=int, default=1, help='explicit candidates per item (KR of the kernel instance)')
    ap.add_argument('--skip', type=int, default=2, help='timesteps left out in front (the transient behind row 0)')
    ap.add_argument('--slacks', type=int, nargs='+', default=[0, 1, 2, 3, 4])
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
