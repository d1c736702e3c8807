"""Measure path statistics (torbi_amd.paths.path_statistics, PATHS.md) on one MI355X; prints one JSON line.

At B x K x T x S (512 x {1, 16} x 500 x 1440 by default) under the pitch band matrix (synth.banded_transition(S, 88,
tiny=True): 175 diagonals, log(tiny) outside), with a caller-owned workspace, every time from hipEvents on the stream around
one call, after a warm-up call, as median / min / max of --repeats calls, for three kinds of paths:

  decoded / sampled   the decoder's own path (K = 1) or `sample_paths` draws (K > 1) of the synthetic observations under that
           matrix (random observations: the paths move at almost every frame)
  random   uniformly random states: no two adds of a path meet
  runs     notes held for --run frames, every path of the batch within the same 64 states: the contended case of the
           float64 atomics (B K (T - 1) adds on a few thousand cells, most of them on 64)

  * path_statistics scores only, counts only (no model), and both
  * the same statistics with torch ops in this process, on the same inputs: the T-step float32 gather-and-add loop (its
    scores are asserted equal to the kernel's bit for bit before it is timed) and `index_put_(accumulate=True)` on float64
    (its counts asserted equal)
  * with K = 1: `viterbi_counts` against `from_probabilities` alone and against `expected_counts` on the same inputs
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torbi_amd  # noqa: E402
from torbi_amd import paths, synth  # noqa: E402


def spread(values):
    v = sorted(values)
    return {'median': float(np.median(v)), 'min': float(v[0]), 'max': float(v[-1]), 'runs': len(v)}


def timed(fn, repeats):
    """ms of `fn` between two events on the current stream, after one warm-up call."""
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(repeats):
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        fn()
        end.record()
        end.synchronize()
        out.append(start.elapsed_time(end))
    return spread(out)


def torch_scores(obs, trans, init, q):
    """The chain with torch ops: one gather-and-add step per frame (every item has all T frames, every index is valid)."""
    T = q.shape[2]
    q = q.long()
    s = obs[:, 0].gather(1, q[:, :, 0]) + init[q[:, :, 0]]
    for t in range(1, T):
        s = obs[:, t].gather(1, q[:, :, t]) + (s + trans[q[:, :, t], q[:, :, t - 1]])
    return s


def torch_counts(q, S):
    """The unweighted counts with index_put_(accumulate=True) on float64, rounded once."""
    q = q.long()
    one = torch.ones((), dtype=torch.float64, device=q.device)
    X = torch.zeros((S * S,), dtype=torch.float64, device=q.device)
    cell = (q[:, :, 1:] * S + q[:, :, :-1]).reshape(-1)
    X.index_put_((cell,), one.expand(cell.numel()), accumulate=True)
    first = q[:, :, 0].reshape(-1)
    I = torch.zeros((S,), dtype=torch.float64, device=q.device).index_put_((first,), one.expand(first.numel()), accumulate=True)
    return X.view(S, S).float(), I.float()


def bits_equal(a, b):
    return bool((a.contiguous().view(torch.int32) == b.contiguous().view(torch.int32)).all())


def rows_for(kind, q, obs, frames, trans, init, ws, repeats, torch_repeats):
    B, K, T = q.shape
    S = obs.shape[2]
    row = {'paths': kind, 'K': K,
           'distinct_cells_per_path': float(np.mean([(q[b, 0, 1:].long() * S + q[b, 0, :-1]).unique().numel()
                                                     for b in range(min(B, 8))]))}
    row['scores_ms'] = timed(lambda: paths.path_statistics(obs, frames, trans, init, q, counts=False), repeats)
    row['counts_ms'] = timed(lambda: paths.count_paths(q, S, frames), repeats)      # (its 16.6 MB workspace from torch's cache)
    row['both_ms'] = timed(lambda: paths.path_statistics(obs, frames, trans, init, q, workspace=ws), repeats)
    got = paths.path_statistics(obs, frames, trans, init, q, workspace=ws)
    want_s, want_c = torch_scores(obs, trans, init, q), torch_counts(q, S)
    assert bits_equal(got[0], want_s), 'the torch loop gives other score bits'
    assert torch.equal(got[1], want_c[0]) and torch.equal(got[2], want_c[1]), 'index_put_ gives other counts'
    assert float(got[1].double().sum()) == B * K * (T - 1) and float(got[2].double().sum()) == B * K
    row['torch_scores_ms'] = timed(lambda: torch_scores(obs, trans, init, q), torch_repeats)
    row['torch_counts_ms'] = timed(lambda: torch_counts(q, S), torch_repeats)
    row['scores_speedup'] = row['torch_scores_ms']['median'] / row['scores_ms']['median']
    row['counts_speedup'] = row['torch_counts_ms']['median'] / row['counts_ms']['median']
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--B', type=int, default=512)
    ap.add_argument('--T', type=int, default=500)
    ap.add_argument('--S', type=int, default=1440)
    ap.add_argument('--K', type=int, nargs='+', default=[1, 16])
    ap.add_argument('--half-width', type=int, default=88)
    ap.add_argument('--run', type=int, default=40, help="frames a note is held in the 'runs' paths")
    ap.add_argument('--repeats', type=int, default=7)
    ap.add_argument('--torch-repeats', type=int, default=3)
    ap.add_argument('--skip-training', action='store_true', help='leave out viterbi_counts / from_probabilities / expected_counts')
    args = ap.parse_args()
    B, T, S = args.B, args.T, args.S
    dev = torch.device('cuda:0')
    obs, _, init = (torch.from_numpy(x).to(dev) for x in synth.problem(B, T, S, seed=1))
    trans = torch.from_numpy(synth.banded_transition(S, args.half_width, tiny=True)).to(dev)
    frames = torch.full((B,), T, dtype=torch.int32, device=dev)
    out = {'device': torch.cuda.get_device_name(0), 'shape': [B, T, S], 'diagonals': 2 * args.half_width - 1, 'rows': []}
    for K in args.K:
        ws = torch.empty(paths.path_statistics_workspace_bytes(B, T, S, K), dtype=torch.uint8, device=dev)
        out['workspace_bytes'] = ws.numel()
        if K == 1:
            held = torbi_amd.decode(obs, frames, trans, init)[:, None, :].contiguous()
        else:
            held = torbi_amd.sample_paths(obs, K, frames, trans, init, log_probs=True, gpu=0, route='auto',
                                          generator=torch.Generator(device=dev).manual_seed(1))[0]
            assert int(held.min()) >= 0
        rand = torch.randint(0, S, (B, K, T), dtype=torch.int32, device=dev, generator=torch.Generator(device=dev).manual_seed(2))
        # notes held for --run frames, every path within 64 states: runs of equal (q_t, q_{t-1}) inside a chunk, and the paths
        # of the whole batch on the same few cells
        g = torch.Generator(device=dev).manual_seed(3)
        notes = torch.randint(S // 2, S // 2 + 64, (B, K, (T + args.run - 1) // args.run), dtype=torch.int32, device=dev, generator=g)
        runs = notes.repeat_interleave(args.run, dim=2)[:, :, :T].contiguous()
        for kind, q in (('decoded' if K == 1 else 'sampled', held), ('random', rand), ('runs', runs)):
            out['rows'].append(rows_for(kind, q, obs, frames, trans, init, ws, args.repeats, args.torch_repeats))
        del ws, held, rand, runs, notes
    if not args.skip_training:
        model = dict(batch_frames=frames, transition=trans, initial=init, log_probs=True, gpu=0)
        out['training'] = {
            'from_probabilities_ms': timed(lambda: torbi_amd.from_probabilities(obs.clone(), **model), args.repeats),
            'viterbi_counts_ms': timed(lambda: paths.viterbi_counts(obs, **model), args.repeats),
            'expected_counts_ms': timed(lambda: torbi_amd.expected_counts(obs, **model), args.torch_repeats),
            'observation_clone_ms': timed(lambda: obs.clone(), args.repeats),
        }
    print(json.dumps(out))


if __name__ == '__main__':
    main()
