"""Measure path entropy (torbi_amd.entropy.forward_entropy, ENTROPY.md) on one MI355X; prints one JSON line.

At every B x T x S of --shapes (512 x 500 x 1440 and 1 x 500 x 1440 by default), with a caller-owned workspace, every time
from hipEvents on the stream around one call, after a warm-up call, as median / min / max of --repeats calls:

  (a) the dense route on a dense random matrix (synth.problem)
  (b) the uniform route (transition=None): the algorithmic bytes -- the observation read once, 4 B T S -- over the time, as a
      fraction of the HBM peak

and in the same process on the same inputs:

  * the comparator: the same recursion with torch ops in float32 (three matrix products per frame); its entropy is asserted
    equal to the kernel's within the bound of tests/test_path_entropy_gpu.py before it is timed
  * the yardstick: torbi_amd.forward_backward (one product per frame in each of two passes)

and, measured but asserted nowhere, the error against the float64 host route on a deliberately mismatched input: softmax rows
of scale 12 whose peak jumps anywhere among the states, under the -inf pitch band of 23 diagonals, where the filtered
distribution underflows float32 (--mismatched-items items, 0 to skip).

With --band, the band rows alone (ENTROPY.md, "Band route"): entropy.forward_entropy_banded against the dense route on the
same inputs in the same process, for the pitch band of --half-widths (12: 23 diagonals, 88: 175) in both forms of its
background (-inf and log(tiny)) at every batch of --batches, by the same method.  A band the band route does not cover (175
diagonals: beyond its window of 64 entries) has a dense time and no band time.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torbi_amd  # noqa: E402
from torbi_amd import entropy, synth  # noqa: E402

HBM_PEAK_BYTES = 8e12
RTOL_H, ATOL_H_PER_FRAME = 2e-5, 2e-5          # tests/test_path_entropy_gpu.py


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


def torch_entropy(obs, trans, init):
    """The recursion with torch ops in float32 (every item has all T frames): (H, L)."""
    B, T, S = obs.shape
    E = torch.exp(trans)
    G = torch.where(trans == -torch.inf, torch.zeros_like(E), E * trans)
    Et, Gt = E.t().contiguous(), G.t().contiguous()
    x = obs[:, 0] + init
    m = x.amax(dim=1, keepdim=True)
    a = torch.exp(x - m)
    h = torch.zeros_like(a)
    L = torch.zeros((B,), dtype=torch.float64, device=obs.device)
    for t in range(T):
        if t > 0:
            d = p @ Et
            h = torch.where(d == 0, torch.zeros_like(d), torch.log(d) + (u @ Et - p @ Gt) / d)
            m = obs[:, t].amax(dim=1, keepdim=True)
            a = torch.exp(obs[:, t] - m) * d
        c = a.sum(dim=1, keepdim=True)
        p = a / c
        u = p * h - torch.where(p > 0, p * torch.log(p), torch.zeros_like(p))
        L += (torch.log(c) + m)[:, 0].double()
    return u.double().sum(dim=1).float(), L.float()


def mismatched(items, T, S):
    """Worst error against the float64 host route where float32 underflows: rows of scale 12 under a -inf band."""
    dev = torch.device('cuda:0')
    g = torch.Generator().manual_seed(5)
    obs = torch.log_softmax(12 * torch.randn(items, T, S, generator=g), 2)
    trans = torch.from_numpy(synth.banded_transition(S, 12))
    init = torch.log_softmax(torch.randn(S, generator=g), 0)
    frames = torch.full((items,), T, dtype=torch.int32)
    H, L, _ = entropy._host(obs, frames, trans, None, init)
    got = entropy.forward_entropy(obs.to(dev), frames.to(dev), trans.to(dev), init.to(dev))
    h, l = (x.double().cpu() for x in got)
    ok = torch.isfinite(H) & torch.isfinite(h)
    return {'items': items, 'frames_states': [T, S], 'diagonals': 23, 'scale': 12,
            'items_finite_in_both': int(ok.sum()), 'items_finite_in_float64': int(torch.isfinite(H).sum()),
            'worst_relative_error_of_H': float(((h - H).abs() / H.abs().clamp_min(1e-30))[ok].max()) if ok.any() else None,
            'worst_absolute_error_of_H': float((h - H).abs()[ok].max()) if ok.any() else None,
            'worst_absolute_error_of_L': float((l - L).abs()[ok].max()) if ok.any() else None,
            'entropy_float64_min_max': [float(H[ok].min()), float(H[ok].max())] if ok.any() else None}


def shape_rows(B, T, S, repeats, torch_repeats):
    dev = torch.device('cuda:0')
    obs, trans, init = (torch.from_numpy(x).to(dev) for x in synth.problem(B, T, S, seed=1))
    frames = torch.full((B,), T, dtype=torch.int32, device=dev)
    ws = torch.empty(entropy.path_entropy_workspace_bytes(B, T, S), dtype=torch.uint8, device=dev)
    out = {'shape': [B, T, S], 'workspace_bytes': ws.numel(),
           'uniform_workspace_bytes': entropy.path_entropy_workspace_bytes(B, T, S, uniform=True)}
    a = timed(lambda: entropy.forward_entropy(obs, frames, trans, init, workspace=ws), repeats)
    out['a_dense'] = {'ms': a, 'us_per_frame': 1e3 * a['median'] / T,
                      'flops_per_s': 3 * 2.0 * B * (T - 1) * S * S / (a['median'] * 1e-3)}
    b = timed(lambda: entropy.forward_entropy(obs, frames, None, init, workspace=ws), repeats)
    moved = 4.0 * B * T * S
    out['b_uniform'] = {'ms': b, 'gbps': moved / b['median'] / 1e6,
                        'fraction_of_hbm_peak': moved / (b['median'] * 1e-3) / HBM_PEAK_BYTES}

    got = entropy.forward_entropy(obs, frames, trans, init, workspace=ws)
    want = torch_entropy(obs, trans, init)
    error = (got[0].double() - want[0].double()).abs()
    bound = RTOL_H * want[0].double().abs() + ATOL_H_PER_FRAME * T
    assert bool((error <= bound).all()), ('the torch formulation and the kernel disagree', float(error.max()))
    ref = timed(lambda: torch_entropy(obs, trans, init), torch_repeats)
    out['torch_ops'] = {'ms': ref, 'worst_difference_of_H': float(error.max()), 'entropy_min_max': [float(got[0].min()), float(got[0].max())],
                        'speedup_of_a': ref['median'] / a['median']}

    fws = torch.empty(torbi_amd.forward_backward_workspace_bytes(B, T, S), dtype=torch.uint8, device=dev)
    f = timed(lambda: torbi_amd.forward_backward(obs, frames, trans, init, workspace=fws), repeats)
    post, L = torbi_amd.forward_backward(obs, frames, trans, init, workspace=fws)
    out['forward_backward'] = {'ms': f, 'a_over_this': a['median'] / f['median'],
                               'worst_difference_of_L': float((L.double() - got[1].double()).abs().max())}
    return out


def band_rows(T, S, repeats, batches, half_widths):
    """The band route (entropy.forward_entropy_banded) against the dense route on the same inputs in the same process: the
    pitch band of `half_width` (2 * half_width - 1 diagonals) in both forms of its background, -inf and log(tiny), at every
    batch of `batches`.  `wins`: the dense median exceeds the band median by more than the dense route's own spread
    (max - min); `difference_in_units`: the worst |H_band - H_dense| and the same for the prefix entries in units of
    1e-6 |H| + 1e-6 F (each route is within 20 units of float64 on the test shapes)."""
    dev = torch.device('cuda:0')
    rows = []
    for B in batches:
        obs, _, init = (torch.from_numpy(x).to(dev) for x in synth.problem(B, T, S, seed=1))
        frames = torch.full((B,), T, dtype=torch.int32, device=dev)
        dense_ws = torch.empty(entropy.path_entropy_workspace_bytes(B, T, S), dtype=torch.uint8, device=dev)
        upto = torch.arange(1, T + 1, dtype=torch.float64, device=dev)[None, :]
        for half_width in half_widths:
            reach = half_width - 1
            for tiny in (False, True):
                matrix = synth.banded_transition(S, half_width, tiny=tiny)
                background = float(matrix[0, S - 1])
                trans = torch.from_numpy(matrix).to(dev)
                dense = timed(lambda: entropy.forward_entropy(obs, frames, trans, init, workspace=dense_ws), repeats)
                row = {'batch': B, 'diagonals': 2 * reach + 1, 'background': background, 'dense_ms': dense,
                       'covered': bool(entropy._covered(B, T, S, reach, reach, background))}
                rows.append(row)
                if not row['covered']:
                    continue
                band_ws = torch.empty(entropy.path_entropy_banded_workspace_bytes(B, T, S, reach, reach), dtype=torch.uint8,
                                      device=dev)
                run = lambda prefix=False: entropy.forward_entropy_banded(obs, frames, trans, init, reach, reach, background,
                                                                          workspace=band_ws, prefix=prefix)
                band = timed(run, repeats)
                want = [x.double() for x in entropy.forward_entropy(obs, frames, trans, init, workspace=dense_ws, prefix=True)]
                got = [x.double() for x in run(prefix=True)]
                units = lambda g, w, f: float(((g - w).abs() / (1e-6 * w.abs() + 1e-6 * f)).max())
                row.update({'band_ms': band, 'speedup': dense['median'] / band['median'],
                            'wins': dense['median'] - band['median'] > dense['max'] - dense['min'],
                            'difference_in_units': [units(got[0], want[0], T), units(got[2], want[2], upto)],
                            'worst_difference_of_L': float((got[1] - want[1]).abs().max()),
                            'nan_values': int(sum(torch.isnan(x).sum() for x in got)),
                            'entropy_min_max': [float(want[0].min()), float(want[0].max())],
                            'band_workspace_bytes': band_ws.numel()})
                del want, got
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--band', action='store_true', help='the band rows alone (ENTROPY.md, "Band route")')
    ap.add_argument('--batches', type=int, nargs='+', default=[1, 8, 512])
    ap.add_argument('--half-widths', type=int, nargs='+', default=[12, 88])
    ap.add_argument('--shapes', type=int, nargs=3, action='append', metavar=('B', 'T', 'S'))
    ap.add_argument('--repeats', type=int, default=7)
    ap.add_argument('--torch-repeats', type=int, default=3)
    ap.add_argument('--mismatched-items', type=int, default=8)
    ap.add_argument('--out', default=None, help='also write the JSON here')
    args = ap.parse_args()
    if args.band:
        T, S = (args.shapes or [[0, 500, 1440]])[0][1:]
        out = {'device': torch.cuda.get_device_name(0), 'frames_states': [T, S], 'repeats': args.repeats,
               'band_rows': band_rows(T, S, args.repeats, args.batches, args.half_widths)}
    else:
        shapes = args.shapes or [[512, 500, 1440], [1, 500, 1440]]
        out = {'device': torch.cuda.get_device_name(0), 'repeats': args.repeats,
               'shapes': [shape_rows(B, T, S, args.repeats, args.torch_repeats) for B, T, S in shapes]}
        if args.mismatched_items:
            out['mismatched'] = mismatched(args.mismatched_items, 500, 1440)
    text = json.dumps(out)
    if args.out:
        with open(args.out, 'w') as fh:
            fh.write(text + '\n')
    print(text)


if __name__ == '__main__':
    main()
