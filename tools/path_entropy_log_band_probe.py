"""Measure the log-space band route of path entropy (entropy.forward_entropy_log_banded) on one MI355X; prints one JSON line
per case.

  --errors   per case of tests/test_path_entropy_log_band_gpu.py and on mismatched inputs (tools/posterior_log_band_probe.py
             mismatched) at 8 x 500 x 1440 on 23 diagonals, -inf outside: the worst error of H, of every prefix entry and of L
             against the test file's float64 log-space reference, run on the device, absolute and as a share of the bounds
             4e-5 |ref| + 4e-5 F and 1e-6 |ref| + 4e-6 F -- for this route and, on the same inputs, for the scaled routes
             forward_entropy_wide_banded and (where the band has at most 64 entries) forward_entropy_banded: the contrast
             table of ENTROPY.md.  A NaN where the reference is finite counts as an infinite error.
  (default)  time at B x T x 1440 on 23 and 175 diagonals, -inf outside, peaked rows: this route with the library's tile and
             with every tile forced (TORBI_HIP_LOG_BAND_ITEMS), the scaled route of the same band (narrow or wide) and
             forward_backward_log_banded (both passes of the same forward rows), alternated call by call in one process with
             caller-owned workspaces and device events: median, min and max of --repeats calls.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, 'tools'), os.path.join(ROOT, 'tests'), ROOT]
import torbi_amd  # noqa: E402
from torbi_amd import _lib, entropy, synth  # noqa: E402
from posterior_log_band_probe import forced, mismatched  # noqa: E402
from posterior_probe import peaked_rows  # noqa: E402
from posterior_wide_band_probe import alternated  # noqa: E402

DEV = torch.device('cuda:0')
NINF = float('-inf')


def worst(got, want, frames):
    """{'H' | 'prefix' | 'L': (largest absolute error, largest share of its bound)} of one route's (H, L, prefix)."""
    T = got[2].shape[1]
    F = frames.cpu().long().clamp(1, T)
    steps = torch.arange(1, T + 1, dtype=torch.float64)[None, :].expand_as(want[2])
    out = {}
    for name, g, w, scale, per_frame, n in (('H', got[0], want[0], 4e-5, 4e-5, F), ('L', got[1], want[1], 1e-6, 4e-6, F),
                                            ('prefix', got[2], want[2], 4e-5, 4e-5, steps)):
        d = torch.nan_to_num((g.cpu().double() - w).abs(), nan=float('inf'))
        show = lambda x: float(x) if np.isfinite(float(x)) else str(float(x))
        out[name] = {'abs': show(d.max()), 'share': show((d / (scale * w.abs() + per_frame * n)).max())}
    return out


def errors(name, obs, frames, trans, init, left, right):
    import test_path_entropy_log_band_gpu as cases
    want = cases.log_space(obs, frames, trans, init)
    B, T, S = obs.shape
    out = {'case': name, 'shape': [B, T, S], 'reach': [left, right], 'H_reference': [float(x) for x in want[0][:4]]}
    routes = {'log': entropy.forward_entropy_log_banded, 'wide': entropy.forward_entropy_wide_banded}
    if min(left, S - 1) + min(right, S - 1) + 1 <= 64:
        routes['narrow'] = entropy.forward_entropy_banded
    for route, fn in routes.items():
        out[route] = worst(fn(obs, frames, trans, init, left, right, NINF, prefix=True), want, frames)
    return out


def timing(B, T, S, half_width, repeats):
    reach = half_width - 1
    trans = torch.from_numpy(synth.banded_transition(S, half_width)).to(DEV)
    init = torch.full((S,), float(np.log(1. / S)), device=DEV)
    obs = peaked_rows(B, T, S, DEV)
    frames = torch.full((B,), T, dtype=torch.int32, device=DEV)
    narrow = 2 * reach + 1 <= 64
    scaled = entropy.forward_entropy_banded if narrow else entropy.forward_entropy_wide_banded
    size = entropy.path_entropy_banded_workspace_bytes if narrow else entropy.path_entropy_wide_banded_workspace_bytes
    ws = {name: torch.empty(need(B, T, S, reach, reach), dtype=torch.uint8, device=DEV) for name, need in
          (('entropy_log', entropy.path_entropy_log_banded_workspace_bytes), ('entropy_scaled', size),
           ('posterior_log', torbi_amd.forward_backward_log_banded_workspace_bytes))}
    run = lambda fn, name: lambda: fn(obs, frames, trans, init, reach, reach, workspace=ws[name])
    calls = {'entropy_log': run(entropy.forward_entropy_log_banded, 'entropy_log'),
             'entropy_scaled': run(scaled, 'entropy_scaled'),
             'posterior_log': run(torbi_amd.forward_backward_log_banded, 'posterior_log')}
    calls.update({f'entropy_log_G{G}': forced(G, calls['entropy_log']) for G in (1, 2)})
    return {'shape': [B, T, S], 'diagonals': 2 * reach + 1, 'scaled_route': 'narrow' if narrow else 'wide',
            'chosen_G': _lib.load().torbi_hip_path_entropy_log_band_tile(B, S, reach, reach, 0), 'ms': alternated(calls, repeats)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--errors', action='store_true')
    ap.add_argument('--repeats', type=int, default=7)
    ap.add_argument('--T', type=int, default=500)
    ap.add_argument('--batches', type=int, nargs='+', default=[1, 8, 64, 512, 4096])
    args = ap.parse_args()
    print(json.dumps({'device': torch.cuda.get_device_name(0)}), flush=True)
    if args.errors:
        import test_path_entropy_log_band_gpu as cases
        for case in cases.MODERATE + cases.WIDE:
            print(json.dumps(errors('-'.join(map(str, case)), *cases.problem(case), *case[-2:])), flush=True)
        obs, frames, trans, init, left, right, _ = mismatched(8, 500, 1440, 12, False)
        obs, frames, trans, init = (torch.as_tensor(np.array(a)).to(DEV) for a in (obs, frames, trans, init))
        print(json.dumps(errors('mismatched', obs, frames, trans, init, left, right)), flush=True)
        return
    for B in args.batches:
        for half_width in (12, 88):
            print(json.dumps(timing(B, args.T, 1440, half_width, args.repeats)), flush=True)


if __name__ == '__main__':
    main()
