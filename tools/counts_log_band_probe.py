"""Measure the log-space band counts (torbi_amd.forward_backward_counts_log_banded) on one MI355X; prints one JSON line per
case.

  --errors   per case of tests/test_counts_log_band_gpu.py and on mismatched inputs (tools/posterior_log_band_probe.py
             mismatched) at 8 x 500 x 1440 on 23 and on 175 diagonals, -inf outside: the worst share of every bound of
             check_counts (elementwise and summed, X and I) and of L's bound against the test file's float64 log-space
             reference, run on the device
  (default)  time at B x T x 1440 on 23 and 175 diagonals, -inf outside, peaked rows: this operator, the launch that feeds
             it (forward_backward_log_banded: the difference is the price of the counts) and the scaled narrow or wide
             counts operator, alternated call by call in one process with caller-owned workspaces and device events: median,
             min and max of --repeats calls; the float64 host route (gpu=None) once at 8 items; the counts kernel's
             exponentials per second (one per term of the instance's padded band) beside the transcendental issue rate
             256 CUs x 64 lanes x --clock-ghz
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, 'tools'), os.path.join(ROOT, 'tests'), ROOT]
import torbi_amd  # noqa: E402
from torbi_amd import synth  # noqa: E402
from posterior_log_band_probe import mismatched  # noqa: E402
from posterior_probe import peaked_rows  # noqa: E402
from posterior_wide_band_probe import alternated  # noqa: E402

DEV = torch.device('cuda:0')


def errors(name, obs, frames, trans, init, left, right, background):
    import test_counts_log_band_gpu as cases
    obs, frames, trans, init = (torch.as_tensor(np.array(a)).to(DEV) for a in (obs, frames, trans, init))
    _, rL, rX, rI = cases.log_space_counts(obs, frames, trans, init, left, right)
    _, L, X, I = (x.double().cpu().numpy() for x in
                  torbi_amd.forward_backward_counts_log_banded(obs, frames, trans, init, left, right, background))
    B, T, S = obs.shape
    F = np.clip(frames.cpu().numpy(), 1, T)
    share = lambda d, b: float(np.max(np.where(d > 0, d / np.maximum(b, 1e-300), 0.)))
    dX, dI, dL = np.abs(X - rX), np.abs(I - rI), np.abs(L - rL)
    return {'case': name, 'shape': [B, T, S], 'reach': [left, right], 'background': background if np.isfinite(background) else '-inf',
            'X_elementwise': share(dX, 1e-4 * np.abs(rX) + 1e-6 * np.abs(rX).max()),
            'X_sum': float(dX.sum() / (1e-5 * max((F - 1).sum(), 1))),
            'I_elementwise': share(dI, 1e-4 * np.abs(rI) + 1e-6 * np.abs(rI).max()), 'I_sum': float(dI.sum() / (1e-5 * B)),
            'L': share(dL, 1e-6 * np.abs(rL) + 4e-6 * F), 'X_largest_error': float(dX.max()), 'X_largest': float(rX.max())}


def timing(B, T, S, half_width, repeats, clock_ghz, host):
    reach = half_width - 1
    trans = torch.from_numpy(synth.banded_transition(S, half_width, tiny=False)).to(DEV)
    init = torch.full((S,), float(np.log(1. / S)), device=DEV)
    obs = peaked_rows(B, T, S, DEV)
    frames = torch.full((B,), T, dtype=torch.int32, device=DEV)
    narrow = 2 * reach + 1 <= 64
    scaled = torbi_amd.forward_backward_counts_banded if narrow else torbi_amd.forward_backward_counts_wide_banded
    size = torbi_amd.expected_counts_banded_workspace_bytes if narrow else torbi_amd.expected_counts_wide_banded_workspace_bytes
    ws = {name: torch.empty(need(B, T, S, reach, reach), dtype=torch.uint8, device=DEV) for name, need in
          (('counts_log', torbi_amd.expected_counts_log_banded_workspace_bytes),
           ('posterior_log', torbi_amd.forward_backward_log_banded_workspace_bytes), ('counts_scaled', size))}
    run = lambda fn, name: lambda: fn(obs, frames, trans, init, reach, reach, workspace=ws[name])
    calls = {'counts_log': run(torbi_amd.forward_backward_counts_log_banded, 'counts_log'),
             'posterior_log': run(torbi_amd.forward_backward_log_banded, 'posterior_log'),
             'counts_scaled': run(scaled, 'counts_scaled')}
    out = {'shape': [B, T, S], 'diagonals': 2 * reach + 1, 'scaled_route': 'narrow' if narrow else 'wide',
           'ms': alternated(calls, repeats)}
    W = 2 * reach + 1
    quarter = (-(-W // -(-W // 128)) + 3) // 4                           # csrc/counts_log_band.hpp counts_plan: the instance
    dq = 4 if quarter <= 4 else -(-quarter // 8) * 8
    padded = 4 * dq * -(-W // (4 * dq))                                   # diagonals the chunks compute
    price = out['ms']['counts_log']['median'] - out['ms']['posterior_log']['median']
    out['counts_price_ms'] = price
    out['exponentials_per_second'] = padded * B * (T - 1) * (-(-S // 64) * 64) / (price * 1e-3) if price > 0 else None
    out['issue_rate_per_second'] = 256 * 64 * clock_ghz * 1e9
    if host:
        t0 = time.perf_counter()
        torbi_amd.expected_counts(obs.cpu(), frames.cpu(), trans.cpu(), init.cpu(), log_probs=True, gpu=None)
        out['host_float64_ms'] = (time.perf_counter() - t0) * 1e3
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--errors', action='store_true')
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--T', type=int, default=500)
    ap.add_argument('--batches', type=int, nargs='+', default=[1, 8, 64, 512, 4096])
    ap.add_argument('--clock-ghz', type=float, default=2.4)
    args = ap.parse_args()
    print(json.dumps({'device': torch.cuda.get_device_name(0)}), flush=True)
    if args.errors:
        import test_counts_log_band_gpu as cases
        for case in cases.CASES + cases.WIDE_RANGE:
            print(json.dumps(errors('test', *cases.problem(*case), *case[3:])), flush=True)
        for half_width in (12, 88):
            print(json.dumps(errors('mismatched', *mismatched(8, 500, 1440, half_width, False))), flush=True)
        return
    for B in args.batches:
        for half_width in (12, 88):
            print(json.dumps(timing(B, args.T, 1440, half_width, args.repeats, args.clock_ghz, host=B == 8)), flush=True)


if __name__ == '__main__':
    main()
