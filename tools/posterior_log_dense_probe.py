"""Measure the dense log-space route of the state posteriors (torbi_amd.forward_backward_log) on one MI355X; prints one JSON
line per case.

  --errors   per case of tests/test_posterior_log_dense_gpu.py: the largest error of gamma, of the row sums and of L against
             float64 log space (the test file's reference, run on the device in float64) with L's share of the project's bound
             1e-6 |L| + 4e-6 F, for this route and for the scaled dense route (torbi_amd.forward_backward) on the same inputs,
             with the items whose L the route returns as NaN
  (default)  time at B x 500 x 1440 on the 175-diagonal pitch matrix (-inf outside) with peaked rows: this route with the
             library's own tile and once per tile size TB (TORBI_HIP_LOG_DENSE_ITEMS), the scaled dense route and the
             log-space band route on the same inputs, alternated call by call in one process with caller-owned workspaces and
             device events: median, min and max of --repeats calls; this route and the scaled dense one also on a matrix with
             no band (log_softmax(4 randn)); the float64 host route (gpu=None) once at 1 and 8 items; exponentials per second
             (1.25 per term, S x 4 ceil(S / 4) terms per frame and pass) beside the transcendental issue rate
             256 CUs x 64 lanes x --clock-ghz
Every line is strict JSON.
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
from torbi_amd import _lib, synth  # noqa: E402
from posterior_probe import peaked_rows  # noqa: E402
from posterior_wide_band_probe import alternated  # noqa: E402

DEV = torch.device('cuda:0')
TILES = (1, 2, 4, 8)


def errors(case):
    """One line: the errors of the log route and of the scaled dense route against float64 log space."""
    import test_posterior_log_dense_gpu as cases
    obs, frames, trans, init = (torch.as_tensor(np.array(a)).to(DEV) for a in cases.problem(*case))
    rg, rL = (torch.as_tensor(x) for x in cases.log_space(obs, frames, trans, init))
    B, T, S = obs.shape
    F = frames.cpu().clamp(1, T).double()
    valid = (torch.arange(T)[None, :] < F[:, None])
    bound = 1e-6 * rL.abs() + 4e-6 * F
    out = {'case': 'wide-range' if case in cases.WIDE_RANGE else 'test', 'shape': [B, T, S]}
    for route, fn in (('log', torbi_amd.forward_backward_log), ('scaled', torbi_amd.forward_backward)):
        g, L = (x.double().cpu() for x in fn(obs, frames, trans, init))
        out[route] = {'gamma': float((g - rg).abs().nan_to_num(nan=np.inf).max()),
                      'row_sum': float((g.sum(-1) - 1).abs()[valid].nan_to_num(nan=np.inf).max()),
                      'L': float((L - rL).abs().nan_to_num(nan=np.inf).max()),
                      'L_share_of_bound': float(((L - rL).abs() / bound).nan_to_num(nan=np.inf).max()),
                      'nan_items': int(torch.isnan(L).sum())}
        out[route] = {k: v if np.isfinite(v) else 'inf' for k, v in out[route].items()}
    return out


def forced(TB, fn):
    def call():
        os.environ['TORBI_HIP_LOG_DENSE_ITEMS'] = str(TB)
        try:
            return fn()
        finally:
            del os.environ['TORBI_HIP_LOG_DENSE_ITEMS']
    return call


def timing(B, T, S, repeats, clock_ghz, host):
    reach = 87
    pitch = torch.from_numpy(synth.banded_transition(S, reach + 1)).to(DEV)
    full = torch.log_softmax(4 * torch.randn(S, S, generator=torch.Generator().manual_seed(5)), 0).to(DEV)
    init = torch.full((S,), float(np.log(1. / S)), device=DEV)
    obs = peaked_rows(B, T, S, DEV)
    frames = torch.full((B,), T, dtype=torch.int32, device=DEV)
    wd = torch.empty(torbi_amd.forward_backward_log_workspace_bytes(B, T, S), dtype=torch.uint8, device=DEV)
    ws = torch.empty(torbi_amd.forward_backward_workspace_bytes(B, T, S), dtype=torch.uint8, device=DEV)
    wb = torch.empty(torbi_amd.forward_backward_log_banded_workspace_bytes(B, T, S, reach, reach), dtype=torch.uint8, device=DEV)
    log = lambda: torbi_amd.forward_backward_log(obs, frames, pitch, init, workspace=wd)
    calls = {'scaled': lambda: torbi_amd.forward_backward(obs, frames, pitch, init, workspace=ws), 'log': log,
             'log_band': lambda: torbi_amd.forward_backward_log_banded(obs, frames, pitch, init, reach, reach, -np.inf, workspace=wb),
             'scaled_no_band': lambda: torbi_amd.forward_backward(obs, frames, full, init, workspace=ws),
             'log_no_band': lambda: torbi_amd.forward_backward_log(obs, frames, full, init, workspace=wd)}
    calls.update({f'log_TB{TB}': forced(TB, log) for TB in TILES})
    out = {'shape': [B, T, S], 'chosen_TB': _lib.load().torbi_hip_forward_backward_log_tile(B, S, 0), 'ms': alternated(calls, repeats)}
    terms = 2 * S * 4 * ((S + 3) // 4)                                    # per item and frame, both passes
    out['exponentials_per_second'] = 1.25 * terms * B * (T - 1) / (out['ms']['log']['median'] * 1e-3)
    out['issue_rate_per_second'] = 256 * 64 * clock_ghz * 1e9
    out['log_over_scaled'] = out['ms']['log']['median'] / out['ms']['scaled']['median']
    out['log_over_log_band'] = out['ms']['log']['median'] / out['ms']['log_band']['median']
    if host:
        t0 = time.perf_counter()
        torbi_amd.state_posteriors(obs.cpu(), frames.cpu(), pitch.cpu(), init.cpu(), log_probs=True, gpu=None)
        out['host_float64_ms'] = (time.perf_counter() - t0) * 1e3
        out['host_over_log'] = out['host_float64_ms'] / out['ms']['log']['median']
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--errors', action='store_true')
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--T', type=int, default=500)
    ap.add_argument('--batches', type=int, nargs='+', default=[1, 8, 64, 512])
    ap.add_argument('--clock-ghz', type=float, default=2.4)
    args = ap.parse_args()
    print(json.dumps({'device': torch.cuda.get_device_name(0)}), flush=True)
    if args.errors:
        import test_posterior_log_dense_gpu as cases
        for case in cases.SHAPES + cases.WIDE_RANGE:
            print(json.dumps(errors(case)), flush=True)
        return
    for B in args.batches:
        print(json.dumps(timing(B, args.T, 1440, args.repeats, args.clock_ghz, host=B <= 8)), flush=True)


if __name__ == '__main__':
    main()
