"""Measure the log-space band route of the state posteriors (torbi_amd.forward_backward_log_banded) on one MI355X; prints one
JSON line per case.

  --errors   per case of tests/test_posterior_log_band_gpu.py and on mismatched inputs (log_softmax(12 randn), seed 5, as
             tools/path_entropy_probe.py mismatched) at 8 x 500 x 1440 on 23 diagonals (-inf outside) and on 175 (log(tiny)
             outside): the largest error of gamma, of the row sums and of L against float64 log space (the test file's
             reference, run on the device in float64), for this route and for the scaled band route on the same inputs,
             with L's share of the project's bound 1e-6 |L| + 4e-6 F
  (default)  time: this route, once per tile size G (TORBI_HIP_LOG_BAND_ITEMS) and with the library's own choice, beside the
             scaled narrow route (23 diagonals) and the scaled wide route (175 diagonals) on peaked rows, alternated call by
             call in one process with caller-owned workspaces and device events: median, min and max of --repeats calls; the
             float64 host route (gpu=None) once at 8 items; exponentials per second (1.25 per term of the packed band, both
             passes) beside the transcendental issue rate 256 CUs x 64 lanes x --clock-ghz
Every line is strict JSON: a background of -inf is the string '-inf'.
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


def errors(name, obs, frames, trans, init, left, right, background):
    """One line: the errors of the log route and of the scaled band route that covers the band against float64 log space."""
    import test_posterior_log_band_gpu as cases
    obs, frames, trans, init = (torch.as_tensor(np.array(a)) for a in (obs, frames, trans, init))
    rg, rL = (torch.as_tensor(x) for x in cases.log_space(obs.to(DEV), frames.to(DEV), trans.to(DEV), init.to(DEV)))
    B, T, S = obs.shape
    F = frames.clamp(1, T).double()
    valid = (torch.arange(T)[None, :] < F[:, None])
    narrow = _lib.load().torbi_hip_forward_backward_band_covers(B, T, S, left, right, background, 0)
    scaled = torbi_amd.forward_backward_banded if narrow else torbi_amd.forward_backward_wide_banded
    out = {'case': name, 'shape': [B, T, S], 'reach': [left, right], 'background': background if np.isfinite(background) else '-inf'}
    for route, fn in (('log', torbi_amd.forward_backward_log_banded), ('scaled', scaled)):
        g, L = (x.double().cpu() for x in fn(obs.to(DEV), frames.to(DEV), trans.to(DEV), init.to(DEV), left, right, background))
        bound = 1e-6 * rL.abs() + 4e-6 * F
        out[route] = {'gamma': float((g - rg).abs().nan_to_num(nan=np.inf).max()),
                      'row_sum': float((g.sum(-1) - 1).abs()[valid].nan_to_num(nan=np.inf).max()),
                      'L': float((L - rL).abs().nan_to_num(nan=np.inf).max()),
                      'L_share_of_bound': float(((L - rL).abs() / bound).nan_to_num(nan=np.inf).max()),
                      'nan_items': int(torch.isnan(L).sum())}
    return out


def mismatched(B, T, S, half_width, tiny):
    g = torch.Generator().manual_seed(5)
    obs = torch.log_softmax(12 * torch.randn(B, T, S, generator=g), 2)
    init = torch.log_softmax(torch.randn(S, generator=g), 0)
    trans = synth.banded_transition(S, half_width, tiny=tiny)
    return obs, torch.full((B,), T, dtype=torch.int32), trans, init, half_width - 1, half_width - 1, float(trans[0, S - 1])


def forced(G, fn):
    def call():
        os.environ['TORBI_HIP_LOG_BAND_ITEMS'] = str(G)
        try:
            return fn()
        finally:
            del os.environ['TORBI_HIP_LOG_BAND_ITEMS']
    return call


def timing(B, T, S, half_width, tiny, repeats, clock_ghz, host):
    reach = half_width - 1
    trans = torch.from_numpy(synth.banded_transition(S, half_width, tiny=tiny)).to(DEV)
    background = float(trans[0, S - 1])
    init = torch.full((S,), float(np.log(1. / S)), device=DEV)
    obs = peaked_rows(B, T, S, DEV)
    frames = torch.full((B,), T, dtype=torch.int32, device=DEV)
    narrow = 2 * reach + 1 <= 64
    size = torbi_amd.forward_backward_banded_workspace_bytes if narrow else torbi_amd.forward_backward_wide_banded_workspace_bytes
    scaled = torbi_amd.forward_backward_banded if narrow else torbi_amd.forward_backward_wide_banded
    wl = torch.empty(torbi_amd.forward_backward_log_banded_workspace_bytes(B, T, S, reach, reach), dtype=torch.uint8, device=DEV)
    wsc = torch.empty(size(B, T, S, reach, reach), dtype=torch.uint8, device=DEV)
    log = lambda: torbi_amd.forward_backward_log_banded(obs, frames, trans, init, reach, reach, background, workspace=wl)
    calls = {'scaled': lambda: scaled(obs, frames, trans, init, reach, reach, background, workspace=wsc), 'log': log}
    calls.update({f'log_G{G}': forced(G, log) for G in (1, 2, 4)})
    out = {'shape': [B, T, S], 'diagonals': 2 * reach + 1, 'background': background if np.isfinite(background) else '-inf',
           'scaled_route': 'narrow' if narrow else 'wide',
           'chosen_G': _lib.load().torbi_hip_forward_backward_log_band_tile(B, S, reach, reach, 0), 'ms': alternated(calls, repeats)}
    dquads = (2 * reach + 1 + (-reach) % 4 + 3) // 4                      # the band with its leading diagonals, in fours
    terms = 2 * 4 * dquads                                                # per state and frame, both passes
    out['exponentials_per_second'] = 1.25 * terms * B * (T - 1) * S / (out['ms']['log']['median'] * 1e-3)
    out['issue_rate_per_second'] = 256 * 64 * clock_ghz * 1e9
    out['log_over_scaled'] = out['ms']['log']['median'] / out['ms']['scaled']['median']
    if host:
        t0 = time.perf_counter()
        torbi_amd.state_posteriors(obs.cpu(), frames.cpu(), trans.cpu(), init.cpu(), log_probs=True, gpu=None)
        out['host_float64_ms'] = (time.perf_counter() - t0) * 1e3
        out['host_over_log'] = out['host_float64_ms'] / out['ms']['log']['median']
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
        import test_posterior_log_band_gpu as cases
        for case in cases.SHAPES + cases.WIDE_RANGE:
            print(json.dumps(errors('test', *cases.problem(*case), *case[3:])), flush=True)
        for half_width, tiny in ((12, False), (88, True)):
            print(json.dumps(errors('mismatched', *mismatched(8, 500, 1440, half_width, tiny))), flush=True)
        return
    for B in args.batches:
        for half_width, tiny in ((12, False), (88, True)):
            print(json.dumps(timing(B, args.T, 1440, half_width, tiny, args.repeats, args.clock_ghz, host=B == 8)), flush=True)


if __name__ == '__main__':
    main()
