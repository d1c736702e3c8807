"""Measure the wide band route of the state posteriors (torbi_amd.forward_backward_wide_banded) against the dense route
(torbi_amd.forward_backward) on one MI355X; prints one JSON line per case.

The matrix is the pitch matrix of 175 diagonals, synth.banded_transition(1440, 87.2), with -inf and with log(tiny) outside
the band, the rows peaked (tools/posterior_probe.py peaked_rows).  Per batch size the routes alternate call by call in one
process on the same inputs, each with a caller-owned workspace, timed with device events: the median of --repeats calls
with min and max.  The wide route runs once per tile size G (TORBI_HIP_WIDE_BAND_ITEMS) and once with the library's own choice.
--narrow adds the 23-diagonal pitch matrix on both band kernels.  Every line is strict JSON: a background of -inf is the
string '-inf'.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torbi_amd  # noqa: E402
from torbi_amd import _lib, synth  # noqa: E402
from posterior_probe import peaked_rows, spread  # noqa: E402


def alternated(calls, repeats):
    """{name: spread of ms} of `calls` {name: fn}, alternated call by call after one warm-up round."""
    for fn in calls.values():
        fn()
    torch.cuda.synchronize()
    times = {name: [] for name in calls}
    for _ in range(repeats):
        for name, fn in calls.items():
            start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            fn()
            stop.record()
            stop.synchronize()
            times[name].append(start.elapsed_time(stop))
    return {name: spread(v) for name, v in times.items()}


def forced(G, fn):
    def call():
        os.environ['TORBI_HIP_WIDE_BAND_ITEMS'] = str(G)
        try:
            return fn()
        finally:
            del os.environ['TORBI_HIP_WIDE_BAND_ITEMS']
    return call


def case(B, T, S, half_width, tiny, repeats, dev, tiles=(1, 2, 4), narrow=False):
    reach = int(np.ceil(half_width)) - 1                                  # clip(half_width - |i - j|, 0) is 0 from there on
    trans = torch.from_numpy(synth.banded_transition(S, half_width, tiny=tiny)).to(dev)
    background = float(trans[0, S - 1])
    init = torch.full((S,), float(np.log(1. / S)), device=dev)
    obs = peaked_rows(B, T, S, dev)
    frames = torch.full((B,), T, dtype=torch.int32, device=dev)
    ws = torch.empty(torbi_amd.forward_backward_workspace_bytes(B, T, S), dtype=torch.uint8, device=dev)
    ww = torch.empty(torbi_amd.forward_backward_wide_banded_workspace_bytes(B, T, S, reach, reach), dtype=torch.uint8, device=dev)
    wide = lambda: torbi_amd.forward_backward_wide_banded(obs, frames, trans, init, reach, reach, background, workspace=ww)
    calls = {'dense': lambda: torbi_amd.forward_backward(obs, frames, trans, init, workspace=ws), 'wide': wide}
    calls.update({f'wide_G{G}': forced(G, wide) for G in tiles})
    if narrow:
        wn = torch.empty(torbi_amd.forward_backward_banded_workspace_bytes(B, T, S, reach, reach), dtype=torch.uint8, device=dev)
        calls['narrow'] = lambda: torbi_amd.forward_backward_banded(obs, frames, trans, init, reach, reach, background, workspace=wn)
    g, L = wide()
    rg, rL = calls['dense']()
    out = {'shape': [B, T, S], 'diagonals': 2 * reach + 1, 'background': background if np.isfinite(background) else str(background),
           'chosen_G': _lib.load().torbi_hip_forward_backward_wide_band_tile(B, S, reach, reach, 0),
           'max_abs_gamma_wide_vs_dense': float((g - rg).abs().max()), 'max_abs_loglik_wide_vs_dense': float((L - rL).abs().max())}
    del g, L, rg, rL
    out['ms'] = alternated(calls, repeats)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--T', type=int, default=500)
    ap.add_argument('--batches', type=int, nargs='+', default=[1, 8, 64, 512, 4096])
    ap.add_argument('--narrow', action='store_true', help='only the 23-diagonal matrix on both band kernels, 512 items')
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    print(json.dumps({'device': torch.cuda.get_device_name(0)}), flush=True)
    if args.narrow:
        print(json.dumps(case(512, args.T, 1440, 12, False, args.repeats, dev, tiles=(), narrow=True)), flush=True)
        return
    for B in args.batches:
        for tiny in (False, True):
            print(json.dumps(case(B, args.T, 1440, 87.2, tiny, args.repeats, dev)), flush=True)


if __name__ == '__main__':
    main()
