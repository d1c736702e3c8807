"""Measure the wide band route of path entropy (entropy.forward_entropy_wide_banded) against the dense route
(entropy.forward_entropy) on one MI355X; prints one JSON line per case.

The matrix is the pitch matrix of 175 diagonals, synth.banded_transition(1440, 87.2), with -inf and with log(tiny) outside
the band, the rows peaked (tools/posterior_probe.py peaked_rows).  Per batch size the routes alternate call by call in one
process on the same inputs, each with a caller-owned workspace, timed with device events after one warm-up round: the median
of --repeats calls with min and max.  The wide route runs once per tile size G (TORBI_HIP_WIDE_BAND_ITEMS) and once with the
library's own choice.  Every line is strict JSON: a background of -inf is the string '-inf'.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from torbi_amd import _lib, entropy, synth  # noqa: E402
from posterior_probe import peaked_rows  # noqa: E402
from posterior_wide_band_probe import alternated, forced  # noqa: E402


def case(B, T, S, half_width, tiny, repeats, dev, tiles=(1, 2)):
    reach = int(np.ceil(half_width)) - 1                                  # clip(half_width - |i - j|, 0) is 0 from there on
    trans = torch.from_numpy(synth.banded_transition(S, half_width, tiny=tiny)).to(dev)
    background = float(trans[0, S - 1])
    init = torch.full((S,), float(np.log(1. / S)), device=dev)
    obs = peaked_rows(B, T, S, dev)
    frames = torch.full((B,), T, dtype=torch.int32, device=dev)
    ws = torch.empty(entropy.path_entropy_workspace_bytes(B, T, S), dtype=torch.uint8, device=dev)
    ww = torch.empty(entropy.path_entropy_wide_banded_workspace_bytes(B, T, S, reach, reach), dtype=torch.uint8, device=dev)
    wide = lambda: entropy.forward_entropy_wide_banded(obs, frames, trans, init, reach, reach, background, workspace=ww)
    calls = {'dense': lambda: entropy.forward_entropy(obs, frames, trans, init, workspace=ws), 'wide': wide}
    calls.update({f'wide_G{G}': forced(G, wide) for G in tiles})
    H, L = wide()
    rH, rL = calls['dense']()
    out = {'shape': [B, T, S], 'diagonals': 2 * reach + 1, 'background': background if np.isfinite(background) else str(background),
           'chosen_G': _lib.load().torbi_hip_path_entropy_wide_band_tile(B, S, reach, reach, 0),
           'max_abs_entropy_wide_vs_dense': float((H - rH).abs().max()), 'max_abs_loglik_wide_vs_dense': float((L - rL).abs().max())}
    out['ms'] = alternated(calls, repeats)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeats', type=int, default=7)
    ap.add_argument('--T', type=int, default=500)
    ap.add_argument('--batches', type=int, nargs='+', default=[1, 8, 64, 512, 4096])
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    print(json.dumps({'device': torch.cuda.get_device_name(0)}), flush=True)
    for B in args.batches:
        for tiny in (False, True):
            print(json.dumps(case(B, args.T, 1440, 87.2, tiny, args.repeats, dev)), flush=True)


if __name__ == '__main__':
    main()
