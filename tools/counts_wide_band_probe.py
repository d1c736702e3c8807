"""Measure the wide band route of the expected counts (torbi_amd.forward_backward_counts_wide_banded) against the dense route
(torbi_amd.forward_backward_counts) and against the posteriors alone (torbi_amd.forward_backward_wide_banded) on one MI355X;
prints one JSON line per batch size.

The matrix is the pitch matrix of 175 diagonals, synth.banded_transition(1440, 87.2), -inf outside the band (the only
background the routing of expected_counts sends to a band route), the rows peaked (tools/posterior_probe.py peaked_rows).
Per batch size the three calls alternate call by call in one process on the same inputs, each with a caller-owned
workspace, timed with device events: the median of --repeats calls with min and max.  'wide_wins' is the rule of the 'auto'
table: the wide route's slowest call under the dense route's fastest.
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
from posterior_probe import peaked_rows  # noqa: E402
from posterior_wide_band_probe import alternated  # noqa: E402


def case(B, T, S, half_width, repeats, dev):
    reach = int(np.ceil(half_width)) - 1
    trans = torch.from_numpy(synth.banded_transition(S, half_width, tiny=False)).to(dev)
    init = torch.full((S,), float(np.log(1. / S)), device=dev)
    obs = peaked_rows(B, T, S, dev)
    frames = torch.full((B,), T, dtype=torch.int32, device=dev)
    need = {'dense': torbi_amd.expected_counts_workspace_bytes(B, T, S),
            'wide': torbi_amd.expected_counts_wide_banded_workspace_bytes(B, T, S, reach, reach),
            'posterior': torbi_amd.forward_backward_wide_banded_workspace_bytes(B, T, S, reach, reach)}
    ws = {name: torch.empty(n, dtype=torch.uint8, device=dev) for name, n in need.items()}
    calls = {'dense': lambda: torbi_amd.forward_backward_counts(obs, frames, trans, init, workspace=ws['dense']),
             'wide': lambda: torbi_amd.forward_backward_counts_wide_banded(obs, frames, trans, init, reach, reach,
                                                                           workspace=ws['wide']),
             'posterior': lambda: torbi_amd.forward_backward_wide_banded(obs, frames, trans, init, reach, reach,
                                                                         workspace=ws['posterior'])}
    X = torbi_amd.band_counts_to_dense(calls['wide']()[2], reach, reach)
    rX = calls['dense']()[2]
    out = {'shape': [B, T, S], 'diagonals': 2 * reach + 1, 'workspace_bytes': need,
           'shares': _lib.load().torbi_hip_forward_backward_counts_wide_band_shares(B, T, S, reach, reach),
           'max_abs_counts_wide_vs_dense': float((X - rX).abs().max()), 'max_counts': float(rX.max()),
           'sum_abs_counts_wide_vs_dense_per_pair': float((X - rX).abs().sum()) / (B * (T - 1))}
    del X, rX
    out['ms'] = alternated(calls, repeats)
    out['wide_wins'] = out['ms']['wide']['max'] < out['ms']['dense']['min']
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--T', type=int, default=500)
    ap.add_argument('--batches', type=int, nargs='+', default=[1, 8, 64, 512, 4096])
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    print(json.dumps({'device': torch.cuda.get_device_name(0)}), flush=True)
    for B in args.batches:
        try:
            print(json.dumps(case(B, args.T, 1440, 87.2, args.repeats, dev)), flush=True)
        except torch.cuda.OutOfMemoryError as exc:
            print(json.dumps({'shape': [B, args.T, 1440], 'out_of_memory': str(exc).splitlines()[0]}), flush=True)
        torch.cuda.empty_cache()


if __name__ == '__main__':
    main()
