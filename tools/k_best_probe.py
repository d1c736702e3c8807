"""Measure k-best Viterbi decoding (torbi_amd.decode_k_best) on one MI355X; prints one JSON line.

Cases (timesteps/s = B * T / seconds per call):
  dense_k{1,4,16}     B=512, T=500, S=1440, dense synthetic matrix (synth.problem's streams, filled on the device)
  uniform_k{1,4,16}   the same observation, transition=None (uniform route)
  band_{inf,tiny}_k{1,4,8}, band23_{inf,tiny}_k{1,4,8}   (--band-ks) the same observation on banded_transition(1440, 87.2)
                      (175 diagonals; with tiny the matrix the reference's evaluation decodes) and banded_transition(1440, 12)
                      (23 diagonals), -inf or log(tiny) outside the band; each holds {'dense': ..., 'band': ...}, the two
                      device routes (--routes) on the same input.  Every other case runs route='dense'.
  small_states_k4     B=4096, T=500, S=64, dense
  decode              torbi_amd.decode on the dense case, for scale
Every call owns its workspace; each time is taken from device events around one call after --warmup calls, and reported
as the median of --repeats calls with its min and max.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torbi_amd  # noqa: E402
from torbi_amd import synth, viterbi  # noqa: E402


def timed(fn, warmup, repeats):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(repeats):
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        fn()
        end.record()
        end.synchronize()
        ms.append(start.elapsed_time(end))
    ms.sort()
    return {'median': float(np.median(ms)), 'min': float(ms[0]), 'max': float(ms[-1]), 'runs': len(ms)}


def case(obs, frames, trans, init, k, warmup, repeats, route='dense'):
    B, T, S = obs.shape
    need = torbi_amd.decode_k_best_workspace_bytes(B, T, 1 if trans is None else S, k)
    if route == 'band':
        left, right, _ = viterbi.band_over(trans, trans, S)
        need = torbi_amd.decode_k_best_banded_workspace_bytes(B, T, S, k, left, right)
    ws = torch.empty(need, dtype=torch.uint8, device=obs.device)
    t = timed(lambda: torbi_amd.decode_k_best(obs, frames, trans, init, k, workspace=ws, route=route), warmup, repeats)
    out = {'shape': [B, T, S], 'k': k, 'ms': t, 'timesteps_per_s': B * T / (t['median'] * 1e-3),
           'workspace_bytes': ws.numel()}
    del ws
    torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--warmup', type=int, default=1)
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--B', type=int, default=512)
    ap.add_argument('--T', type=int, default=500)
    ap.add_argument('--ks', default='1,4,16')
    ap.add_argument('--band-ks', default='1,4,8')
    ap.add_argument('--routes', default='dense,band')
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    B, T, S = args.B, args.T, 1440
    ks = [int(k) for k in args.ks.split(',')]
    obs = viterbi.fill_synthetic((B, T, S), synth.STREAM_OBSERVATION, seed=0, device=dev)
    trans = viterbi.fill_synthetic((S, S), synth.STREAM_TRANSITION, seed=0, device=dev)
    init = viterbi.fill_synthetic((S,), synth.STREAM_INITIAL, seed=0, device=dev)
    frames = torch.full((B,), T, dtype=torch.int32, device=dev)
    out = {'device': torch.cuda.get_device_name(0), 'warmup': args.warmup, 'repeats': args.repeats}
    d = timed(lambda: torbi_amd.decode(obs, frames, trans, init), args.warmup, args.repeats)
    out['decode'] = {'shape': [B, T, S], 'ms': d, 'timesteps_per_s': B * T / (d['median'] * 1e-3)}
    for k in ks:
        out[f'dense_k{k}'] = case(obs, frames, trans, init, k, args.warmup, args.repeats)
    for k in ks:
        out[f'uniform_k{k}'] = case(obs, frames, None, init, k, args.warmup, args.repeats)
    for width, half in (('band', 87.2), ('band23', 12)):
        for name, tiny in (('inf', False), ('tiny', True)):
            band = torch.from_numpy(synth.banded_transition(S, half, tiny=tiny)).to(dev)
            for k in [int(k) for k in args.band_ks.split(',') if k]:
                out[f'{width}_{name}_k{k}'] = {route: case(obs, frames, band, init, k, args.warmup, args.repeats, route)
                                               for route in args.routes.split(',')}
            del band
    del obs
    torch.cuda.empty_cache()
    Bs, Ss = 4096, 64
    obs = viterbi.fill_synthetic((Bs, T, Ss), synth.STREAM_OBSERVATION, seed=1, device=dev)
    trans = viterbi.fill_synthetic((Ss, Ss), synth.STREAM_TRANSITION, seed=1, device=dev)
    init = viterbi.fill_synthetic((Ss,), synth.STREAM_INITIAL, seed=1, device=dev)
    frames = torch.full((Bs,), T, dtype=torch.int32, device=dev)
    out['small_states_k4'] = case(obs, frames, trans, init, 4, args.warmup, args.repeats)
    print(json.dumps(out), flush=True)


if __name__ == '__main__':
    main()
