"""Measure torbi_amd.StreamPosteriors on one MI355X; prints one JSON line and the rows of STREAM.md's tables.

  (a) B=512, S=1440, dense synthetic matrix, 500 frames in pushes of 100, lag 8: seconds per run (flush included), alternated
      run by run in one process with StreamDecoder(route='dense', max_lag=8) on the same inputs
  (b) B=1, S=1440, one-frame pushes, the pitch matrix synth.banded_transition(1440, 12), lag 8: wall time per push with the
      device synchronised inside the timed span (StreamDecoder synchronises by itself, StreamPosteriors does not), p50 / p99,
      alternated push by push with StreamDecoder(route='dense', max_lag=8); and the host's own time per push without it
  (c) state bytes per stream
  (d) the accuracy of tests/test_stream_posterior_gpu.py's shapes against the float64 route, as shares of the bounds
Every figure of (a) and (b) is the median of --repeats runs with its min and max.

--band measures the band route against the dense route instead (STREAM.md, "Streaming posteriors: band route"): both routes
of StreamPosteriors alternated in one process on the same inputs, the pitch matrix synth.banded_transition(1440, 12) with -inf
and with log(tiny) outside the band, lag 8:
  (a) B=512, 500 frames in pushes of 100: milliseconds per run (flush included)
  (b) B=1, one-frame pushes: wall time per push with the device synchronised inside the timed span, p50 / p99, and the host's
      own time per push without it
  (c) B=8, 300 frames in pushes of 15: milliseconds per run
and the accuracy of tests/test_stream_posterior_band_gpu.py's shapes against the float64 route, as shares of the bounds.
"""
import argparse
import json
import math
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import torbi_amd  # noqa: E402
from torbi_amd import synth  # noqa: E402
from stream_posterior_cases import DEVICE_GAMMA, ROW_SUM, Feeder, problem, ragged_plan  # noqa: E402
from stream_posterior_band_cases import BACKGROUNDS, band_problem  # noqa: E402

DEV = torch.device('cuda:0')
LAG = 8


def spread(values):
    v = sorted(values)
    return {'median': float(np.median(v)), 'min': float(v[0]), 'max': float(v[-1]), 'runs': len(v)}


def batch_case(B, T, S, push, repeats):
    obs, trans, init = (torch.tensor(x, device=DEV) for x in synth.problem(B, T, S, seed=3))
    times = {'posteriors': [], 'decoder': []}
    for _ in range(repeats + 1):
        for name in ('posteriors', 'decoder'):
            if name == 'posteriors':
                dec = torbi_amd.StreamPosteriors(B, S, trans, init, log_probs=True, gpu=0, lag=LAG)
            else:
                dec = torbi_amd.StreamDecoder(B, S, trans, init, log_probs=True, gpu=0, max_lag=LAG, route='dense')
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for t in range(0, T, push):
                dec.push(obs[:, t:t + push])
            dec.flush()
            torch.cuda.synchronize()
            times[name].append(time.perf_counter() - t0)
            if name == 'posteriors':
                state, capacity = dec._state_bytes, dec.capacity
                tile = dec._lib.torbi_hip_stream_posterior_tile(B, S, 0)
    found = {name: spread([1e3 * s for s in v[1:]]) for name, v in times.items()}       # (the first pass grows the ring)
    found['ratio'] = spread([a / b for a, b in zip(times['posteriors'][1:], times['decoder'][1:])])
    found.update(push_frames=push, state_bytes_per_stream=state // B, capacity=capacity, streams_per_workgroup=tile)
    return found


def single_case(S, pushes, repeats):
    gen = torch.Generator(device=DEV).manual_seed(7)
    one = torch.log_softmax(torch.randn((1, pushes + 20, S), device=DEV, generator=gen) * 2.0, dim=-1)
    trans = torch.tensor(synth.banded_transition(S, 12), device=DEV)
    init = torch.log(torch.full((S,), 1. / S, device=DEV))
    runs = {'posteriors': [], 'decoder': [], 'posteriors_host_only': []}
    for _ in range(repeats):
        sp = torbi_amd.StreamPosteriors(1, S, trans, init, log_probs=True, gpu=0, lag=LAG)
        dec = torbi_amd.StreamDecoder(1, S, trans, init, log_probs=True, gpu=0, max_lag=LAG, route='dense')
        times = {'posteriors': [], 'decoder': [], 'posteriors_host_only': []}
        for t in range(one.shape[1]):
            frame = one[:, t:t + 1]
            for name, d in (('posteriors', sp), ('decoder', dec)):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                d.push(frame)
                t1 = time.perf_counter()
                torch.cuda.synchronize()
                t2 = time.perf_counter()
                if t >= 20:                                      # (warm-up pushes: ring growth, first launches)
                    times[name].append(t2 - t0)
                    if name == 'posteriors':
                        times['posteriors_host_only'].append(t1 - t0)
        for name, v in times.items():
            runs[name].append((np.percentile(v, 50) * 1e3, np.percentile(v, 99) * 1e3))
    return {name: {'p50_ms': spread([r[0] for r in v]), 'p99_ms': spread([r[1] for r in v])} for name, v in runs.items()}


def accuracy():
    """Worst errors of the prefix property after every push on the shapes of the GPU tests: rows for STREAM.md."""
    rows = []
    cases = [(B, S, lag, 'dense', 24) for S in (1, 3, 63, 64, 65, 257) for B, lag in ((1, 0), (5, 4), (17, 8))]
    cases += [(511, 64, 2, 'dense', 9), (1021, 63, 2, 'dense', 9), (2041, 64, 2, 'dense', 9), (4081, 63, 2, 'dense', 9),
              (2, 1440, 3, 'pitch', 12), (2, 1440, 3, 'pitch, log(tiny)', 12)]
    for B, S, lag, kind, T in cases:
        obs, trans, init = problem(B, T, S, 'dense' if kind == 'dense' else 'none', True, seed=S + B)
        if kind != 'dense':
            trans = torch.from_numpy(synth.banded_transition(S, 12, tiny='tiny' in kind))
        sp = torbi_amd.StreamPosteriors(B, S, trans, init, log_probs=True, gpu=0, lag=lag)
        fd = Feeder(sp, obs, trans, init, True, DEVICE_GAMMA, record=False)
        for Tc, f in ragged_plan(B, T, seed=S + B + lag):
            fd.push(Tc, f)
        fd.flush()
        tile = sp._lib.torbi_hip_stream_posterior_tile(B, S, 0)
        rows.append({'B': B, 'S': S, 'lag': lag, 'matrix': kind, 'G': tile, 'gamma': fd.worst['gamma'],
                     'gamma_share': fd.worst['gamma'] / DEVICE_GAMMA, 'sum': fd.worst['sum'], 'sum_share': fd.worst['sum'] / ROW_SUM,
                     'loglik_share': float(fd.worst['loglik_share'])})
    return rows


ROUTES = ('dense', 'band')


def pitch_matrix(S, tiny):
    return torch.tensor(synth.banded_transition(S, 12, tiny=tiny), device=DEV)


def band_batch_case(B, T, S, push, repeats, tiny):
    """Milliseconds per run of T frames in pushes of `push`, flush included, the two routes alternated run by run."""
    gen = torch.Generator(device=DEV).manual_seed(3)
    obs = torch.log_softmax(torch.randn((B, T, S), device=DEV, generator=gen) * 2.0, dim=-1)
    trans, init = pitch_matrix(S, tiny), torch.log(torch.full((S,), 1. / S, device=DEV))
    times = {route: [] for route in ROUTES}
    for _ in range(repeats + 1):
        for route in ROUTES:
            sp = torbi_amd.StreamPosteriors(B, S, trans, init, log_probs=True, gpu=0, lag=LAG, route=route)
            assert sp.route == route
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for t in range(0, T, push):
                sp.push(obs[:, t:t + push])
            sp.flush()
            torch.cuda.synchronize()
            times[route].append(time.perf_counter() - t0)
    found = {route: spread([1e3 * s for s in v[1:]]) for route, v in times.items()}      # (the first pass grows the ring)
    found['band_wins'] = found['band']['max'] < found['dense']['min']                    # the slowest of one, the fastest of the other
    found.update(batch=B, frames=T, push_frames=push, tiny=tiny,
                 streams_per_workgroup=sp._lib.torbi_hip_stream_smooth_band_tile(B, S, 11, 11, 0))
    return found


def band_single_case(S, pushes, repeats, tiny):
    """One stream, one-frame pushes: (p50, p99) of the wall time per push with the device synchronised inside the timed span,
    and of the host's own time per push, the two routes alternated push by push."""
    gen = torch.Generator(device=DEV).manual_seed(7)
    one = torch.log_softmax(torch.randn((1, pushes + 20, S), device=DEV, generator=gen) * 2.0, dim=-1)
    trans, init = pitch_matrix(S, tiny), torch.log(torch.full((S,), 1. / S, device=DEV))
    names = [f'{route}{part}' for route in ROUTES for part in ('', '_host_only')]
    runs = {name: [] for name in names}
    for _ in range(repeats):
        decoders = [torbi_amd.StreamPosteriors(1, S, trans, init, log_probs=True, gpu=0, lag=LAG, route=route) for route in ROUTES]
        times = {name: [] for name in names}
        for t in range(one.shape[1]):
            frame = one[:, t:t + 1]
            for route, sp in zip(ROUTES, decoders):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                sp.push(frame)
                t1 = time.perf_counter()
                torch.cuda.synchronize()
                t2 = time.perf_counter()
                if t >= 20:                                      # (warm-up pushes: first launches)
                    times[route].append(t2 - t0)
                    times[route + '_host_only'].append(t1 - t0)
        for name, v in times.items():
            runs[name].append((np.percentile(v, 50) * 1e3, np.percentile(v, 99) * 1e3))
    found = {name: {'p50_ms': spread([r[0] for r in v]), 'p99_ms': spread([r[1] for r in v])} for name, v in runs.items()}
    found['band_wins'] = found['band']['p50_ms']['max'] < found['dense']['p50_ms']['min']
    found['tiny'] = tiny
    return found


def band_accuracy():
    """Worst errors of the prefix property after every push on the shapes of the band route's GPU tests."""
    rows = []
    cases = [(B, S, lag, reach, BACKGROUNDS[(S + B) % 3], 24)
             for S, reach in ((1, (0, 0)), (5, (5, 2)), (37, (36, 36)), (64, (1, 2)), (65, (5, 2)), (257, (3, 0)))
             for B, lag in ((1, 0), (5, 4), (17, 8))]
    cases += [(511, 64, 2, (1, 2), -20., 9), (1021, 63, 2, (1, 2), -3., 9), (2041, 64, 2, (1, 2), -math.inf, 9),
              (2, 1440, 3, 'pitch', -math.inf, 12), (2, 1440, 3, 'pitch', 'log(tiny)', 12), (1, 4096, 2, (31, 32), -20., 6)]
    for B, S, lag, reach, background, T in cases:
        if reach == 'pitch':
            obs, _, init = problem(B, T, S, 'none', True, seed=S + B)
            trans = torch.from_numpy(synth.banded_transition(S, 12, tiny=background != -math.inf))
            sp = torbi_amd.StreamPosteriors(B, S, trans, init, log_probs=True, gpu=0, lag=lag, route='band')
            left, right = 11, 11
        else:
            left, right = reach
            obs, trans, init, band = band_problem(B, T, S, left, right, background, True, seed=S + B)
            sp = torbi_amd.StreamPosteriors(B, S, trans, init, log_probs=True, gpu=0, lag=lag, route='band', band=band)
        fd = Feeder(sp, obs, trans, init, True, DEVICE_GAMMA, record=False)
        for Tc, f in ragged_plan(B, T, seed=S + B + lag):
            fd.push(Tc, f)
        fd.flush()
        rows.append({'B': B, 'S': S, 'lag': lag, 'reach': f'{left}/{right}', 'background': str(background),
                     'G': sp._lib.torbi_hip_stream_smooth_band_tile(B, S, left, right, 0), 'gamma': fd.worst['gamma'],
                     'gamma_share': fd.worst['gamma'] / DEVICE_GAMMA, 'sum': fd.worst['sum'], 'sum_share': fd.worst['sum'] / ROW_SUM,
                     'loglik_share': float(fd.worst['loglik_share'])})
    return rows


def band_main(args):
    found = {'device': torch.cuda.get_device_name(0), 'lag': LAG, 'batch': [], 'single': [], 'small_batch': []}
    for tiny in (False, True):
        found['batch'].append(band_batch_case(args.batch, args.frames, args.states, args.push, args.repeats, tiny))
        found['single'].append(band_single_case(args.states, args.single_pushes, args.repeats, tiny))
        found['small_batch'].append(band_batch_case(8, 300, args.states, 15, args.repeats, tiny))
    if not args.skip_accuracy:
        found['accuracy'] = band_accuracy()
    print(json.dumps(found))
    form = lambda v, digits=2: f"{v['median']:.{digits}f} ms ({v['min']:.{digits}f} - {v['max']:.{digits}f})"
    for b in found['batch'] + found['small_batch']:
        print(f"| {b['batch']} x {b['frames']} x {args.states}, pushes of {b['push_frames']}, {'log(tiny)' if b['tiny'] else '-inf'} "
              f"(G = {b['streams_per_workgroup']}) | {form(b['dense'])} | {form(b['band'])} | "
              f"{b['dense']['median'] / b['band']['median']:.1f} x | {'yes' if b['band_wins'] else 'no'} |")
    for one in found['single']:
        for name in ('dense', 'band', 'dense_host_only', 'band_host_only'):
            print(f"| {name}, {'log(tiny)' if one['tiny'] else '-inf'} | {form(one[name]['p50_ms'], 4)} | {form(one[name]['p99_ms'], 4)} |")
        print(f"| band wins, {'log(tiny)' if one['tiny'] else '-inf'} | {'yes' if one['band_wins'] else 'no'} | |")
    for r in found.get('accuracy', []):
        print(f"| {r['B']} x {r['S']}, lag {r['lag']}, reach {r['reach']}, background {r['background']} (G = {r['G']}) | "
              f"{r['gamma']:.1e} ({r['gamma_share']:.3f}) | {r['sum']:.1e} ({r['sum_share']:.3f}) | {r['loglik_share']:.3f} |")


def main():
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument('--repeats', type=int, default=5)
    p.add_argument('--batch', type=int, default=512)
    p.add_argument('--frames', type=int, default=500)
    p.add_argument('--states', type=int, default=1440)
    p.add_argument('--push', type=int, default=100)
    p.add_argument('--single-pushes', type=int, default=300)
    p.add_argument('--skip-accuracy', action='store_true')
    p.add_argument('--only-batch', action='store_true', help='case (a) alone: the target of a kernel trace')
    p.add_argument('--band', action='store_true', help='the band route against the dense route (see above)')
    args = p.parse_args()
    if args.band:
        return band_main(args)
    found = {'device': torch.cuda.get_device_name(0), 'lag': LAG,
             'batch': batch_case(args.batch, args.frames, args.states, args.push, args.repeats)}
    if not args.only_batch:
        found['single'] = single_case(args.states, args.single_pushes, args.repeats)
    if not args.skip_accuracy and not args.only_batch:
        found['accuracy'] = accuracy()
    print(json.dumps(found))
    b = found['batch']
    print(f"| {args.batch} x {args.frames} x {args.states}, pushes of {args.push}, lag {LAG} | "
          + ' | '.join(f"{b[k]['median']:.2f} ms ({b[k]['min']:.2f} - {b[k]['max']:.2f})" for k in ('posteriors', 'decoder'))
          + f" | {b['ratio']['median']:.2f} x ({b['ratio']['min']:.2f} - {b['ratio']['max']:.2f}) |")
    for name, v in found.get('single', {}).items():
        print(f'| {name} | ' + ' | '.join(f"{v[k]['median']:.4f} ms ({v[k]['min']:.4f} - {v[k]['max']:.4f})" for k in ('p50_ms', 'p99_ms')) + ' |')
    for r in found.get('accuracy', []):
        print(f"| {r['B']} x {r['S']}, lag {r['lag']}, {r['matrix']} (G = {r['G']}) | {r['gamma']:.1e} ({r['gamma_share']:.3f}) | "
              f"{r['sum']:.1e} ({r['sum_share']:.3f}) | {r['loglik_share']:.3f} |")


if __name__ == '__main__':
    main()
