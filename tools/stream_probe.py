"""Measure the streaming decoder (torbi_amd.StreamDecoder) on one MI355X; prints one JSON line.

  (a) B=512, S=1440, dense synthetic matrix, 500 frames in pushes of 100: timesteps/s of the stream (flush included) and
      of torbi_amd.decode on the same whole batch in the same process, and their ratio
  (b) the same with posteriorgram-like rows and the reference's banded pitch matrix (half width 87.2)
  (c) B=1, S=1440, 1-frame pushes: host wall time per push, p50 / p99
  (d) state bytes per stream and the largest `pending` seen on (a) and (b)
Every figure of (a)-(c) is the median of --repeats runs with its min and max, device synchronised around each timed span.

--max-lag N [N ...] adds, per decision depth N (StreamDecoder(max_lag=N)):
  (e) case (c) again: p50 / p99 per push, the share of pushes that forced frames out, and the SEAMS on this input: a forced
      span whose last state is not the backpointer of the next returned frame (the whole sequence's backpointers, numpy
      float32 on the host, from the states actually returned)
  (f) an identity matrix, --identity-pushes one-frame pushes (every commit is forced): the smallest and largest capacity and
      state bytes once the bound binds (from push N + 2 on), and the time per push of the first and of the last hundred
      forcing pushes
--only-single skips the timed batches (a), (b) and (d); the input of (c) stays the same.
--route auto|dense|band builds every decoder with that route (StreamDecoder(route=...); 'band' only where the matrix has a
band: case (a) keeps 'auto'); every case reports the route its decoder took and, on the band route, the streams per
workgroup of its forward kernel.  --half-width W replaces the pitch band of (b), (c), (e): 87.2 gives 175 diagonals, 12 gives 23.
"""
import argparse
import json
import math
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torbi_amd  # noqa: E402
from torbi_amd import synth, viterbi  # noqa: E402


def spread(values):
    v = sorted(values)
    return {'median': float(np.median(v)), 'min': float(v[0]), 'max': float(v[-1]), 'runs': len(v)}


def peaked(B, T, S, dev):
    gen = torch.Generator(device=dev).manual_seed(7)
    logits = torch.randn((B, T, S), device=dev, generator=gen) * 2.0
    centre = torch.randint(0, S, (B, T, 1), device=dev, generator=gen)
    logits -= ((torch.arange(S, device=dev)[None, None, :] - centre).abs().float() / 12.0) ** 2
    return torch.log_softmax(logits, dim=-1).clamp_(min=math.log(torch.finfo(torch.float32).tiny))


ROUTE = {}            # the `route` argument of every decoder ({}: the constructor's default)


def route_of(dec):
    """{'route': ..., 'streams_per_workgroup': ...} of a decoder."""
    found = {'route': getattr(dec, 'route', 'dense')}
    band = getattr(dec, '_band', None)
    if band is not None:
        found['reach'] = [band[0], band[1]]
        found['streams_per_workgroup'] = dec._lib.torbi_hip_stream_band_tile(dec.batch, dec.states, band[0], band[1], 0)
    return found


def batch_case(obs, trans, init, push, repeats, route=None):
    B, T, S = obs.shape
    route = ROUTE if route is None else route
    dev = obs.device
    frames = torch.full((B,), T, dtype=torch.int32, device=dev)
    stream_s, decode_s, pending_max = [], [], 0
    viterbi.decode(obs, frames, trans, init)                # warm-up (library load, path choice)
    for _ in range(repeats + 1):
        dec = torbi_amd.StreamDecoder(B, S, trans, init, log_probs=True, gpu=0, **route)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for t in range(0, T, push):
            dec.push(obs[:, t:t + push])
            pending_max = max(pending_max, int(dec.pending.max()))
        dec.flush()
        torch.cuda.synchronize()
        stream_s.append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        viterbi.decode(obs, frames, trans, init)
        torch.cuda.synchronize()
        decode_s.append(time.perf_counter() - t0)
    stream_s, decode_s = stream_s[1:], decode_s[1:]          # (the first pass grows the ring)
    ts = [B * T / s for s in stream_s]
    td = [B * T / s for s in decode_s]
    return {'stream_timesteps_per_s': spread(ts), 'decode_timesteps_per_s': spread(td),
            'ratio': spread([a / b for a, b in zip(ts, td)]), 'push_frames': push,
            'state_bytes_per_stream': dec._state_bytes // B, 'pending_max': pending_max, **route_of(dec)}


def single_case(one, trans, init, repeats, max_lag=None):
    """(c): one live stream, one frame per push; the outputs of the last run come back as well."""
    S = one.shape[2]
    runs, outputs, forced_pushes = [], [], 0
    for _ in range(repeats):
        dec = torbi_amd.StreamDecoder(1, S, trans, init, log_probs=True, gpu=0, **({} if max_lag is None else {'max_lag': max_lag}),
                                      **ROUTE)
        outputs, forced_pushes = [], 0
        for t in range(20):                                  # warm-up pushes (ring growth)
            outputs.append(dec.push(one[:, t:t + 1])[0])
        times = []
        for t in range(20, one.shape[1]):
            before = int(dec.forced[0]) if max_lag is not None else 0
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = dec.push(one[:, t:t + 1])[0]
            times.append(time.perf_counter() - t0)
            outputs.append(out)
            forced_pushes += max_lag is not None and int(dec.forced[0]) > before
        outputs = [o.cpu().numpy() for o in outputs]
        dec.flush()
        runs.append((np.percentile(times, 50) * 1e3, np.percentile(times, 99) * 1e3))
    return ({'p50': spread([r[0] for r in runs]), 'p99': spread([r[1] for r in runs]), **route_of(dec)}, outputs,
            forced_pushes / len(times))


def backpointers(seq, trans, init):
    """The whole sequence's backpointers, numpy float32 (first maximum; the probe's inputs hold no NaN)."""
    T, S = seq.shape
    bp = np.zeros((T, S), np.int64)
    post = seq[0] + init
    for t in range(1, T):
        cand = post[None, :] + trans
        bp[t] = cand.argmax(axis=1)
        post = seq[t] + cand.max(axis=1)
    return bp


def seams(outputs, bp):
    """Pushes whose returned span does not continue the span before it: bp[first frame][its state] != the state before."""
    count, frame, last = 0, 0, None
    for out in outputs:
        if len(out):
            count += last is not None and int(bp[frame][int(out[0])]) != last
            frame, last = frame + len(out), int(out[-1])
    return count, frame


def identity_case(S, pushes, max_lag):
    """(f): nothing is ever decided, every returned frame is forced."""
    dev = torch.device('cuda:0')
    eye = torch.full((S, S), -math.inf, device=dev).fill_diagonal_(0.)
    flat = torch.full((S,), math.log(1. / S), dtype=torch.float32, device=dev)
    obs = peaked(1, pushes, S, dev)
    dec = torbi_amd.StreamDecoder(1, S, eye, flat, log_probs=True, gpu=0, max_lag=max_lag, **ROUTE)
    times, capacity, nbytes = [], [], []
    for t in range(pushes):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        dec.push(obs[:, t:t + 1])
        times.append(time.perf_counter() - t0)
        capacity.append(dec.capacity)
        nbytes.append(dec._state_bytes)
    warm = max_lag + 1                                        # pushes until the bound binds; the ring has its size by then
    first, last = np.array(times[warm:warm + 100]) * 1e3, np.array(times[-100:]) * 1e3      # (both force every push)
    return {'pushes': pushes, 'capacity': [min(capacity[warm:]), max(capacity[warm:])],
            'state_bytes': [min(nbytes[warm:]), max(nbytes[warm:])],
            'pending': int(dec.pending[0]), 'forced': int(dec.forced[0]), **route_of(dec),
            'first_hundred_ms': spread(first.tolist()), 'last_hundred_ms': spread(last.tolist())}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--batch', type=int, default=512)
    ap.add_argument('--frames', type=int, default=500)
    ap.add_argument('--states', type=int, default=1440)
    ap.add_argument('--push', type=int, default=100)
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--single-pushes', type=int, default=400)
    ap.add_argument('--max-lag', type=int, nargs='*', default=[], help='decision depths to measure: cases (e) and (f)')
    ap.add_argument('--identity-pushes', type=int, default=1000)
    ap.add_argument('--only-single', action='store_true', help='skip the timed batches (a), (b), (d)')
    ap.add_argument('--route', choices=['auto', 'dense', 'band'], default=None, help='StreamDecoder(route=...) of every decoder')
    ap.add_argument('--half-width', type=float, default=87.2, help='half width of the pitch band of (b), (c), (e)')
    args = ap.parse_args()
    if args.route is not None:
        ROUTE['route'] = args.route
    dev = torch.device('cuda:0')
    B, T, S = args.batch, args.frames, args.states
    result = {'device': torch.cuda.get_device_name(0), 'B': B, 'T': T, 'S': S, 'route_asked': args.route or 'default',
              'half_width': args.half_width}

    _, trans, init = synth.problem(1, 1, S, seed=0)
    trans, init = torch.from_numpy(trans).to(dev), torch.from_numpy(init).to(dev)
    obs = viterbi.fill_synthetic((B, T, S), synth.STREAM_OBSERVATION, seed=0, device=dev)
    if not args.only_single:
        result['a_dense'] = batch_case(obs, trans, init, args.push, args.repeats,      # (a dense matrix has no band to force)
                                       route={} if args.route == 'band' else None)
    del obs
    band = torch.from_numpy(synth.banded_transition(S, args.half_width)).to(dev)
    flat = torch.full((S,), math.log(1. / S), dtype=torch.float32, device=dev)
    obs = peaked(B, T, S, dev)
    if not args.only_single:
        result['b_pitch'] = batch_case(obs, band, flat, args.push, args.repeats)

    # (c) one live stream, one frame per push
    one = obs[:1, :args.single_pushes + 20].contiguous()
    result['c_single_push_ms'], _, _ = single_case(one, band, flat, args.repeats)
    if args.max_lag:
        seq = one[0].clone()                                 # the epsilon round trip of the decoder's input
        torch.exp_(seq)
        seq += torch.finfo(torch.float32).tiny
        torch.log_(seq)
        bp = backpointers(seq.cpu().numpy(), band.cpu().numpy(), flat.cpu().numpy())
    for lag in args.max_lag:
        ms, outputs, share = single_case(one, band, flat, args.repeats, max_lag=lag)
        found, returned = seams(outputs, bp)
        result[f'e_max_lag_{lag}'] = {'single_push_ms': ms, 'share_of_pushes_forced': share, 'seams': found,
                                      'frames_returned': returned, 'identity': identity_case(S, args.identity_pushes, lag)}
    result['d_bytes_per_pending_frame_per_stream'] = 4 * S + 4
    print(json.dumps(result))


if __name__ == '__main__':
    main()
