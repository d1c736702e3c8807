"""Measure the expected-counts route (torbi_amd.forward_backward_counts / log_likelihood) on one MI355X; prints one JSON
line.

  (a) B=512, T=500, S=1440, dense synthetic matrix (synth.problem): the counts call against forward_backward on the same
      inputs, alternated in one process; TFLOP/s of the counts call counting 6 B T S^2 FLOP
  (b) the same at B=1
  (c) the counts call against a per-step torch implementation (torch.matmul plus elementwise, the same scaled recurrence)
  (d) log_likelihood forward plus L.sum().backward() for observation, transition and initial, against forward_backward
      plus the counts call
  (e) workspace bytes of (a)
  accuracy: errors of the counts against the float64 host route on the shapes of tests/test_counts_gpu.py, with the share
      of the test bounds they use
Every time is the median of --repeats calls with its min and max, device synchronised around each call.

  --band: the band counts route (torbi_amd.forward_backward_counts_banded, csrc/counts_band.hpp) instead: on the pitch
      matrix (synth.banded_transition(1440, 12), peaked rows) the band counts call against the dense counts call and
      against forward_backward_banded (what the counting adds), the three alternated call by call, at 512 x T x 1440 with
      -inf and with log(tiny) outside the band, 1 x T x 1440 and 8 x 120 x 1440; expected_counts through both routes;
      workspace bytes (tests/test_counts_band_gpu.py prints the share of every accuracy bound it uses)
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torbi_amd  # noqa: E402
from torbi_amd import synth, training  # noqa: E402

PEAK_FLOPS = 157.3e12


def spread(values):
    v = sorted(values)
    return {'median': float(np.median(v)), 'min': float(v[0]), 'max': float(v[-1]), 'runs': len(v)}


def alternated(fns, repeats):
    """Times of each function, called in turn `repeats` times after one warm-up call each."""
    for fn in fns:
        fn()
    torch.cuda.synchronize()
    out = [[] for _ in fns]
    for _ in range(repeats):
        for k, fn in enumerate(fns):
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            out[k].append((time.perf_counter() - t0) * 1e3)
    return [spread(v) for v in out]


def torch_counts(obs, trans, init):
    """The scaled recurrence with torch ops, one matmul per step and pass plus one per counts pair."""
    B, T, S = obs.shape
    E = torch.exp(trans)
    x0 = obs[:, 0] + init
    m = torch.cat([x0.amax(-1, keepdim=True), obs[:, 1:].amax(-1)], dim=1)
    alpha = torch.empty_like(obs)
    c = torch.empty((B, T), dtype=torch.float32, device=obs.device)
    alpha[:, 0] = torch.exp(x0 - m[:, 0, None])
    c[:, 0] = alpha[:, 0].sum(-1)
    for t in range(1, T):
        alpha[:, t] = torch.exp(obs[:, t] - m[:, t, None]) * torch.matmul(alpha[:, t - 1], E.t()) / c[:, t - 1, None]
        c[:, t] = alpha[:, t].sum(-1)
    L = (torch.log(c.double()) + m.double()).sum(-1)
    w = torch.exp(obs[:, T - 1] - m[:, T - 1, None]) / c[:, T - 1, None]
    alpha[:, T - 1] /= c[:, T - 1, None]
    acc = torch.zeros((S, S), dtype=torch.float32, device=obs.device)
    for t in range(T - 2, -1, -1):
        acc += torch.matmul(w.t(), alpha[:, t] / c[:, t, None])
        beta = torch.matmul(w, E)
        alpha[:, t] *= beta / c[:, t, None]
        w = torch.exp(obs[:, t] - m[:, t, None]) * beta / c[:, t, None]
    return alpha, L.float(), E * acc, alpha[:, 0].sum(0)


def dense_case(B, T, S, repeats, dev, baseline):
    obs, trans, init = (torch.from_numpy(x).to(dev) for x in synth.problem(B, T, S, seed=1))
    frames = torch.full((B,), T, dtype=torch.int32, device=dev)
    ws = torch.empty(torbi_amd.expected_counts_workspace_bytes(B, T, S), dtype=torch.uint8, device=dev)
    fb = lambda: torbi_amd.forward_backward(obs, frames, trans, init, workspace=ws)
    counts = lambda: torbi_amd.forward_backward_counts(obs, frames, trans, init, workspace=ws)
    leaves = [x.clone().requires_grad_() for x in (obs, trans, init)]

    def autograd():
        L = torbi_amd.log_likelihood(leaves[0], frames, leaves[1], leaves[2])
        L.sum().backward()
        for x in leaves:
            x.grad = None

    t_fb, t_counts, t_auto = alternated([fb, counts, autograd], repeats)
    flops = 6.0 * B * T * S * S
    out = {'shape': [B, T, S], 'forward_backward_ms': t_fb, 'counts_ms': t_counts,
           'counts_over_forward_backward': t_counts['median'] / t_fb['median'],
           'counts_tflops': flops / t_counts['median'] / 1e9,
           'counts_fraction_of_f32_mfma_peak': flops / (t_counts['median'] * 1e-3) / PEAK_FLOPS,
           'log_likelihood_fwd_bwd_ms': t_auto,
           'fwd_bwd_over_fb_plus_counts': t_auto['median'] / (t_fb['median'] + t_counts['median'])}
    if baseline:
        (ref,) = alternated([lambda: torch_counts(obs, trans, init)], max(2, repeats // 2))
        _, _, X, I = counts()
        _, _, rX, rI = torch_counts(obs, trans, init)
        out.update(torch_ms=ref, counts_speedup_vs_torch=ref['median'] / t_counts['median'],
                   max_rel_counts_vs_torch=float(((X - rX).abs() / rX.abs().max()).max()))
    return out


def accuracy(dev):
    rows = []
    for B, T, S in [(1, 500, 1440), (3, 50, 200), (17, 64, 65), (64, 100, 256), (512, 40, 1440), (4, 20, 4096),
                    (5, 30, 1441), (520, 8, 1441)]:
        obs, trans, init = synth.problem(B, T, S, seed=B + T + S)
        frames = np.clip(synth.lengths(B, 1, T, seed=S), 1, T).astype(np.int32)
        frames[0] = T
        args = [torch.as_tensor(np.ascontiguousarray(x)) for x in (obs, frames, trans, init)]
        _, _, X, I = torbi_amd.forward_backward_counts(*[a.to(dev) for a in args])
        _, _, rX, rI = training._host_counts(*args, None)
        X, I, rX, rI = X.cpu().double(), I.cpu().double(), rX, rI
        dX, dI = (X - rX).abs(), (I - rI).abs()
        pairs = float(np.maximum(np.clip(frames, 1, T) - 1, 0).sum())
        rows.append({'shape': [B, T, S],
                     'max_rel_X': float((dX / rX.abs().clamp_min(1e-30)).max()),
                     'elementwise_X_bound_share': float((dX / (1e-4 * rX.abs() + 1e-6 * rX.abs().max())).max()),
                     'sum_abs_dX_bound_share': float(dX.sum()) / (1e-5 * max(pairs, 1.)),
                     'elementwise_I_bound_share': float((dI / (1e-4 * rI.abs() + 1e-6 * rI.abs().max())).max()),
                     'sum_abs_dI_bound_share': float(dI.sum()) / (1e-5 * B)})
    return rows


def peaked(B, T, S, half_width, seed, dev):
    """Posteriorgram rows peaked around a pitch track that moves inside the band (log of a normalised row), made on the
    device 16 items at a time."""
    rng = np.random.default_rng(seed)
    track = np.clip(np.cumsum(rng.integers(-half_width + 1, half_width, size=(B, T)), axis=1)
                    + rng.integers(S // 4, 3 * S // 4, size=(B, 1)), 0, S - 1)
    track = torch.from_numpy(track).to(dev)
    x = torch.arange(S, device=dev)
    gen = torch.Generator(device=dev).manual_seed(seed)
    obs = torch.empty((B, T, S), dtype=torch.float32, device=dev)
    for b in range(0, B, 16):
        rows = torch.exp(-0.5 * ((x - track[b:b + 16, :, None]) / 3.) ** 2)
        rows += 1e-3 * torch.rand(rows.shape, device=dev, generator=gen)
        obs[b:b + 16] = torch.log(rows / rows.sum(-1, keepdim=True))
    return obs


def band_case(B, T, S, half_width, tiny, repeats, dev):
    reach = half_width - 1
    background = float(np.log(np.finfo(np.float32).tiny)) if tiny else -np.inf
    obs = peaked(B, T, S, half_width, 1, dev)
    trans = torch.from_numpy(synth.banded_transition(S, half_width, tiny=tiny)).to(dev)
    init = torch.full((S,), float(np.log(np.float32(1. / S))), device=dev)
    frames = torch.full((B,), T, dtype=torch.int32, device=dev)
    ws = torch.empty(max(torbi_amd.expected_counts_workspace_bytes(B, T, S),
                         torbi_amd.expected_counts_banded_workspace_bytes(B, T, S, reach, reach)), dtype=torch.uint8, device=dev)
    dense = lambda: torbi_amd.forward_backward_counts(obs, frames, trans, init, workspace=ws)
    band = lambda: torbi_amd.forward_backward_counts_banded(obs, frames, trans, init, reach, reach, background, workspace=ws)
    post = lambda: torbi_amd.forward_backward_banded(obs, frames, trans, init, reach, reach, background, workspace=ws)
    fns = [dense, band, post]
    if not tiny:
        fns += [lambda: torbi_amd.expected_counts(obs, frames, trans, init, log_probs=True, gpu=0, route='dense'),
                lambda: torbi_amd.expected_counts(obs, frames, trans, init, log_probs=True, gpu=0, route='band')]
    t = alternated(fns, repeats)
    out = {'shape': [B, T, S], 'reach': reach, 'background': 'log(tiny)' if tiny else '-inf', 'dense_counts_ms': t[0],
           'band_counts_ms': t[1], 'forward_backward_banded_ms': t[2], 'dense_over_band': t[0]['median'] / t[1]['median'],
           'band_counts_over_banded': t[1]['median'] / t[2]['median'],
           'band_workspace_bytes': torbi_amd.expected_counts_banded_workspace_bytes(B, T, S, reach, reach),
           'dense_workspace_bytes': torbi_amd.expected_counts_workspace_bytes(B, T, S),
           'auto_route': torbi_amd.counts_route(trans, B, T, S, gpu=0, log_probs=True)}
    if not tiny:
        out.update(expected_counts_dense_ms=t[3], expected_counts_band_ms=t[4])
        Xd, Xb = dense()[2], torbi_amd.band_counts_to_dense(band()[2], reach, reach)
        out['max_abs_band_minus_dense_over_max'] = float((Xd - Xb).abs().max() / Xd.abs().max())
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--T', type=int, default=500)
    ap.add_argument('--no-accuracy', action='store_true')
    ap.add_argument('--band', action='store_true', help='measure the band counts route on the pitch matrix')
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    out = {'device': torch.cuda.get_device_name(0)}
    if args.band:
        out['band_512_ninf'] = band_case(512, args.T, 1440, 12, False, args.repeats, dev)
        out['band_512_tiny'] = band_case(512, args.T, 1440, 12, True, args.repeats, dev)
        out['band_1'] = band_case(1, args.T, 1440, 12, False, args.repeats, dev)
        out['band_8x120'] = band_case(8, 120, 1440, 12, False, args.repeats, dev)
        print(json.dumps(out))
        return
    out['a_dense_512'] = dense_case(512, args.T, 1440, args.repeats, dev, baseline=True)
    out['b_dense_1'] = dense_case(1, args.T, 1440, args.repeats, dev, baseline=False)
    out['e_workspace_bytes'] = torbi_amd.expected_counts_workspace_bytes(512, args.T, 1440)
    if not args.no_accuracy:
        out['accuracy'] = accuracy(dev)
    print(json.dumps(out))


if __name__ == '__main__':
    main()
