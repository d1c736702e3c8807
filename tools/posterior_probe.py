"""Measure the forward-backward route (torbi_amd.forward_backward / state_posteriors) on one MI355X; prints one JSON line.

  (a) B=512, T=500, S=1440, dense synthetic matrix (synth.problem): ms per call, the fraction of the f32 MFMA peak
      (4 B T S^2 FLOP against 157.3 TFLOP/s), and a plain torch implementation (per-step torch.matmul plus elementwise ops,
      the same scaled recurrence) on the same GPU in the same process
  (b) the same at B=1
  (c) the uniform route (transition=None) at 512 x 500 x 1440: GB/s (observation read + posterior written) against 8 TB/s
  (d) workspace bytes of (a)
  (e) --band: the band route (torbi_amd.forward_backward_banded) against the dense one on the pitch matrix
      (synth.banded_transition(1440, 12), half-width 12 = 23 diagonals) with peaked rows: 512 x T x 1440 on both matrices
      (-inf and log(tiny) outside the band), 1 x T x 1440 and 8 x 120 x 1440; the two routes alternate call by call in one
      process on the same inputs, and the largest difference of their posteriors is reported
Every time is the median of --repeats calls with its min and max, device synchronised around each call.
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
from torbi_amd import synth  # noqa: E402

PEAK_FLOPS = 157.3e12
PEAK_BYTES = 8e12


def spread(values):
    v = sorted(values)
    return {'median': float(np.median(v)), 'min': float(v[0]), 'max': float(v[-1]), 'runs': len(v)}


def timed(fn, repeats):
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return spread(out)


def torch_forward_backward(obs, trans, init):
    """The scaled recurrence with torch ops, one matmul per step (all items run every frame)."""
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
    for t in range(T - 2, -1, -1):
        beta = torch.matmul(w, E)
        alpha[:, t] *= beta / c[:, t, None]
        w = torch.exp(obs[:, t] - m[:, t, None]) * beta / c[:, t, None]
    return alpha, L.float()


def dense_case(B, T, S, repeats, dev, baseline=True):
    obs, trans, init = (torch.from_numpy(x).to(dev) for x in synth.problem(B, T, S, seed=1))
    frames = torch.full((B,), T, dtype=torch.int32, device=dev)
    ws = torch.empty(torbi_amd.forward_backward_workspace_bytes(B, T, S), dtype=torch.uint8, device=dev)
    hip = timed(lambda: torbi_amd.forward_backward(obs, frames, trans, init, workspace=ws), repeats)
    flops = 4.0 * B * T * S * S
    out = {'shape': [B, T, S], 'ms': hip, 'tflops': flops / hip['median'] / 1e9, 'fraction_of_f32_mfma_peak':
           flops / (hip['median'] * 1e-3) / PEAK_FLOPS}
    if baseline:
        ref = timed(lambda: torch_forward_backward(obs, trans, init), max(2, repeats // 2))
        g, L = torbi_amd.forward_backward(obs, frames, trans, init, workspace=ws)
        rg, rL = torch_forward_backward(obs, trans, init)
        out.update(torch_ms=ref, speedup_vs_torch=ref['median'] / hip['median'],
                   max_abs_gamma_vs_torch=float((g - rg).abs().max()), max_abs_loglik_vs_torch=float((L - rL).abs().max()))
    return out


def uniform_case(B, T, S, repeats, dev):
    gen = torch.Generator(device=dev).manual_seed(3)
    p = torch.rand((B, T, S), device=dev, generator=gen)
    p /= p.sum(-1, keepdim=True)
    obs = torch.log(p)
    init = torch.full((S,), float(np.log(1. / S)), device=dev)
    frames = torch.full((B,), T, dtype=torch.int32, device=dev)
    ws = torch.empty(torbi_amd.forward_backward_workspace_bytes(B, T, S), dtype=torch.uint8, device=dev)
    from torbi_amd.posterior import _run
    u = float(torch.tensor(np.log(1. / S), dtype=torch.float32))
    t = timed(lambda: _run(obs, frames, None, u, init, ws), repeats)
    moved = 2.0 * B * T * S * 4
    return {'shape': [B, T, S], 'ms': t, 'gbps': moved / t['median'] / 1e6,
            'fraction_of_hbm_peak': moved / (t['median'] * 1e-3) / PEAK_BYTES}


def peaked_rows(B, T, S, dev, seed=1):
    """Log posteriorgram rows peaked around a track that moves at most 11 bins per frame (built on the device)."""
    gen = torch.Generator(device=dev).manual_seed(seed)
    moves = torch.randint(-11, 12, (B, T), device=dev, generator=gen)
    start = torch.randint(S // 4, 3 * S // 4, (B, 1), device=dev, generator=gen)
    track = (start + moves.cumsum(1)).clamp_(0, S - 1)
    x = torch.arange(S, device=dev, dtype=torch.float32)
    obs = torch.empty((B, T, S), dtype=torch.float32, device=dev)
    for b0 in range(0, B, 32):
        c = track[b0:b0 + 32, :, None].float()
        row = torch.exp(-0.5 * ((x - c) / 3.) ** 2)
        row += 1e-3 * torch.rand(row.shape, device=dev, generator=gen)
        obs[b0:b0 + 32] = torch.log(row / row.sum(-1, keepdim=True))
    return obs


def band_case(B, T, S, tiny, repeats, dev):
    """Band against dense on one pitch problem, alternated call by call."""
    trans = torch.from_numpy(synth.banded_transition(S, 12, tiny=tiny)).to(dev)
    background = float(trans[0, S - 1])
    init = torch.full((S,), float(np.log(1. / S)), device=dev)
    obs = peaked_rows(B, T, S, dev)
    frames = torch.full((B,), T, dtype=torch.int32, device=dev)
    ws = torch.empty(torbi_amd.forward_backward_workspace_bytes(B, T, S), dtype=torch.uint8, device=dev)
    wb = torch.empty(torbi_amd.forward_backward_banded_workspace_bytes(B, T, S, 11, 11), dtype=torch.uint8, device=dev)
    dense = lambda: torbi_amd.forward_backward(obs, frames, trans, init, workspace=ws)
    band = lambda: torbi_amd.forward_backward_banded(obs, frames, trans, init, 11, 11, background, workspace=wb)
    g, L = band()
    rg, rL = dense()
    torch.cuda.synchronize()
    out = {'shape': [B, T, S], 'background': background, 'max_abs_gamma_band_vs_dense': float((g - rg).abs().max()),
           'max_abs_loglik_band_vs_dense': float((L - rL).abs().max()), 'band_workspace_bytes': wb.numel()}
    del g, L, rg, rL
    times = {'dense': [], 'band': []}
    for _ in range(repeats):
        for name, fn in (('dense', dense), ('band', band)):
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t0) * 1e3)
    out.update(dense_ms=spread(times['dense']), band_ms=spread(times['band']))
    out['band_speedup'] = out['dense_ms']['median'] / out['band_ms']['median']
    moved = 6.0 * B * T * S * 4             # o read by the row maxima and both passes, a written and read, gamma written
    out['band_gbps'] = moved / out['band_ms']['median'] / 1e6
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--T', type=int, default=500)
    ap.add_argument('--band', action='store_true', help='only the band cases (e)')
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    out = {'device': torch.cuda.get_device_name(0)}
    if args.band:
        out['e_band_512'] = band_case(512, args.T, 1440, False, args.repeats, dev)
        out['e_band_512_tiny'] = band_case(512, args.T, 1440, True, args.repeats, dev)
        out['e_band_1'] = band_case(1, args.T, 1440, False, args.repeats, dev)
        out['e_band_8x120'] = band_case(8, 120, 1440, False, args.repeats, dev)
        print(json.dumps(out))
        return
    out['a_dense_512'] = dense_case(512, args.T, 1440, args.repeats, dev)
    out['b_dense_1'] = dense_case(1, args.T, 1440, args.repeats, dev)
    out['c_uniform_512'] = uniform_case(512, args.T, 1440, args.repeats, dev)
    out['d_workspace_bytes'] = torbi_amd.forward_backward_workspace_bytes(512, args.T, 1440)
    print(json.dumps(out))


if __name__ == '__main__':
    main()
