"""Measure the forward-backward route (torbi_amd.forward_backward / state_posteriors) on one MI355X; prints one JSON line.

  (a) B=512, T=500, S=1440, dense synthetic matrix (synth.problem): ms per call, the fraction of the f32 MFMA peak
      (4 B T S^2 FLOP against 157.3 TFLOP/s), and a plain torch implementation (per-step torch.matmul plus elementwise ops,
      the same scaled recurrence) on the same GPU in the same process
  (b) the same at B=1
  (c) the uniform route (transition=None) at 512 x 500 x 1440: GB/s (observation read + posterior written) against 8 TB/s
  (d) workspace bytes of (a)
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--T', type=int, default=500)
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    out = {'device': torch.cuda.get_device_name(0)}
    out['a_dense_512'] = dense_case(512, args.T, 1440, args.repeats, dev)
    out['b_dense_1'] = dense_case(1, args.T, 1440, args.repeats, dev)
    out['c_uniform_512'] = uniform_case(512, args.T, 1440, args.repeats, dev)
    out['d_workspace_bytes'] = torbi_amd.forward_backward_workspace_bytes(512, args.T, 1440)
    print(json.dumps(out))


if __name__ == '__main__':
    main()
