"""Measure posterior path sampling (torbi_amd.forward_sample / sample_paths) on one MI355X; prints one JSON line.

  (a) forward_sample at 512 x T x 1440 with 1 and 16 draws and at 1 x T x 1440 with 1 draw, against forward_backward on the
      same inputs, alternated call by call in one process; the sampler launch alone (from the kernel times torch.profiler
      reports for one call) in total and per frame
  (b) the same shapes against a per-step torch implementation on the same GPU: the scaled forward recurrence with
      torch.matmul, then a backward loop of cumsum and searchsorted
  (c) the uniform route (transition=None) at 512 x T x 1440 with 1 and 16 draws: GB/s (observation and uniforms read,
      indices written) against 8 TB/s, beside forward_backward's uniform route (observation read, posterior written)
  (d) workspace bytes
  --band: instead of (a) - (d), forward_sample against forward_sample_banded on the pitch matrix (1440 states, half-width 12,
      -inf and log(tiny) outside the band), alternated call by call in one process on the same inputs, at 512 x T x 1440 with 1
      and 16 draws, 1 x T x 1440 and 8 x 120 x 1440 with 1 draw (SAMPLING.md, "Band route"); with --trace only the kernel times
      of one call of each (the sampler launches and the filters), a run of its own
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
from torbi_amd import posterior, sampling, synth  # noqa: E402

PEAK_BYTES = 8e12


def spread(values):
    v = sorted(values)
    return {'median': float(np.median(v)), 'min': float(v[0]), 'max': float(v[-1]), 'runs': len(v)}


def alternated(calls, repeats):
    """{name: spread of ms}: the calls alternate call by call, after one untimed round."""
    for fn in calls.values():
        fn()
    torch.cuda.synchronize()
    times = {name: [] for name in calls}
    for _ in range(repeats):
        for name, fn in calls.items():
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t0) * 1e3)
    return {name: spread(v) for name, v in times.items()}


def kernel_ms(fn, needle):
    """Device time (ms) of the kernels whose name contains `needle` in one call of fn, or None where the profiler reports
    no kernels."""
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        total, seen = 0., False
        for event in prof.key_averages():
            if needle in event.key:
                seen = True
                total += getattr(event, 'device_time_total', None) or getattr(event, 'cuda_time_total', 0.)
        return total / 1e3 if seen else None
    except Exception as exc:                      # the numbers above do not depend on the profiler
        return f'profiler failed: {exc}'


def torch_sample(obs, trans, init, uniforms):
    """Forward filtering with one matmul per step, backward sampling with cumsum / searchsorted per step."""
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
    N = uniforms.shape[1]
    out = torch.empty((B, N, T), dtype=torch.int64, device=obs.device)
    j = None
    for t in range(T - 1, -1, -1):
        w = alpha[:, t, None, :].expand(B, N, S)
        if j is not None:
            w = w * E[j]
        P = torch.cumsum(w, dim=-1)
        j = torch.searchsorted(P, (uniforms[:, :, t] * P[..., -1])[..., None], right=True)[..., 0].clamp_(max=S - 1)
        out[:, :, t] = j
    return out.int(), L.float()


def dense_case(B, T, S, draws, repeats, dev, baseline=True):
    obs, trans, init = (torch.from_numpy(x).to(dev) for x in synth.problem(B, T, S, seed=1))
    frames = torch.full((B,), T, dtype=torch.int32, device=dev)
    wf = torch.empty(torbi_amd.forward_backward_workspace_bytes(B, T, S), dtype=torch.uint8, device=dev)
    out = {'shape': [B, T, S]}
    calls = {'forward_backward': lambda: torbi_amd.forward_backward(obs, frames, trans, init, workspace=wf)}
    us = {}
    ws = torch.empty(torbi_amd.forward_sample_workspace_bytes(B, T, S, max(draws)), dtype=torch.uint8, device=dev)
    for n in draws:
        us[n] = torch.rand((B, n, T), device=dev, generator=torch.Generator(device=dev).manual_seed(n))
        calls[f'forward_sample_{n}'] = lambda n=n: torbi_amd.forward_sample(obs, frames, trans, init, us[n], workspace=ws)
    out['ms'] = alternated(calls, repeats)
    for n in draws:
        name = f'forward_sample_{n}'
        out[f'{name}_over_forward_backward'] = out['ms'][name]['median'] / out['ms']['forward_backward']['median']
        k = kernel_ms(calls[name], 'sample_backward_kernel')
        out[f'sampler_launch_ms_{n}'] = k
        if isinstance(k, float):
            out[f'sampler_us_per_frame_{n}'] = 1e3 * k / T
    if baseline:
        del wf
        for n in draws:
            ref = alternated({'torch': lambda n=n: torch_sample(obs, trans, init, us[n])}, max(2, repeats // 2))['torch']
            out[f'torch_ms_{n}'] = ref
            out[f'speedup_vs_torch_{n}'] = ref['median'] / out['ms'][f'forward_sample_{n}']['median']
    out['workspace_bytes'] = ws.numel()
    return out


def uniform_case(B, T, S, draws, repeats, dev):
    gen = torch.Generator(device=dev).manual_seed(3)
    p = torch.rand((B, T, S), device=dev, generator=gen)
    p /= p.sum(-1, keepdim=True)
    obs = torch.log(p)
    init = torch.full((S,), float(np.log(1. / S)), device=dev)
    frames = torch.full((B,), T, dtype=torch.int32, device=dev)
    value = float(torch.tensor(np.log(1. / S), dtype=torch.float32))
    wf = torch.empty(torbi_amd.forward_backward_workspace_bytes(B, T, S), dtype=torch.uint8, device=dev)
    calls = {'forward_backward_uniform': lambda: posterior._run(obs, frames, None, value, init, wf)}
    ws = torch.empty(torbi_amd.forward_sample_workspace_bytes(B, T, S, max(draws), uniform=True), dtype=torch.uint8, device=dev)
    us = {}
    for n in draws:
        us[n] = torch.rand((B, n, T), device=dev, generator=gen)
        calls[f'sample_uniform_{n}'] = lambda n=n: sampling._run(obs, frames, None, value, init, us[n], ws)
    out = {'shape': [B, T, S], 'ms': alternated(calls, repeats), 'workspace_bytes': ws.numel()}
    moved = {'forward_backward_uniform': 2.0 * B * T * S * 4}
    for n in draws:
        moved[f'sample_uniform_{n}'] = B * T * S * 4.0 + 2.0 * B * n * T * 4
    out['fraction_of_hbm_peak'] = {k: moved[k] / (out['ms'][k]['median'] * 1e-3) / PEAK_BYTES for k in moved}
    out['gbps'] = {k: moved[k] / out['ms'][k]['median'] / 1e6 for k in moved}
    # the row kernels alone (the calls above also hold the per-item sum and, for sampling, the mask launch)
    rows = {'forward_backward_uniform': 'fb_uniform_rows_kernel'}
    rows.update({f'sample_uniform_{n}': 'sample_uniform_rows_kernel' for n in draws})
    out['rows_kernel_ms'] = {k: kernel_ms(calls[k], needle) for k, needle in rows.items()}
    out['rows_kernel_fraction_of_hbm_peak'] = {k: moved[k] / (v * 1e-3) / PEAK_BYTES
                                               for k, v in out['rows_kernel_ms'].items() if isinstance(v, float)}
    return out


def band_case(B, T, S, draws, tiny, repeats, dev, trace):
    obs, _, init = (torch.from_numpy(x).to(dev) for x in synth.problem(B, T, S, seed=1))
    trans = torch.as_tensor(synth.banded_transition(S, 12, tiny=tiny)).to(dev)
    frames = torch.full((B,), T, dtype=torch.int32, device=dev)
    background = float(np.log(np.finfo(np.float32).tiny)) if tiny else -float('inf')
    wd = torch.empty(torbi_amd.forward_sample_workspace_bytes(B, T, S, max(draws)), dtype=torch.uint8, device=dev)
    wb = torch.empty(torbi_amd.forward_sample_banded_workspace_bytes(B, T, S, max(draws), 11, 11), dtype=torch.uint8, device=dev)
    out = {'shape': [B, T, S], 'background': 'log(tiny)' if tiny else '-inf', 'workspace_bytes': {'dense': wd.numel(), 'band': wb.numel()}}
    calls, us = {}, {}
    for n in draws:
        us[n] = torch.rand((B, n, T), device=dev, generator=torch.Generator(device=dev).manual_seed(n))
        calls[f'dense_{n}'] = lambda n=n: torbi_amd.forward_sample(obs, frames, trans, init, us[n], workspace=wd)
        calls[f'band_{n}'] = lambda n=n: torbi_amd.forward_sample_banded(obs, frames, trans, init, us[n], 11, 11, background,
                                                                        workspace=wb)
    if trace:
        for fn in calls.values():
            fn()
        torch.cuda.synchronize()
        out['kernel_ms'] = {}
        for n in draws:
            out['kernel_ms'][f'dense_{n}'] = {'sampler': kernel_ms(calls[f'dense_{n}'], 'sample_backward_kernel')}
            out['kernel_ms'][f'band_{n}'] = {'sampler': kernel_ms(calls[f'band_{n}'], 'sample_band_backward_kernel'),
                                             'filter': kernel_ms(calls[f'band_{n}'], 'fb_band_filter_kernel')}
        return out
    out['ms'] = alternated(calls, repeats)
    for n in draws:
        dense, band = out['ms'][f'dense_{n}'], out['ms'][f'band_{n}']
        out[f'dense_over_band_{n}'] = dense['median'] / band['median']
        # faster by more than the spread: the slowest band call against the fastest dense call
        out[f'band_faster_beyond_spread_{n}'] = band['max'] < dense['min']
    L = [calls[f'{k}_{draws[0]}']()[1] for k in ('dense', 'band')]
    out['finite_L'] = bool(torch.isfinite(L[0]).all() and torch.isfinite(L[1]).all())
    out['max_abs_L_difference'] = float((L[0].double() - L[1].double()).abs().max())
    return out


def band_main(args, dev):
    out = {'device': torch.cuda.get_device_name(0), 'trace': bool(args.trace)}
    for tiny in (False, True):
        form = 'tiny' if tiny else 'inf'
        out[f'band_512_{form}'] = band_case(512, args.T, 1440, (1, 16), tiny, args.repeats, dev, args.trace)
        out[f'band_1_{form}'] = band_case(1, args.T, 1440, (1,), tiny, args.repeats, dev, args.trace)
        out[f'band_8_{form}'] = band_case(8, 120, 1440, (1,), tiny, args.repeats, dev, args.trace)
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--band', action='store_true', help='forward_sample against forward_sample_banded on the pitch matrix')
    ap.add_argument('--trace', action='store_true', help='with --band: kernel times of one call each instead of call times')
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--T', type=int, default=500)
    ap.add_argument('--no-torch', action='store_true', help='skip the per-step torch implementation (b)')
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    if args.band:
        return band_main(args, dev)
    out = {'device': torch.cuda.get_device_name(0)}
    out['a_dense_512'] = dense_case(512, args.T, 1440, (1, 16), args.repeats, dev, not args.no_torch)
    out['a_dense_1'] = dense_case(1, args.T, 1440, (1,), args.repeats, dev, not args.no_torch)
    out['c_uniform_512'] = uniform_case(512, args.T, 1440, (1, 16), args.repeats, dev)
    print(json.dumps(out))


if __name__ == '__main__':
    main()
