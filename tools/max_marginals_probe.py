"""Measure max-marginals (torbi_amd.margins.forward_backward_max, MARGINALS.md) on one MI355X; prints one JSON line.

At B x T x S (512 x 500 x 1440 by default), with a caller-owned workspace, every time from hipEvents on the stream around one
call, after a warm-up call, as median / min / max of --repeats calls:

  (a) dense random matrix (synth.problem)
  (b) the -inf pitch band (synth.banded_transition(S, 12)) through the dense route
  (c) the uniform model (transition=None): the algorithmic bytes -- the observation read twice, the marginals written
      once, 12 B T S -- over the time, as a fraction of the HBM peak

and the yardsticks, in the same process on the same inputs:

  * the torch-op formulation of (a): the contract's loop with broadcast add and amax, chunked over next-states so that a
    temporary holds at most 2^28 values; its values are compared with the HIP route's
  * the every-cell dense decode (torbi_amd.decode(..., path='dense')) of the same shape: twice its time is the cost of the
    same cell count, 2 B (T - 1) S^2, in the project's most tuned kernel

With --band, the band rows alone: margins.forward_backward_max_banded against the dense route on the same inputs in the same
process, for the pitch band of --half-widths (12: 23 diagonals, 88: 175) in both forms of its background (-inf and
log(tiny)) at every batch of --batches, by the same method; the band route moves 20 B T S bytes (the observation read twice,
the marginals written, read and written again).
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torbi_amd  # noqa: E402
from torbi_amd import margins, synth  # noqa: E402

HBM_PEAK_BYTES = 8e12
CHUNK_VALUES = 1 << 28


def spread(values):
    v = sorted(values)
    return {'median': float(np.median(v)), 'min': float(v[0]), 'max': float(v[-1]), 'runs': len(v)}


def timed(fn, repeats):
    """ms of `fn` between two events on the current stream, after one warm-up call."""
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(repeats):
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        fn()
        end.record()
        end.synchronize()
        out.append(start.elapsed_time(end))
    return spread(out)


def max_plus(M, v):
    """out[b, r] = max_c (M[r, c] + v[b, c]) with torch ops, chunked over r."""
    B, S = v.shape
    out = torch.empty_like(v)
    step = max(1, min(S, CHUNK_VALUES // (B * S)))
    for r0 in range(0, S, step):
        out[:, r0:r0 + step] = (M[None, r0:r0 + step, :] + v[:, None, :]).amax(dim=2)
    return out


def torch_max_marginals(obs, trans, init):
    """The contract with torch ops (every item has all T frames)."""
    B, T, S = obs.shape
    m = torch.empty_like(obs)
    m[:, 0] = obs[:, 0] + init
    for t in range(1, T):
        m[:, t] = obs[:, t] + max_plus(trans, m[:, t - 1])
    score = m[:, T - 1].amax(dim=1)
    At = trans.t().contiguous()
    beta = torch.zeros((B, S), dtype=torch.float32, device=obs.device)
    for t in range(T - 2, -1, -1):
        beta = max_plus(At, obs[:, t + 1] + beta)
        m[:, t] += beta
    return m, score


def band_rows(T, S, repeats, batches, half_widths):
    """The band route (margins.forward_backward_max_banded) against the dense route on the same inputs in the same process:
    the pitch band of `half_width` (2 * half_width - 1 diagonals) in both forms of its background, -inf and log(tiny), at
    every batch of `batches`.  `wins`: the dense median exceeds the band median by more than the dense route's own spread
    (max - min); `equal`: the two routes' values agree by == with equal NaN positions."""
    dev = torch.device('cuda:0')
    rows = []
    for B in batches:
        obs, _, init = (torch.from_numpy(x).to(dev) for x in synth.problem(B, T, S, seed=1))
        frames = torch.full((B,), T, dtype=torch.int32, device=dev)
        dense_ws = torch.empty(margins.max_marginals_workspace_bytes(B, T, S), dtype=torch.uint8, device=dev)
        for half_width in half_widths:
            reach = half_width - 1
            band_ws = torch.empty(margins.max_marginals_banded_workspace_bytes(B, T, S, reach, reach), dtype=torch.uint8, device=dev)
            for tiny in (False, True):
                matrix = synth.banded_transition(S, half_width, tiny=tiny)
                background = float(matrix[0, S - 1])
                trans = torch.from_numpy(matrix).to(dev)
                dense = timed(lambda: margins.forward_backward_max(obs, frames, trans, init, workspace=dense_ws), repeats)
                band = timed(lambda: margins.forward_backward_max_banded(obs, frames, trans, init, reach, reach, background,
                                                                         workspace=band_ws), repeats)
                want = margins.forward_backward_max(obs, frames, trans, init, workspace=dense_ws)
                got = margins.forward_backward_max_banded(obs, frames, trans, init, reach, reach, background, workspace=band_ws)
                equal = all(bool(((g == w) | (torch.isnan(g) & torch.isnan(w))).all()) for g, w in zip(got, want))
                nan = int(torch.isnan(got[0]).sum())
                del want, got
                rows.append({'batch': B, 'diagonals': 2 * reach + 1, 'background': background, 'dense_ms': dense, 'band_ms': band,
                             'speedup': dense['median'] / band['median'], 'equal': equal, 'nan_values': nan,
                             'wins': dense['median'] - band['median'] > dense['max'] - dense['min'],
                             'band_workspace_bytes': band_ws.numel(),
                             'band_gbps_of_20_B_T_S': 20.0 * B * T * S / band['median'] / 1e6})
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--band', action='store_true', help='the band rows alone (MARGINALS.md, "Band route")')
    ap.add_argument('--batches', type=int, nargs='+', default=[1, 8, 512])
    ap.add_argument('--half-widths', type=int, nargs='+', default=[12, 88])
    ap.add_argument('--B', type=int, default=512)
    ap.add_argument('--T', type=int, default=500)
    ap.add_argument('--S', type=int, default=1440)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--torch-repeats', type=int, default=2)
    ap.add_argument('--skip-torch', action='store_true')
    args = ap.parse_args()
    B, T, S = args.B, args.T, args.S
    if args.band:
        print(json.dumps({'device': torch.cuda.get_device_name(0), 'frames_states': [T, S], 'repeats': args.repeats,
                          'band_rows': band_rows(T, S, args.repeats, args.batches, args.half_widths)}))
        return
    dev = torch.device('cuda:0')
    obs, trans, init = (torch.from_numpy(x).to(dev) for x in synth.problem(B, T, S, seed=1))
    frames = torch.full((B,), T, dtype=torch.int32, device=dev)
    ws = torch.empty(margins.max_marginals_workspace_bytes(B, T, S), dtype=torch.uint8, device=dev)
    cells = 2.0 * B * (T - 1) * S * S
    out = {'device': torch.cuda.get_device_name(0), 'shape': [B, T, S], 'workspace_bytes': ws.numel(),
           'uniform_workspace_bytes': margins.max_marginals_workspace_bytes(B, T, S, uniform=True)}

    a = timed(lambda: margins.forward_backward_max(obs, frames, trans, init, workspace=ws), args.repeats)
    out['a_dense'] = {'ms': a, 'us_per_step_launch': 1e3 * a['median'] / max(1, 2 * (T - 1)),
                      'cells_per_s': cells / (a['median'] * 1e-3)}

    band = torch.from_numpy(synth.banded_transition(S, 12)).to(dev)
    b = timed(lambda: margins.forward_backward_max(obs, frames, band, init, workspace=ws), args.repeats)
    m, _ = margins.forward_backward_max(obs, frames, band, init, workspace=ws)
    out['b_pitch_band_dense_route'] = {'ms': b, 'nan_values': int(torch.isnan(m).sum()),
                                       'minus_inf_entries_of_the_matrix': int(torch.isinf(band).sum())}
    del m

    c = timed(lambda: margins.forward_backward_max(obs, frames, None, init, workspace=ws), args.repeats)
    moved = 12.0 * B * T * S
    out['c_uniform'] = {'ms': c, 'gbps': moved / c['median'] / 1e6,
                        'fraction_of_hbm_peak': moved / (c['median'] * 1e-3) / HBM_PEAK_BYTES}

    dws = torch.empty(torbi_amd.workspace_bytes(B, T, S), dtype=torch.uint8, device=dev)
    d = timed(lambda: torbi_amd.decode(obs, frames, trans, init, workspace=dws, path='dense'), args.repeats)
    del dws
    out['every_cell_dense_decode'] = {'ms': d, 'a_over_twice_this': a['median'] / (2 * d['median'])}

    if not args.skip_torch:
        got = margins.forward_backward_max(obs, frames, trans, init, workspace=ws)
        want = torch_max_marginals(obs, trans, init)
        equal = bool(((got[0] == want[0]) | (torch.isnan(got[0]) & torch.isnan(want[0]))).all()) and bool((got[1] == want[1]).all())
        del got, want
        ref = timed(lambda: torch_max_marginals(obs, trans, init), args.torch_repeats)
        out['torch_ops'] = {'ms': ref, 'hip_values_equal_torch': equal, 'speedup_of_a': ref['median'] / a['median']}
    print(json.dumps(out))


if __name__ == '__main__':
    main()
