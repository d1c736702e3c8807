"""The log-space band route of path entropy on an MI355X (csrc/path_entropy_log_band.hpp behind
torbi_hip_path_entropy_log_band, entropy.forward_entropy_log_banded and path_entropy(arithmetic='log')) against a plain float64
log-space entropy over the FULL matrix, on entropy, every prefix entry and the log-likelihood.

Bounds: the band routes' 4e-5 |ref| + 4e-5 F on H and on prefix_t (F = t + 1), POSTERIOR.md's 1e-6 |ref| + 4e-6 F on L; L also
equals `forward_backward_log_banded`'s bit for bit.  `check` prints the worst share of each bound before it asserts; ENTROPY.md,
"Log-space band route", has the table.

pe_log_band_kernel<G> is instantiated for G = 1 and 2 (4 needs scratch).  On 256 compute units 515 items run G = 2 with a last
tile of one item, every smaller case G = 1."""
import functools
import math

import numpy as np
import pytest
import torch

import torbi_amd
from torbi_amd import _lib, entropy, inputs, synth, viterbi

from test_posterior_log_band_gpu import WIDE_RANGE, problem as posterior_problem
from workspace_cases import DEV, assert_guards_intact, assert_same_bits, guarded

pytestmark = pytest.mark.gpu
NINF = -math.inf

# B, T, S, reach_left, reach_right, -inf outside; inputs of tests/test_posterior_log_band_gpu.py::problem
MODERATE = [(1, 1, 8, 1, 1),                       # one frame reads no matrix entry
            (3, 40, 64, 2, 5),                     # asymmetric reaches, ragged lengths
            (17, 33, 65, 0, 0),                    # zero reach
            (5, 30, 1441, 12, 12),                 # odd S, unaligned rows
            (2, 30, 300, 87, 87),                  # 175 diagonals: several dquads and slices
            (2, 6, 4096, 255, 256),                # W = 512, the limit
            (515, 4, 65, 2, 1)]                    # G = 2 and a partial last tile
# where the scaled routes fail (ENTROPY.md, "Where float32 is not enough"): (scale of randn, ...) on synth.banded_transition(S,
# reach + 1), generator seed 5; and the left-to-right case of WIDE_RANGE
WIDE = [(40, 2, 40, 257, 3, 3), (30, 2, 60, 512, 2, 2), (None,) + WIDE_RANGE[3][:5]]


@functools.lru_cache(maxsize=None)
def problem(case):
    """(observation, frames, transition, initial) of one case on the device."""
    if len(case) == 5 or case[0] is None:
        arrays = posterior_problem(*case[-5:], NINF)
    else:
        scale, B, T, S, left, _ = case
        g = torch.Generator().manual_seed(5)
        obs = torch.log_softmax(scale * torch.randn(B, T, S, generator=g), 2).numpy()
        init = torch.log_softmax(torch.randn(S, generator=g), 0).numpy()
        arrays = (obs, np.full(B, T, dtype=np.int32), synth.banded_transition(S, left + 1), init)
    return tuple(torch.from_numpy(np.array(a)).to(DEV) for a in arrays)


def log_space(obs, frames, A, pi):
    """(H, L, prefix) in float64 log space with plain torch ops over the full matrix, where the inputs are; prefix entries
    t >= F are 0."""
    obs, A, pi = obs.double(), A.double(), pi.double()
    B, T, S = obs.shape
    F = frames.long().clamp(1, T)
    zero = torch.zeros((), dtype=torch.float64, device=obs.device)
    la, h = pi + obs[:, 0], torch.zeros_like(obs[:, 0])
    rows, logz = torch.zeros_like(obs[:, :, 0]), torch.zeros_like(obs[:, :, 0])
    for t in range(T):
        if t > 0:
            e = A[None] + la[:, None, :]                                  # (B, next, prev)
            lse = torch.logsumexp(e, 2)
            logq = torch.where(e == NINF, zero, e - lse[..., None])       # (a term with q = 0 contributes 0)
            h = (torch.where(e == NINF, zero, logq.exp()) * (h[:, None, :] - logq)).sum(2)
            la = obs[:, t] + lse
        logz[:, t] = torch.logsumexp(la, 1)
        logp = torch.where(la == NINF, zero, la - logz[:, t, None])
        rows[:, t] = (torch.where(la == NINF, zero, logp.exp()) * (h - logp)).sum(1)
    rows = torch.where(torch.arange(T, device=obs.device)[None, :] < F[:, None], rows, zero)
    at = torch.arange(B, device=obs.device)
    return rows[at, F - 1].cpu(), logz[at, F - 1].cpu(), rows.cpu()


@functools.lru_cache(maxsize=None)
def reference(case):
    return log_space(*problem(case))


def band_of(case):
    return case[-2], case[-1], NINF


def log_band(obs, frames, A, pi, case, workspace=None, prefix=True):
    out = entropy.forward_entropy_log_banded(obs, frames, A, pi, *band_of(case), workspace=workspace, prefix=prefix)
    assert all(x.device == DEV and x.dtype == torch.float32 for x in out)
    return tuple(x.cpu() for x in out)


def check(got, want, frames, what):
    """The bounds of the module's docstring, every worst share printed first."""
    T = got[2].shape[1]
    F = frames.cpu().long().clamp(1, T)
    steps = torch.arange(1, T + 1, dtype=torch.float64)[None, :].expand_as(want[2])
    shares = {}
    for name, g, w, scale, per_frame, n in (('H', got[0], want[0], 4e-5, 4e-5, F), ('L', got[1], want[1], 1e-6, 4e-6, F),
                                            ('prefix', got[2], want[2], 4e-5, 4e-5, steps)):
        assert not torch.isnan(g).any(), name
        shares[name] = float(((g.double() - w).abs() / (scale * w.abs() + per_frame * n)).max())
    print(what, ' '.join(f'{name} {share:.4f} of its bound' for name, share in shares.items()))
    assert all(share <= 1 for share in shares.values()), shares
    assert all((got[2][b, F[b]:] == 0).all() for b in range(len(F)))


@pytest.mark.parametrize('case', MODERATE + WIDE, ids=lambda c: '-'.join(map(str, c)))
def test_against_float64_log_space(case):
    B, T, S = case[-5:-2]
    obs, frames, A, pi = problem(case)
    if B == 515 and _lib.load().torbi_hip_compute_units(0) == 256:
        assert _lib.load().torbi_hip_path_entropy_log_band_tile(B, S, case[-2], case[-1], 0) == 2
    got = log_band(obs, frames, A, pi, case)
    assert got[0].shape == got[1].shape == (B,) and got[2].shape == (B, T)
    check(got, reference(case), frames, case)
    assert torch.equal(got[1], torbi_amd.forward_backward_log_banded(obs, frames, A, pi, *band_of(case))[1].cpu())
    assert_same_bits(log_band(obs, frames, A, pi, case, prefix=False), got[:2], 'without the prefix output')


def test_an_item_s_bits_depend_neither_on_its_tile_nor_on_the_batch():
    case = MODERATE[-1]
    obs, frames, A, pi = problem(case)
    whole = log_band(obs, frames, A, pi, case)                           # G = 2; item 514 sits alone in the last tile
    for rows in (slice(0, 1), slice(514, 515)):                           # G = 1: each alone
        assert_same_bits(log_band(obs[rows], frames[rows], A, pi, case), tuple(x[rows] for x in whole), rows)


@pytest.mark.parametrize('value', [math.nan, math.inf, 'no state is possible'])
def test_a_nonfinite_item_keeps_to_itself(value):
    case = MODERATE[1]
    obs, frames, A, pi = problem(case)                                   # frames 40, 1, 2
    clean = log_band(obs, frames, A, pi, case)
    bad = obs.clone()
    if isinstance(value, str):
        bad[0, 17] = NINF                                                 # a frame of probability 0
    else:
        bad[0, 17, 9] = value
    H, L, prefix = got = log_band(bad, frames, A, pi, case)
    assert torch.isnan(H[0]) and torch.isnan(prefix[0]).all() and (L[0] == NINF if isinstance(value, str) else torch.isnan(L[0]))
    assert_same_bits(tuple(x[1:] for x in got), tuple(x[1:] for x in clean), 'the neighbours')


def test_a_broken_promise_is_nan_and_the_next_call_is_clean():
    case = MODERATE[1]
    obs, frames, A, pi = problem(case)
    ws = torch.empty(entropy.path_entropy_log_banded_workspace_bytes(*case), dtype=torch.uint8, device=DEV)
    clean = log_band(obs, frames, A, pi, case, workspace=ws)
    stray = A.clone()
    stray[60, 3] = -1.0                                                   # outside the stated band, not -inf
    H, L, prefix = log_band(obs, frames, stray, pi, case, workspace=ws)
    F = frames.cpu().long().clamp(1, case[1])
    assert torch.isnan(H).all() and torch.isnan(L).all()
    assert all(torch.isnan(prefix[b, :F[b]]).all() and (prefix[b, F[b]:] == 0).all() for b in range(case[0]))
    assert_same_bits(log_band(obs, frames, A, pi, case, workspace=ws), clean, 'the call after the broken one')


def test_a_caller_owned_workspace_of_exactly_the_queried_bytes():
    case = MODERATE[1]
    obs, frames, A, pi = problem(case)
    need = entropy.path_entropy_log_banded_workspace_bytes(*case)
    with pytest.raises(RuntimeError, match='workspace'):
        log_band(obs, frames, A, pi, case, workspace=torch.empty(need - 1, dtype=torch.uint8, device=DEV))
    ws = guarded(need, offset=1, fill=0xFF)
    for prefix in (True, False):                                          # (without: the prefix rows live in the workspace)
        assert_same_bits(log_band(obs, frames, A, pi, case, workspace=ws, prefix=prefix),
                         log_band(obs, frames, A, pi, case, prefix=prefix), 'a stale, odd-based workspace')
    assert_guards_intact(ws)


def test_path_entropy_takes_the_route_and_says_what_it_cannot_serve():
    case = MODERATE[1]
    o, f, a, p = (x.cpu() for x in problem(case))
    trans, uniform, init = inputs.model(a, p, True, case[2], DEV, plain=True)
    band = viterbi.band_over(trans, trans, case[2])
    assert uniform is None and tuple(band) == band_of(case)
    for prefix in (True, False):
        got = entropy.path_entropy(o, f, a, p, log_probs=True, gpu=0, prefix=prefix, route='band', arithmetic='log')
        want = entropy.forward_entropy_log_banded(inputs.observation(o, True, DEV), f, trans, init, *band, prefix=prefix)
        assert_same_bits(tuple(x.cpu() for x in got), tuple(x.cpu() for x in want), f'prefix={prefix}')
    finite = torch.where(a == NINF, torch.tensor(-20.), a)
    bandless = -torch.rand(320, 320)                                      # dense: no band of up to 512 entries
    for matrix, observation, route in ((a, o, 'dense'), (finite, o, 'band'), (bandless, -torch.rand(1, 2, 320), 'auto')):
        with pytest.raises(RuntimeError, match='band route only.*gpu=None'):
            entropy.path_entropy(observation, None, matrix, log_probs=True, gpu=0, route=route, arithmetic='log')
