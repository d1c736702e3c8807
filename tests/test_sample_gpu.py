"""torbi_amd.forward_sample / sample_paths on an MI355X (csrc/sample.hpp) against the float64 draw rule, which
tests/test_sample_cpu.py checks against enumeration and the posteriors (SAMPLING.md)."""
import functools
import math

import pytest
import torch

import torbi_amd
from torbi_amd import synth

import sample_cases as sc

pytestmark = pytest.mark.gpu

DEV = torch.device('cuda:0')
DRAWS = 33                      # one call with 33 draws per case; its first 1, 4, 16 and 17 draws are asked for again below
BOUND = 1e-4                    # the project's bound on a normalised fp32 row against float64 (test_posterior_gpu.check)

# name -> (B, T, S, matrix, lengths): what each reaches is in SAMPLING.md, "Tests"
CASES = {
    'one_frame': (1, 1, 3, 'dense', None),
    'wave_tail_64': (3, 40, 64, 'dense', None),
    'wave_tail_65': (17, 33, 65, 'dense', None),
    'partial_block': (9, 12, 37, 'dense', None),
    'pitch_plus_one': (5, 30, 1441, 'dense', None),
    'pitch_band_inf': (4, 20, 1440, 'pitch', None),
    'pitch_band_tiny': (4, 20, 1440, 'pitch_tiny', None),
    'held_float4_last': (2, 3, 4096, 'dense', None),
    'streamed_float4_first': (2, 3, 4100, 'dense', None),
    'held_scalar_last': (2, 3, 2047, 'dense', None),
    'streamed_scalar_first': (2, 3, 2049, 'dense', None),
    'long_rows': (1, 3, 4160, 'dense', None),
    'ragged': (70, 6, 257, 'dense', 'ragged'),
    'many_items': (520, 3, 33, 'dense', None),
    'zero_weights': (9, 12, 37, 'zeros', 'ragged'),
}
UNIFORM_CASES = ['one_frame', 'wave_tail_65', 'partial_block', 'pitch_band_inf', 'ragged', 'many_items',
                 ('u1441', (5, 12, 1441)), ('u4096', (5, 12, 4096)), ('u2049', (3, 4, 2049))]


@functools.lru_cache(maxsize=None)
def inputs_of(name, shape=None):
    """(obs, frames, A, pi, u) on the host, built once per case."""
    B, T, S, matrix, lengths = CASES[name] if shape is None else (*shape, 'dense', 'ragged')
    seed = B + T + S
    obs, A, pi = sc.problem(B, T, S, seed)
    if matrix.startswith('pitch'):
        A = torch.as_tensor(synth.banded_transition(S, 12, tiny=matrix == 'pitch_tiny'))
    if matrix == 'zeros':
        obs[:, :, 0] = -math.inf
        obs[:, 2, 1] = -math.inf
        pi[1] = -math.inf
    frames = torch.full((B,), T, dtype=torch.int32)
    if lengths == 'ragged':
        frames = (torch.arange(B, dtype=torch.int32) * 7) % T + 1          # includes 1 and T
        frames[B - 1] = T
    return obs, frames, A, pi, sc.uniforms(B, DRAWS, T, seed)


@functools.lru_cache(maxsize=None)
def reference_of(name, shape=None, uniform=False):
    obs, frames, A, pi, _ = inputs_of(name, shape)
    return sc.reference(obs, frames, None if uniform else A, pi)


def run(obs, frames, A, pi, u, workspace=None):
    """The device at the operator level; A = None: the uniform route on the value `sample_paths` passes."""
    if A is None:
        uniform = float(torch.tensor(math.log(1. / obs.shape[2]), dtype=torch.float32))
        out = torbi_amd.sampling._run(obs.to(DEV).contiguous(), frames.to(DEV), None, uniform, pi.to(DEV), u.to(DEV), workspace)
    else:
        out = torbi_amd.forward_sample(obs.to(DEV), frames.to(DEV), A.to(DEV), pi.to(DEV), u.to(DEV), workspace)
    assert out[0].dtype == torch.int32 and out[1].dtype == torch.float32 and out[0].device == DEV
    return out[0].cpu(), out[1].cpu()


def check_draws(label, indices, L, u, ref, S):
    a, E, L64, F, _ = ref
    assert bool(((indices >= 0) & (indices < S)).all())
    worst, positive = sc.draw_errors(indices, u, a, E, F)
    print(f'{label}: worst d = {worst:.3g} ({100 * worst / BOUND:.2f} % of the bound)')
    assert worst <= BOUND and positive
    assert sc.tails_repeat(indices.long(), F)
    return L64, F


@pytest.mark.parametrize('name', list(CASES))
def test_every_draw_follows_the_float64_rule(name):
    obs, frames, A, pi, u = inputs_of(name)
    B, T, S = obs.shape
    indices, L = run(obs, frames, A, pi, u)
    _, F = check_draws(name, indices, L, u, reference_of(name), S)
    # L: the bits of forward_backward
    _, L2 = torbi_amd.forward_backward(obs.to(DEV), frames.to(DEV), A.to(DEV), pi.to(DEV))
    assert torch.equal(L, L2.cpu())
    # a partial workgroup of draws per item (four waves: four draws), exactly one, exactly four, and four with a tail give
    # the draws of the 33-draw call (eight and a tail)
    for n in (1, 4, 16, 17) if name != 'one_frame' else (1,):
        fewer, Ln = run(obs, frames, A, pi, u[:, :n])
        assert torch.equal(fewer, indices[:, :n]) and torch.equal(Ln, L), n
    if name == 'pitch_band_inf':                                  # exact: no drawn pair is outside the band
        nxt, prv = indices[:, :, 1:].long(), indices[:, :, :-1].long()
        inner = (torch.arange(T - 1)[None, :] < (F - 1)[:, None])[:, None, :].expand_as(nxt)
        assert bool((A[nxt, prv] > -math.inf)[inner].all())
    if name == 'zero_weights':                                    # exact: states of weight 0 are never drawn
        live = (torch.arange(T)[None, :] < F[:, None])[:, None, :].expand_as(indices)
        assert bool((indices != 0)[live].all()) and bool((indices[:, :, 2] != 1)[live[:, :, 2]].all())
        assert bool((indices[:, :, 0] != 1).all())


@pytest.mark.parametrize('case', UNIFORM_CASES, ids=lambda c: c if isinstance(c, str) else c[0])
def test_uniform_route_draws_every_frame_from_its_softmax(case):
    name, shape = (case, None) if isinstance(case, str) else case
    obs, frames, _, pi, u = inputs_of(name, shape)
    S = obs.shape[2]
    indices, L = run(obs, frames, None, pi, u)
    L64, F = check_draws(f'uniform {name}', indices, L, u, reference_of(name, shape, True), S)
    err = torch.abs(L.double() - L64)
    assert bool((err <= 1e-6 * torch.abs(L64) + 4e-6 * F).all()), (err, L64)
    fewer, Ln = run(obs, frames, None, pi, u[:, :1])
    assert torch.equal(fewer, indices[:, :1]) and torch.equal(Ln, L)


def test_sample_paths_on_probabilities():
    B, T, S, N = 6, 9, 360, 5
    g = torch.Generator().manual_seed(4)
    p = torch.rand(B, T, S, generator=g) ** 4
    p /= p.sum(-1, keepdim=True)
    frames = torch.tensor([9, 1, 4, 9, 2, 7], dtype=torch.int32)
    u = sc.uniforms(B, N, T, seed=4)
    trans = torch.as_tensor(synth.banded_transition(S, 12)).exp()
    for transition in (None, trans):
        indices, L = torbi_amd.sample_paths(p.to(DEV), draws=N, batch_frames=frames, transition=transition, uniforms=u, gpu=0)
        host, hostL = torbi_amd.sample_paths(p, draws=N, batch_frames=frames, transition=transition, uniforms=u)
        assert indices.device == DEV and indices.dtype == torch.int32 and tuple(indices.shape) == (B, N, T)
        err = torch.abs(L.cpu().double() - hostL.double())
        assert bool((err <= 1e-6 * torch.abs(hostL.double()) + 4e-6 * frames).all())
        assert float((indices.cpu() == host).double().mean()) > 0.95       # (boundaries aside, the same draws)
    rand, _ = torbi_amd.sample_paths(p.to(DEV), draws=N, batch_frames=frames, transition=trans, gpu=0,
                                     generator=torch.Generator(device=DEV).manual_seed(1))
    again, _ = torbi_amd.sample_paths(p.to(DEV), draws=N, batch_frames=frames, transition=trans, gpu=0,
                                      generator=torch.Generator(device=DEV).manual_seed(1))
    assert torch.equal(rand, again) and bool(((rand >= 0) & (rand < S)).all())


@pytest.mark.parametrize('uniform', [False, True])
def test_draws_and_items_are_independent(uniform):
    obs, frames, A, pi, u = inputs_of('ragged')
    A = None if uniform else A
    indices, L = run(obs, frames, A, pi, u)
    again, L2 = run(obs, frames, A, pi, u)
    assert torch.equal(indices, again) and torch.equal(L, L2)
    one, _ = run(obs, frames, A, pi, u[:, 17:18])
    assert torch.equal(one[:, 0], indices[:, 17])
    alone, La = run(obs[3:4], frames[3:4], A, pi, u[3:4])
    assert torch.equal(alone[0], indices[3]) and torch.equal(La[0], L[3])


@pytest.mark.parametrize('case,seed', [(k, seed) for k, c in enumerate(sc.FREQUENCY_CASES) for seed in c[5]])
def test_frequencies_follow_the_posteriors(case, seed):
    B, T, S, band, lengths, _ = sc.FREQUENCY_CASES[case]
    obs, A, pi = sc.problem(B, T, S, seed, band)
    frames = sc.frames_of(lengths, B, T)
    u = sc.uniforms(B, sc.FREQUENCY_DRAWS, T, seed)
    indices, _ = run(obs, frames, A, pi, u)
    a, E, _, F, gamma = sc.reference(obs, frames, A, pi)
    ratio = sc.frequency_ratio(indices.long(), a, E, F, gamma)
    print(f'frequency ratio case {case} seed {seed}: {ratio:.2f} of 5')
    assert ratio <= 5
    check_draws(f'frequency case {case} seed {seed}', indices, None, u, (a, E, None, F, gamma), S)
    if band is not None:
        nxt, prv = indices[:, :, 1:].long(), indices[:, :, :-1].long()
        inner = (torch.arange(T - 1)[None, :] < (F - 1)[:, None])[:, None, :].expand_as(nxt)
        assert bool((A[nxt, prv] > -math.inf)[inner].all())


@pytest.mark.parametrize('uniform', [False, True])
def test_nonfinite_items_get_minus_one_and_leave_the_others_unchanged(uniform):
    B, T, S, N = 6, 20, 300, 17
    obs, A, pi = sc.problem(B, T, S, seed=6)
    A = None if uniform else A
    frames = torch.tensor([20, 20, 20, 20, 20, 9], dtype=torch.int32)
    u = sc.uniforms(B, N, T, seed=6)
    clean, cleanL = run(obs, frames, A, pi, u)
    bad = obs.clone()
    bad[1, 7, 5] = math.nan
    bad[2, 3, 200] = math.inf
    bad[3, 11, :] = -math.inf                    # a frame of probability 0
    bad[5, 12, 0] = math.nan                     # beyond the item's frames
    indices, L = run(bad, frames, A, pi, u)
    assert math.isnan(float(L[1])) and math.isnan(float(L[2])) and float(L[3]) == -math.inf
    assert bool((indices[1:4] == -1).all())
    for b in (0, 4, 5):
        assert torch.equal(indices[b], clean[b]) and torch.equal(L[b], cleanL[b])
    indices, L = run(obs, frames, A, torch.full((S,), -math.inf), u)
    assert bool((L == -math.inf).all()) and bool((indices == -1).all())


def test_graph_capture_replays_on_new_observations_and_uniforms():
    B, T, S, N = 20, 25, 400, 6
    obs, A, pi = sc.problem(B, T, S, seed=13)
    obs2 = sc.problem(B, T, S, seed=14)[0]
    u, u2 = sc.uniforms(B, N, T, seed=13), sc.uniforms(B, N, T, seed=14)
    frames = (torch.arange(B, dtype=torch.int32) * 3) % T + 1
    tobs, tframes, tA, tpi, tu = (x.to(DEV) for x in (obs, frames, A, pi, u))
    ws = torch.empty(torbi_amd.forward_sample_workspace_bytes(B, T, S, N), dtype=torch.uint8, device=DEV)
    eager = [x.clone() for x in torbi_amd.forward_sample(tobs, tframes, tA, tpi, tu, workspace=ws)]
    eager2 = [x.clone() for x in torbi_amd.forward_sample(obs2.to(DEV), tframes, tA, tpi, u2.to(DEV), workspace=ws)]
    side = torch.cuda.Stream(device=DEV)
    graph = torch.cuda.CUDAGraph()
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            indices, loglik = torbi_amd.forward_sample(tobs, tframes, tA, tpi, tu, workspace=ws)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(indices, eager[0]) and torch.equal(loglik, eager[1])
    tobs.copy_(obs2)
    tu.copy_(u2)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(indices, eager2[0]) and torch.equal(loglik, eager2[1])


def test_a_workspace_that_is_too_small_raises():
    obs, frames, A, pi, u = inputs_of('partial_block')
    B, T, S = obs.shape
    for matrix, uniform in ((A, False), (None, True)):
        need = torbi_amd.forward_sample_workspace_bytes(B, T, S, DRAWS, uniform=uniform)
        with pytest.raises(RuntimeError, match='workspace'):
            run(obs, frames, matrix, pi, u, workspace=torch.empty(need - 1, dtype=torch.uint8, device=DEV))
        run(obs, frames, matrix, pi, u, workspace=torch.empty(need, dtype=torch.uint8, device=DEV))
