"""torbi_amd.forward_sample_banded / sample_paths(route=...) on an MI355X (csrc/sample_band.hpp) against the float64 band
rule, which tests/test_sample_band_cpu.py checks against the dense rule and the posteriors (SAMPLING.md, "Band route")."""
import functools
import math

import numpy as np
import pytest
import torch

import torbi_amd
from torbi_amd import synth

import sample_cases as sc
import sample_band_cases as sbc

pytestmark = pytest.mark.gpu

DEV = torch.device('cuda:0')
DRAWS = 33                      # one call with 33 draws per case; its first 1, 4, 16 and 17 draws are asked for again below
BOUND = 1e-4                    # tests/test_sample_gpu.py's: a normalised fp32 row against float64
TINY = float(np.log(np.finfo(np.float32).tiny))           # what synth.banded_transition(tiny=True) holds outside its band

# name -> (B, T, S, (reach_left, reach_right), background, matrix, lengths, initial): what each reaches is in SAMPLING.md
CASES = {
    'one_frame': (1, 1, 8, (1, 1), -math.inf, 'random', None, None),
    'asymmetric': (3, 40, 64, (2, 5), -math.inf, 'random', None, None),
    'asymmetric_finite': (3, 40, 64, (5, 2), -20., 'random', None, None),
    'one_diagonal': (17, 33, 65, (0, 0), -math.inf, 'random', None, None),
    'clipped_band': (9, 12, 37, (36, 36), -3., 'random', None, None),
    'full_wave': (2, 5, 128, (31, 32), -math.inf, 'random', None, None),
    'unaligned_rows': (5, 30, 1441, (12, 12), -math.inf, 'random', None, None),
    'pitch_inf': (4, 20, 1440, (11, 11), -math.inf, 'pitch', None, None),
    'pitch_tiny': (4, 20, 1440, (11, 11), TINY, 'pitch_tiny', None, None),
    'largest_states': (2, 3, 4096, (31, 32), -math.inf, 'random', None, None),
    'ragged': (70, 6, 257, (3, 0), -math.inf, 'random', 'ragged', None),
    'tile_2': (515, 4, 65, (2, 1), -6., 'random', None, None),
    'tile_4': (1030, 3, 37, (1, 2), -math.inf, 'random', None, None),
    'tile_8': (2050, 3, 33, (0, 3), -9., 'random', None, None),
    'starts_at_first_state': (3, 10, 64, (3, 3), -math.inf, 'random', None, 'first'),
    'starts_at_last_state': (3, 10, 64, (3, 3), -5., 'random', None, 'last'),
}


@functools.lru_cache(maxsize=None)
def inputs_of(name):
    """(obs, frames, A, pi, u) on the host, built once per case."""
    B, T, S, band, bg, matrix, lengths, initial = CASES[name]
    seed = B + T + S
    obs, A, pi = sbc.problem(B, T, S, seed, band, bg)
    if matrix.startswith('pitch'):
        A = torch.as_tensor(synth.banded_transition(S, 12, tiny=matrix == 'pitch_tiny'))
    if initial is not None:
        pi = torch.full((S,), -math.inf)
        pi[0 if initial == 'first' else S - 1] = 0.
    frames = torch.full((B,), T, dtype=torch.int32)
    if lengths == 'ragged':
        frames = (torch.arange(B, dtype=torch.int32) * 7) % T + 1          # includes 1 and T
        frames[B - 1] = T
    return obs, frames, A, pi, sc.uniforms(B, DRAWS, T, seed)


@functools.lru_cache(maxsize=None)
def reference_of(name):
    obs, frames, A, pi, _ = inputs_of(name)
    a, E, L, F = torbi_amd.sampling._filter(obs, frames, A, None, pi)
    return a, E, L, F


def run(obs, frames, A, pi, u, band, bg, workspace=None):
    out = torbi_amd.forward_sample_banded(obs.to(DEV), frames.to(DEV), A.to(DEV), pi.to(DEV), u.to(DEV), band[0], band[1], bg,
                                          workspace)
    assert out[0].dtype == torch.int32 and out[1].dtype == torch.float32 and out[0].device == DEV
    return out[0].cpu(), out[1].cpu()


def band_L(obs, frames, A, pi, band, bg):
    return torbi_amd.forward_backward_banded(obs.to(DEV), frames.to(DEV), A.to(DEV), pi.to(DEV), band[0], band[1], bg)[1].cpu()


def check_draws(label, indices, u, ref, band, bg):
    a, E, _, F = ref
    S = a.shape[2]
    assert bool(((indices >= 0) & (indices < S)).all())
    worst, behind = sbc.draw_errors(indices, u, a, E, F, band, bg)
    print(f'{label}: worst d = {worst:.3g} ({100 * worst / BOUND:.2f} % of the bound), {100 * behind:.1f} % of the draws '
          'from the whole-row part')
    assert worst <= BOUND                       # (inf where the chosen state has no slot of weight > 0)
    assert sc.tails_repeat(indices.long(), F)
    if bg == -math.inf:
        assert sbc.pairs_in_band(indices, F, band)
    return behind


@pytest.mark.parametrize('name', list(CASES))
def test_every_draw_follows_the_float64_rule(name):
    obs, frames, A, pi, u = inputs_of(name)
    band, bg = CASES[name][3], CASES[name][4]
    if name == 'one_frame':
        u = u[:, :1]
    indices, L = run(obs, frames, A, pi, u, band, bg)
    behind = check_draws(name, indices, u, reference_of(name), band, bg)
    if name == 'clipped_band':
        assert behind > 0.2                     # the whole-row part is taken often
    assert torch.equal(L, band_L(obs, frames, A, pi, band, bg))
    for n in (1, 4, 16, 17) if name != 'one_frame' else ():
        fewer, Ln = run(obs, frames, A, pi, u[:, :n], band, bg)
        assert torch.equal(fewer, indices[:, :n]) and torch.equal(Ln, L), n
    if name.startswith('starts_at'):            # the windows of the first frames are clipped at the edge the path starts at
        edge = 0 if name.endswith('first_state') else obs.shape[2] - 1
        assert bool((indices[:, :, 0] == edge).all())


def test_draws_and_items_are_independent():
    obs, frames, A, pi, u = inputs_of('tile_2')
    band, bg = CASES['tile_2'][3], CASES['tile_2'][4]
    indices, L = run(obs, frames, A, pi, u, band, bg)
    again, L2 = run(obs, frames, A, pi, u, band, bg)
    assert torch.equal(indices, again) and torch.equal(L, L2)
    one, _ = run(obs, frames, A, pi, u[:, 17:18], band, bg)
    assert torch.equal(one[:, 0], indices[:, 17])
    alone, La = run(obs[3:4], frames[3:4], A, pi, u[3:4], band, bg)          # filter tile G = 1 against G = 2
    assert torch.equal(alone[0], indices[3]) and torch.equal(La[0], L[3])
    few, Lf = run(obs[:70], frames[:70], A, pi, u[:70], band, bg)
    assert torch.equal(few, indices[:70]) and torch.equal(Lf, L[:70])


@pytest.mark.parametrize('case,seed', [(k, seed) for k, c in enumerate(sbc.FREQUENCY_CASES) for seed in c[6]])
def test_frequencies_follow_the_posteriors(case, seed):
    B, T, S, band, bg, lengths, _ = sbc.FREQUENCY_CASES[case]
    obs, A, pi = sbc.problem(B, T, S, seed, band, bg)
    frames = sc.frames_of(lengths, B, T)
    u = sc.uniforms(B, sbc.FREQUENCY_DRAWS, T, seed)
    indices, _ = run(obs, frames, A, pi, u, band, bg)
    a, E, L64, F, gamma = sc.reference(obs, frames, A, pi)
    ratio = sc.frequency_ratio(indices.long(), a, E, F, gamma)
    print(f'band frequency ratio case {case} seed {seed}: {ratio:.2f} of 5')
    assert ratio <= 5
    check_draws(f'band frequency case {case} seed {seed}', indices, u, (a, E, L64, F), band, bg)


@pytest.mark.parametrize('bg', [-math.inf, -4.])
def test_nonfinite_items_get_minus_one_and_leave_the_others_unchanged(bg):
    B, T, S, N, band = 6, 20, 300, 17, (4, 2)
    obs, A, pi = sbc.problem(B, T, S, seed=6, band=band, background=bg)
    frames = torch.tensor([20, 20, 20, 20, 20, 9], dtype=torch.int32)
    u = sc.uniforms(B, N, T, seed=6)
    clean, cleanL = run(obs, frames, A, pi, u, band, bg)
    assert bool(torch.isfinite(cleanL).all()) and bool((clean >= 0).all())
    bad = obs.clone()
    bad[1, 7, 5] = math.nan
    bad[2, 3, 200] = math.inf
    bad[3, 11, :] = -math.inf                    # a frame of probability 0
    bad[5, 12, 0] = math.nan                     # beyond the item's frames
    indices, L = run(bad, frames, A, pi, u, band, bg)
    assert math.isnan(float(L[1])) and math.isnan(float(L[2])) and float(L[3]) == -math.inf
    assert bool((indices[1:4] == -1).all())
    for b in (0, 4, 5):
        assert torch.equal(indices[b], clean[b]) and torch.equal(L[b], cleanL[b])
    Lb = band_L(bad, frames, A, pi, band, bg)
    assert torch.equal(L[[0, 3, 4, 5]], Lb[[0, 3, 4, 5]]) and bool(torch.isnan(Lb[1:3]).all())
    indices, L = run(obs, frames, A, torch.full((S,), -math.inf), u, band, bg)
    assert bool((L == -math.inf).all()) and bool((indices == -1).all())


def test_a_broken_promise_gives_nan_and_minus_one():
    obs, frames, A, pi, u = inputs_of('asymmetric_finite')
    band, bg = CASES['asymmetric_finite'][3], CASES['asymmetric_finite'][4]
    broken = A.clone()
    broken[40, 3] = -19.5                        # outside the band, and not the background
    indices, L = run(obs, frames, broken, pi, u, band, bg)
    assert bool(torch.isnan(L).all()) and bool((indices == -1).all())
    indices, L = run(obs, frames, A, pi, u, band, bg)                        # (the flag is reset by the next call)
    assert bool(torch.isfinite(L).all()) and bool((indices >= 0).all())


def test_graph_capture_replays_on_new_observations_and_uniforms():
    B, T, S, N, band, bg = 20, 25, 400, 6, (5, 7), -12.
    obs, A, pi = sbc.problem(B, T, S, seed=13, band=band, background=bg)
    obs2 = sbc.problem(B, T, S, seed=14, band=band, background=bg)[0]
    u, u2 = sc.uniforms(B, N, T, seed=13), sc.uniforms(B, N, T, seed=14)
    frames = (torch.arange(B, dtype=torch.int32) * 3) % T + 1
    tobs, tframes, tA, tpi, tu = (x.to(DEV) for x in (obs, frames, A, pi, u))
    ws = torch.empty(torbi_amd.forward_sample_banded_workspace_bytes(B, T, S, N, *band), dtype=torch.uint8, device=DEV)
    call = lambda o, x: torbi_amd.forward_sample_banded(o, tframes, tA, tpi, x, band[0], band[1], bg, workspace=ws)
    eager = [x.clone() for x in call(tobs, tu)]
    eager2 = [x.clone() for x in call(obs2.to(DEV), u2.to(DEV))]
    assert not torch.equal(eager[0], eager2[0])
    side = torch.cuda.Stream(device=DEV)
    graph = torch.cuda.CUDAGraph()
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            indices, loglik = call(tobs, tu)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(indices, eager[0]) and torch.equal(loglik, eager[1])
    tobs.copy_(obs2)
    tu.copy_(u2)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(indices, eager2[0]) and torch.equal(loglik, eager2[1])


def test_a_workspace_that_is_too_small_raises():
    obs, frames, A, pi, u = inputs_of('clipped_band')
    B, T, S = obs.shape
    band, bg = CASES['clipped_band'][3], CASES['clipped_band'][4]
    need = torbi_amd.forward_sample_banded_workspace_bytes(B, T, S, DRAWS, *band)
    with pytest.raises(RuntimeError, match='workspace'):
        run(obs, frames, A, pi, u, band, bg, workspace=torch.empty(need - 1, dtype=torch.uint8, device=DEV))
    run(obs, frames, A, pi, u, band, bg, workspace=torch.empty(need, dtype=torch.uint8, device=DEV))


def test_public_routes_on_probabilities():
    B, T, S, N = 6, 9, 360, 5
    g = torch.Generator().manual_seed(4)
    p = torch.rand(B, T, S, generator=g) ** 4
    p /= p.sum(-1, keepdim=True)
    frames = torch.tensor([9, 1, 4, 9, 2, 7], dtype=torch.int32)
    u = sc.uniforms(B, N, T, seed=4)
    trans = torch.as_tensor(synth.banded_transition(S, 12)).exp()
    args = dict(draws=N, batch_frames=frames, transition=trans, uniforms=u)
    indices, L = torbi_amd.sample_paths(p.to(DEV), gpu=0, route='band', **args)
    _, hostL = torbi_amd.sample_paths(p, **args)
    assert indices.device == DEV and indices.dtype == torch.int32 and tuple(indices.shape) == (B, N, T)
    err = torch.abs(L.cpu().double() - hostL.double())
    assert bool((err <= 1e-6 * torch.abs(hostL.double()) + 4e-6 * frames).all())
    assert bool(((indices >= 0) & (indices < S)).all())
    route = torbi_amd.sample_route(trans, B, T, S, draws=N, gpu=0)
    assert route in ('band', 'dense')
    assert torbi_amd.sample_route(None, B, T, S, draws=N, gpu=0) == 'uniform'
    auto, autoL = torbi_amd.sample_paths(p.to(DEV), gpu=0, route='auto', **args)
    dense, denseL = torbi_amd.sample_paths(p.to(DEV), gpu=0, **args)
    # 'auto' returns what sample_route named: the band route's L is forward_backward_banded's, the dense route's
    # forward_backward's, bit for bit (state_posteriors prepares the same inputs)
    named = torbi_amd.state_posteriors(p.to(DEV), frames, trans, gpu=0, route=route)[1]
    assert torch.equal(autoL, named)
    assert torch.equal(autoL, L if route == 'band' else denseL)
    assert torch.equal(auto, indices if route == 'band' else dense)
    assert torch.equal(denseL, torbi_amd.state_posteriors(p.to(DEV), frames, trans, gpu=0, route='dense')[1])
    with pytest.raises(RuntimeError, match="route='band'"):
        torbi_amd.sample_paths(p.to(DEV), gpu=0, route='band', draws=N, batch_frames=frames, uniforms=u,
                               transition=torch.rand(S, S, generator=g))
