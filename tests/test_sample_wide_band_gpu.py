"""torbi_amd.forward_sample_wide_banded / sample_paths(route=...) on an MI355X (csrc/sample_wide_band.hpp) against the float64
band rule, with the inputs and the checker of the narrow route's tests (SAMPLING.md, "Wide band route")."""
import functools
import math

import numpy as np
import pytest
import torch

import torbi_amd
from torbi_amd import inputs, synth, viterbi

import sample_cases as sc
import sample_band_cases as sbc

pytestmark = pytest.mark.gpu

DEV = torch.device('cuda:0')
DRAWS = 33                      # one call with 33 draws per case; its first 1, 4, 16 and 17 draws are asked for again below
BOUND = 1e-4                    # the project's bound for a normalised fp32 row against float64
NINF = -math.inf
TINY = float(np.log(np.finfo(np.float32).tiny))           # what synth.banded_transition(tiny=True) holds outside its band

# name -> (B, T, S, (reach_left, reach_right), background, matrix, lengths, initial): what each reaches is in SAMPLING.md
CASES = {
    'first_wide_width': (3, 12, 128, (32, 32), NINF, 'random', None, None),
    'asymmetric_finite': (3, 20, 300, (70, 9), -20., 'random', None, None),
    'mirrored': (3, 20, 300, (9, 70), NINF, 'random', None, None),
    'one_round': (2, 8, 520, (126, 126), NINF, 'random', None, None),                 # W = 253: W + 3 = 256
    'two_rounds': (2, 8, 520, (126, 127), -12., 'random', None, None),                # W = 254
    'widest': (2, 4, 1024, (255, 256), NINF, 'random', None, None),                   # W = 512: three rounds
    'below_widest': (2, 4, 1024, (255, 255), -9., 'random', None, None),              # W = 511
    'clipped_band': (9, 12, 100, (99, 99), -3., 'random', None, None),
    'narrow_band': (3, 40, 64, (2, 5), NINF, 'random', None, None),
    'unaligned_rows': (3, 10, 257, (40, 30), -6., 'random', None, None),
    'unaligned_pitch_size': (2, 8, 1441, (87, 87), NINF, 'random', None, None),
    'pitch_inf': (4, 20, 1440, (87, 87), NINF, 'pitch', None, None),
    'pitch_tiny': (4, 20, 1440, (87, 87), TINY, 'pitch_tiny', None, None),
    'largest_states': (2, 3, 4096, (40, 40), NINF, 'random', None, None),
    'ragged': (70, 6, 257, (40, 30), NINF, 'random', 'ragged', None),
    'tile_2': (515, 4, 68, (33, 33), -6., 'random', None, None),
    'tile_4': (1030, 3, 68, (30, 36), NINF, 'random', None, None),
    'starts_at_first_state': (3, 10, 200, (40, 40), NINF, 'random', None, 'first'),
    'starts_at_last_state': (3, 10, 200, (40, 40), -5., 'random', None, 'last'),
}


@functools.lru_cache(maxsize=None)
def case(name):
    """((obs, frames, A, pi, u) on the host, band, background, the float64 filter (a, E, L, F)), built once per case."""
    B, T, S, band, bg, matrix, lengths, initial = CASES[name]
    obs, A, pi = sbc.problem(B, T, S, B + T + S, band, bg)
    if matrix.startswith('pitch'):
        A = torch.as_tensor(synth.banded_transition(S, 87.2, tiny=matrix == 'pitch_tiny'))
    if initial is not None:
        pi = torch.full((S,), NINF)
        pi[0 if initial == 'first' else S - 1] = 0.
    frames = torch.full((B,), T, dtype=torch.int32)
    if lengths == 'ragged':
        frames = (torch.arange(B, dtype=torch.int32) * 7) % T + 1          # includes 1 and T
        frames[B - 1] = T
    return (obs, frames, A, pi, sc.uniforms(B, DRAWS, T, B + T + S)), band, bg, torbi_amd.sampling._filter(obs, frames, A, None, pi)


def run(obs, frames, A, pi, u, band, bg, workspace=None):
    out = torbi_amd.forward_sample_wide_banded(obs.to(DEV), frames.to(DEV), A.to(DEV), pi.to(DEV), u.to(DEV), *band, bg, workspace)
    assert out[0].dtype == torch.int32 and out[1].dtype == torch.float32 and out[0].device == DEV
    return out[0].cpu(), out[1].cpu()


def wide_L(obs, frames, A, pi, band, bg):
    return torbi_amd.forward_backward_wide_banded(obs.to(DEV), frames.to(DEV), A.to(DEV), pi.to(DEV), *band, bg)[1].cpu()


def check_draws(label, indices, u, ref, band, bg):
    a, E, _, F = ref
    assert bool(((indices >= 0) & (indices < a.shape[2])).all())
    worst, behind = sbc.draw_errors(indices, u, a, E, F, band, bg)
    print(f'{label}: worst d = {worst:.3g} ({100 * worst / BOUND:.2f} % of the bound), {100 * behind:.1f} % of the draws '
          'from the whole-row part')
    assert worst <= BOUND                       # (inf where the chosen state has no slot of weight > 0)
    assert sc.tails_repeat(indices.long(), F)
    assert bg != NINF or sbc.pairs_in_band(indices, F, band)
    return behind


@pytest.mark.parametrize('name', list(CASES))
def test_every_draw_follows_the_float64_rule(name):
    (obs, frames, A, pi, u), band, bg, ref = case(name)
    indices, L = run(obs, frames, A, pi, u, band, bg)
    behind = check_draws(name, indices, u, ref, band, bg)
    assert name != 'clipped_band' or behind > 0.2                            # the whole-row part is taken often
    assert torch.equal(L, wide_L(obs, frames, A, pi, band, bg))
    for n in (1, 4, 16, 17):
        fewer, Ln = run(obs, frames, A, pi, u[:, :n], band, bg)
        assert torch.equal(fewer, indices[:, :n]) and torch.equal(Ln, L), n
    if name.startswith('starts_at'):            # the windows of the first frames are clipped at the edge the path starts at
        assert bool((indices[:, :, 0] == (0 if name.endswith('first_state') else obs.shape[2] - 1)).all())


def test_draws_and_items_are_independent():
    (obs, frames, A, pi, u), band, bg, _ = case('tile_2')
    indices, L = run(obs, frames, A, pi, u, band, bg)
    again, L2 = run(obs, frames, A, pi, u, band, bg)
    assert torch.equal(indices, again) and torch.equal(L, L2)
    one, _ = run(obs, frames, A, pi, u[:, 17:18], band, bg)
    assert torch.equal(one[:, 0], indices[:, 17])
    alone, La = run(obs[3:4], frames[3:4], A, pi, u[3:4], band, bg)          # filter tile G = 1 against G = 2
    assert torch.equal(alone[0], indices[3]) and torch.equal(La[0], L[3])
    few, Lf = run(obs[:70], frames[:70], A, pi, u[:70], band, bg)
    assert torch.equal(few, indices[:70]) and torch.equal(Lf, L[:70])


@pytest.mark.parametrize('k,seed', [(k, seed) for k, c in enumerate(sbc.FREQUENCY_CASES) for seed in c[6]])
def test_frequencies_follow_the_posteriors(k, seed):
    B, T, S, band, bg, lengths, _ = sbc.FREQUENCY_CASES[k]
    obs, A, pi = sbc.problem(B, T, S, seed, band, bg)
    frames = sc.frames_of(lengths, B, T)
    u = sc.uniforms(B, sbc.FREQUENCY_DRAWS, T, seed)
    indices, _ = run(obs, frames, A, pi, u, band, bg)
    a, E, L64, F, gamma = sc.reference(obs, frames, A, pi)
    ratio = sc.frequency_ratio(indices.long(), a, E, F, gamma)
    print(f'wide band frequency ratio case {k} seed {seed}: {ratio:.2f} of 5')
    assert ratio <= 5
    check_draws(f'wide band frequency case {k} seed {seed}', indices, u, (a, E, L64, F), band, bg)


@pytest.mark.parametrize('bg', [NINF, -4.])
def test_nonfinite_items_get_minus_one_and_leave_the_others_unchanged(bg):
    B, T, S, N, band = 6, 20, 300, 17, (50, 40)
    obs, A, pi = sbc.problem(B, T, S, seed=6, band=band, background=bg)
    frames = torch.tensor([20, 20, 20, 20, 20, 9], dtype=torch.int32)
    u = sc.uniforms(B, N, T, seed=6)
    clean, cleanL = run(obs, frames, A, pi, u, band, bg)
    assert bool(torch.isfinite(cleanL).all()) and bool((clean >= 0).all())
    bad = obs.clone()
    bad[1, 7, 5] = math.nan
    bad[2, 3, 200] = math.inf
    bad[3, 11, :] = NINF                         # a frame of probability 0
    bad[5, 12, 0] = math.nan                     # beyond the item's frames
    indices, L = run(bad, frames, A, pi, u, band, bg)
    assert math.isnan(float(L[1])) and math.isnan(float(L[2])) and float(L[3]) == NINF
    assert bool((indices[1:4] == -1).all())
    for b in (0, 4, 5):
        assert torch.equal(indices[b], clean[b]) and torch.equal(L[b], cleanL[b])
    Lw = wide_L(bad, frames, A, pi, band, bg)
    assert torch.equal(L[[0, 3, 4, 5]], Lw[[0, 3, 4, 5]]) and bool(torch.isnan(Lw[1:3]).all())


def test_a_broken_promise_gives_nan_and_minus_one():
    (obs, frames, A, pi, u), band, bg, _ = case('asymmetric_finite')
    broken = A.clone()
    broken[200, 3] = -19.5                       # outside the band, and not the background
    indices, L = run(obs, frames, broken, pi, u, band, bg)
    assert bool(torch.isnan(L).all()) and bool((indices == -1).all())
    indices, L = run(obs, frames, A, pi, u, band, bg)                        # (the flag is reset by the next call)
    assert bool(torch.isfinite(L).all()) and bool((indices >= 0).all())


def test_graph_capture_replays_on_new_observations_and_uniforms():
    B, T, S, N, band, bg = 20, 25, 400, 6, (50, 70), -12.
    obs, A, pi = sbc.problem(B, T, S, seed=13, band=band, background=bg)
    obs2 = sbc.problem(B, T, S, seed=14, band=band, background=bg)[0]
    u, u2 = sc.uniforms(B, N, T, seed=13), sc.uniforms(B, N, T, seed=14)
    frames = (torch.arange(B, dtype=torch.int32) * 3) % T + 1
    tobs, tframes, tA, tpi, tu = (x.to(DEV) for x in (obs, frames, A, pi, u))
    ws = torch.empty(torbi_amd.forward_sample_wide_banded_workspace_bytes(B, T, S, N, *band), dtype=torch.uint8, device=DEV)
    call = lambda o, x: torbi_amd.forward_sample_wide_banded(o, tframes, tA, tpi, x, *band, bg, workspace=ws)
    eager = [x.clone() for x in call(tobs, tu)]
    eager2 = [x.clone() for x in call(obs2.to(DEV), u2.to(DEV))]
    assert not torch.equal(eager[0], eager2[0])
    side = torch.cuda.Stream(device=DEV)
    graph = torch.cuda.CUDAGraph()
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            indices, loglik = call(tobs, tu)
    for want in (eager, eager, eager2):          # two replays on the captured inputs, then one on new ones
        if want is eager2:
            tobs.copy_(obs2)
            tu.copy_(u2)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(indices, want[0]) and torch.equal(loglik, want[1])


def test_a_workspace_one_byte_short_raises():
    (obs, frames, A, pi, u), band, bg, _ = case('clipped_band')
    need = torbi_amd.forward_sample_wide_banded_workspace_bytes(*obs.shape, DRAWS, *band)
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
    trans = torch.as_tensor(synth.banded_transition(S, 40)).exp()            # 79 diagonals: beyond the narrow route
    x = inputs.observation(p.to(DEV), False, DEV)                            # what the operator level is handed
    A, _, pi = inputs.model(trans, None, False, S, DEV, plain=True)
    left, right, background = viterbi.band_over(A, A, S)
    assert left + right + 1 > 64
    want = {'band': torbi_amd.forward_sample_wide_banded(x, frames.to(DEV), A, pi, u.to(DEV), left, right, background),
            'dense': torbi_amd.forward_sample(x, frames.to(DEV), A, pi, u.to(DEV))}
    want['auto'] = want[torbi_amd.sample_route(trans, B, T, S, draws=N, gpu=0)]
    assert bool((want['band'][0] >= 0).all())
    for route in ('band', 'dense', 'auto'):
        got = torbi_amd.sample_paths(p.to(DEV), N, frames, trans, gpu=0, uniforms=u, route=route)
        assert torch.equal(got[0], want[route][0]) and torch.equal(got[1], want[route][1]), route
