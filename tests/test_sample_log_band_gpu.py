"""torbi_amd.forward_sample_log_banded / sample_paths(route='log-band') on an MI355X (csrc/sample_log_band.hpp) against the
float64 band rule, with the inputs of the log posterior route's tests and the checker of the band samplers' (SAMPLING.md,
"Log-space band route").  The tile rule at 256 compute units gives G = 1 below 512 items, G = 2 at 515 and G = 4 at 2050."""
import functools
import math

import pytest
import torch

import torbi_amd
from torbi_amd import inputs, synth, viterbi

import sample_cases as sc
import sample_band_cases as sbc
import test_posterior_log_band_gpu as plb

pytestmark = pytest.mark.gpu

DEV = torch.device('cuda:0')
DRAWS = 33                      # one call with 33 draws per case; its first 1, 4, 16 and 17 draws are asked for again below
BOUND = 1e-4                    # the project's bound for a normalised fp32 row against float64
NINF = -math.inf

CASES = {         # name -> (B, T, S, (reach_left, reach_right)), all -inf outside: what each reaches is in SAMPLING.md
    'wide_range_64': (3, 24, 64, (1, 1)), 'wide_range_257': (2, 40, 257, (3, 3)), 'left_to_right': (3, 50, 200, (1, 0)),
    'narrow_ragged': (3, 40, 64, (2, 5)), 'zero_reach': (17, 33, 65, (0, 0)),
    'one_round': (2, 8, 520, (126, 126)), 'two_rounds': (2, 8, 520, (126, 127)),            # W + 3 = 256, 257
    'widest': (2, 4, 1024, (255, 256)),                                                     # W = 512: three rounds
    'unaligned_rows': (3, 10, 257, (40, 30)), 'unaligned_pitch_size': (2, 8, 1441, (87, 87)),   # the scalar-load arm
    'clipped_band': (9, 12, 100, (99, 99)), 'largest_states': (2, 3, 4096, (40, 40)),
    'tile_2': (515, 4, 65, (2, 1)), 'tile_4': (2050, 3, 33, (0, 3)),                        # G = 2, 4: a partial last tile
}
WIDE_RANGE = ('wide_range_64', 'wide_range_257', 'left_to_right')


@functools.lru_cache(maxsize=None)
def case(name):               # ((obs, frames, A, pi, u) on the host, band, the float64 filter (a, E, L, F)), built once
    B, T, S, band = CASES[name]
    if name in WIDE_RANGE or name in ('narrow_ragged', 'zero_reach'):
        obs, frames, A, pi = (torch.from_numpy(x.copy()) for x in plb.problem(B, T, S, *band, NINF))
    else:
        obs, A, pi = sbc.problem(B, T, S, B + T + S, band)
        frames = torch.full((B,), T, dtype=torch.int32)
    return (obs, frames, A, pi, sc.uniforms(B, DRAWS, T, B + T + S)), band, torbi_amd.sampling._filter(obs, frames, A, None, pi)


def run(obs, frames, A, pi, u, band):
    out = torbi_amd.forward_sample_log_banded(obs.to(DEV), frames.to(DEV), A.to(DEV), pi.to(DEV), u.to(DEV), *band)
    assert out[0].dtype == torch.int32 and out[1].dtype == torch.float32 and out[0].device == DEV
    return out[0].cpu(), out[1].cpu()


@pytest.mark.parametrize('name', list(CASES))
def test_every_draw_follows_the_float64_rule(name):
    (obs, frames, A, pi, u), band, (a, E, L64, F) = case(name)
    indices, L = run(obs, frames, A, pi, u, band)
    assert bool(torch.isfinite(L64).all()) and bool(((indices >= 0) & (indices < a.shape[2])).all())
    worst, _ = sbc.draw_errors(indices, u, a, E, F, band, NINF)
    print(f'{name}: worst d = {worst:.3g} ({100 * worst / BOUND:.2f} % of the bound)')
    assert worst <= BOUND                       # (inf where the chosen state has no slot of weight > 0)
    assert sc.tails_repeat(indices.long(), F) and sbc.pairs_in_band(indices, F, band)
    assert torch.equal(L, torbi_amd.forward_backward_log_banded(*(x.to(DEV) for x in (obs, frames, A, pi)), *band)[1].cpu())
    for n in (1, 4, 16, 17):
        fewer, Ln = run(obs, frames, A, pi, u[:, :n], band)
        assert torch.equal(fewer, indices[:, :n]) and torch.equal(Ln, L), n
    if name == 'left_to_right':                 # from state 0, never a step back
        assert bool((indices[:, :, 0] == 0).all()) and bool((indices[:, :, 1:] >= indices[:, :, :-1]).all())


def test_draws_and_items_are_independent():
    (obs, frames, A, pi, u), band, _ = case('tile_2')
    indices, L = run(obs, frames, A, pi, u, band)
    alone, La = run(obs[3:4], frames[3:4], A, pi, u[3:4], band)              # filter tile G = 1 against G = 2
    assert torch.equal(alone[0], indices[3]) and torch.equal(La[0], L[3])
    few, Lf = run(obs[:70], frames[:70], A, pi, u[:70], band)
    assert torch.equal(few, indices[:70]) and torch.equal(Lf, L[:70])


def test_nonfinite_items_get_minus_one_and_leave_the_others_unchanged():
    B, T, S, N, band = 6, 20, 300, 17, (50, 40)
    obs, A, pi = sbc.problem(B, T, S, seed=6, band=band)
    frames, u = torch.full((B,), T, dtype=torch.int32), sc.uniforms(B, N, T, seed=6)
    clean, cleanL = run(obs, frames, A, pi, u, band)
    assert bool(torch.isfinite(cleanL).all()) and bool((clean >= 0).all())
    bad = obs.clone()
    bad[1, 7, 5] = math.nan
    bad[2, 3, 200] = math.inf
    bad[3, 11, :] = NINF                         # a frame of probability 0
    indices, L = run(bad, frames, A, pi, u, band)
    assert math.isnan(float(L[1])) and math.isnan(float(L[2])) and float(L[3]) == NINF and bool((indices[1:4] == -1).all())
    for b in (0, 4, 5):
        assert torch.equal(indices[b], clean[b]) and torch.equal(L[b], cleanL[b])


def test_a_broken_promise_gives_nan_and_minus_one():
    (obs, frames, A, pi, u), band, _ = case('unaligned_rows')
    broken = A.clone()
    broken[200, 3] = -19.5                       # outside the band, and not -inf
    indices, L = run(obs, frames, broken, pi, u, band)
    assert bool(torch.isnan(L).all()) and bool((indices == -1).all())
    indices, L = run(obs, frames, A, pi, u, band)                            # (the flag is reset by the next call)
    assert bool(torch.isfinite(L).all()) and bool((indices >= 0).all())


def test_caller_owned_workspace_and_graph_replay():
    """A workspace of stale 0xFF bytes, one byte short, and a captured call replayed on new observations and uniforms."""
    B, T, S, N, band = 20, 25, 400, 6, (50, 70)
    (obs, A, pi), obs2 = sbc.problem(B, T, S, seed=13, band=band), sbc.problem(B, T, S, seed=14, band=band)[0]
    u, u2 = sc.uniforms(B, N, T, seed=13), sc.uniforms(B, N, T, seed=14)
    frames = (torch.arange(B, dtype=torch.int32) * 3) % T + 1
    tobs, tframes, tA, tpi, tu = (x.to(DEV) for x in (obs, frames, A, pi, u))
    need = torbi_amd.forward_sample_log_banded_workspace_bytes(B, T, S, N, *band)
    ws = torch.full((need,), 0xFF, dtype=torch.uint8, device=DEV)
    call = lambda o, x, w=ws: torbi_amd.forward_sample_log_banded(o, tframes, tA, tpi, x, *band, NINF, workspace=w)
    with pytest.raises(RuntimeError, match='workspace'):
        call(tobs, tu, ws[:need - 1])
    eager = [x.clone() for x in call(tobs, tu)]
    assert torch.equal(eager[0], torbi_amd.forward_sample_log_banded(tobs, tframes, tA, tpi, tu, *band)[0])
    eager2 = [x.clone() for x in call(obs2.to(DEV), u2.to(DEV))]
    side, graph = torch.cuda.Stream(device=DEV), torch.cuda.CUDAGraph()
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


def test_sample_paths_on_probabilities():
    B, T, S, N = 6, 9, 360, 5
    p = torch.rand(B, T, S, generator=torch.Generator().manual_seed(4)) ** 4
    p /= p.sum(-1, keepdim=True)
    frames, u = torch.tensor([9, 1, 4, 9, 2, 7], dtype=torch.int32), sc.uniforms(B, N, T, seed=4)
    trans = torch.as_tensor(synth.banded_transition(S, 40)).exp()            # 79 diagonals, 0 outside
    x = inputs.observation(p.to(DEV), False, DEV)                            # what the operator level is handed
    A, _, pi = inputs.model(trans, None, False, S, DEV, plain=True)
    want = torbi_amd.forward_sample_log_banded(x, frames.to(DEV), A, pi, u.to(DEV), *viterbi.band_over(A, A, S))
    got = torbi_amd.sample_paths(p.to(DEV), N, frames, trans, gpu=0, uniforms=u, route='log-band')
    assert bool((want[0] >= 0).all()) and torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
