"""The five `route=` arguments on an MI355X, at the smallest shape `viterbi.band_over` answers for (64 states): which route
'auto' takes for three matrices, that `route='band'` is the stated-band entry called with the band `band_over` reports, and
that `route='dense'` is the dense entry -- bit for bit.  The expected routes were recorded from the commit before the band
planner (torbi_amd/band_route.py) existed; the file passes there unchanged."""
import math

import numpy as np
import pytest
import torch

import torbi_amd
from torbi_amd import inputs

pytestmark = pytest.mark.gpu

DEV = torch.device('cuda', 0)
B, T, S, K, DRAWS = 2, 5, 64, 2, 1
NINF = -math.inf
# name -> (reach_left, reach_right, background); the entries inside the band are standard normal, far above -20
MATRICES = {'inf': (1, 1, NINF), 'finite': (1, 1, -20.), 'diagonal': (0, 0, NINF)}
# what 'auto' takes: (posterior_route, counts_route, sample_route, k_best_route, stream_route)
ROUTES = {'inf': ('band', 'band', 'dense', 'band', 'band'),
          'finite': ('band', 'dense', 'dense', 'band', 'band'),
          'diagonal': ('band', 'band', 'band', 'band', 'band')}


class Case:
    def __init__(self, name):
        left, right, background = MATRICES[name]
        rng = np.random.default_rng(5)
        trans = rng.standard_normal((S, S)).astype(np.float32)
        j, i = np.meshgrid(np.arange(S), np.arange(S), indexing='ij')           # [next j, prev i]
        trans[(i < j - left) | (i > j + right)] = background
        self.band = (left, right, background)
        self.A = torch.tensor(trans, device=DEV)
        self.pi = torch.tensor(rng.standard_normal(S).astype(np.float32), device=DEV)
        self.obs = torch.tensor(rng.standard_normal((B, T, S)).astype(np.float32), device=DEV)
        self.frames = torch.tensor([T, 3], dtype=torch.int32, device=DEV)
        self.u = torch.tensor(rng.random((B, DRAWS, T)).astype(np.float32), device=DEV)
        self.x = inputs.observation(self.obs, True, DEV)                         # what the operator level is handed
        self.model = dict(batch_frames=self.frames, transition=self.A, initial=self.pi, log_probs=True, gpu=0)


@pytest.fixture(scope='module', params=list(MATRICES))
def case(request):
    return request.param, Case(request.param)


def same(got, want):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert g.dtype == w.dtype and g.shape == w.shape
        assert torch.equal(g.view(torch.int32), w.view(torch.int32))


def test_auto_routes(case):
    name, c = case
    got = (torbi_amd.posterior_route(c.A, B, T, S, gpu=0, log_probs=True),
           torbi_amd.counts_route(c.A, B, T, S, gpu=0, log_probs=True),
           torbi_amd.sample_route(c.A, B, T, S, draws=DRAWS, gpu=0, log_probs=True),
           torbi_amd.k_best_route(c.A, B, T, S, K, gpu=0, log_probs=True),
           torbi_amd.stream_route(c.A, B, S, gpu=0, log_probs=True))
    print(name, got)
    assert torbi_amd.viterbi.band_over(c.A, c.A, S) == c.band
    assert got == ROUTES[name]


def test_posteriors(case):
    _, c = case
    left, right, background = torbi_amd.viterbi.band_over(c.A, c.A, S)
    same(torbi_amd.state_posteriors(c.obs, route='band', **c.model),
         torbi_amd.forward_backward_banded(c.x, c.frames, c.A, c.pi, left, right, background))
    same(torbi_amd.state_posteriors(c.obs, route='dense', **c.model), torbi_amd.forward_backward(c.x, c.frames, c.A, c.pi))


def test_counts(case):
    _, c = case
    left, right, background = torbi_amd.viterbi.band_over(c.A, c.A, S)
    if background == NINF:
        _, L, Xb, I = torbi_amd.forward_backward_counts_banded(c.x, c.frames, c.A, c.pi, left, right, background)
        same(torbi_amd.expected_counts(c.obs, route='band', **c.model), (torbi_amd.band_counts_to_dense(Xb, left, right), I, L))
    else:                                       # the dense result is not zero outside the band: no band counts route
        with pytest.raises(RuntimeError, match="route='band'"):
            torbi_amd.expected_counts(c.obs, route='band', **c.model)
    _, L, X, I = torbi_amd.forward_backward_counts(c.x, c.frames, c.A, c.pi)
    same(torbi_amd.expected_counts(c.obs, route='dense', **c.model), (X, I, L))


def test_sampling(case):
    _, c = case
    left, right, background = torbi_amd.viterbi.band_over(c.A, c.A, S)
    same(torbi_amd.sample_paths(c.obs, DRAWS, uniforms=c.u, route='band', **c.model),
         torbi_amd.forward_sample_banded(c.x, c.frames, c.A, c.pi, c.u, left, right, background))
    same(torbi_amd.sample_paths(c.obs, DRAWS, uniforms=c.u, route='dense', **c.model),
         torbi_amd.forward_sample(c.x, c.frames, c.A, c.pi, c.u))


def test_k_best(case):
    _, c = case
    left, right, background = torbi_amd.viterbi.band_over(c.A, c.A, S)
    banded = torbi_amd.decode_k_best_banded(c.x, c.frames, c.A, c.pi, K, left, right, background)
    dense = torbi_amd.decode_k_best(c.x, c.frames, c.A, c.pi, K, route='dense')
    same(torbi_amd.best_paths(c.obs, K, route='band', **c.model), banded)
    same(torbi_amd.decode_k_best(c.x, c.frames, c.A, c.pi, K, route='band'), banded)
    same(torbi_amd.best_paths(c.obs, K, route='dense', **c.model), dense)
    same(banded, dense)                         # (the k-best routes give the same bits)


def test_stream(case):
    """The streaming decoder has no stated-band entry: its band route against its dense route and the whole-sequence
    decode, which all give the same bits."""
    _, c = case
    whole = torbi_amd.from_probabilities(c.obs, c.frames, c.A, c.pi, log_probs=True, gpu=0)
    for route in ('band', 'dense'):
        dec = torbi_amd.StreamDecoder(B, S, c.A, c.pi, log_probs=True, gpu=0, route=route)
        assert dec.route == route
        first = dec.push(c.obs[:, :2])
        second = dec.push(c.obs[:, 2:], torch.tensor([T - 2, 1]))
        rest = dec.flush()
        for b, n in enumerate(c.frames.tolist()):
            got = torch.cat([first[b], second[b], rest[b]])
            assert torch.equal(got, whole[b, :n].to(torch.int32))
