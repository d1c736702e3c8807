"""The path samplers of csrc/sample.hpp and csrc/sample_band.hpp on an MI355X at interval edges, zero runs and long sequences:
the crafted rows and probe uniforms of tests/sample_edge_cases.py (which tests/test_sample_edges_cpu.py proves on the float64
host route) at the smallest shapes that reach every instance of sample_backward_kernel, every register of `Streamed`, both
forms of sample_uniform_rows_kernel and of sample_band_backward_kernel, and sequences of up to 200 frames (SAMPLING.md, both
accuracy sections).  The only numeric bound is the project's 1e-4 on d; every other assertion is exact."""
import math

import pytest
import torch

import torbi_amd

import sample_edge_cases as ec

pytestmark = pytest.mark.gpu

DEV = torch.device('cuda:0')


class OnDevice:
    """A case's inputs on the device, moved once."""

    def __init__(self, case):
        self.case = case
        self.obs, self.frames, self.pi = case.obs.to(DEV).contiguous(), case.frames.to(DEV), case.pi.to(DEV)
        self.A = None if case.A is None else case.A.to(DEV)
        self.u = case.u.to(DEV)

    def run(self, draws=None):
        """The route at the operator level on the first `draws` draws: (indices, L) on the host."""
        case, u = self.case, self.u if draws is None else self.u[:, :draws].contiguous()
        if case.route == 'uniform':
            uniform = float(torch.tensor(math.log(1. / case.S), dtype=torch.float32))
            out = torbi_amd.sampling._run(self.obs, self.frames, None, uniform, self.pi, u)
        elif case.route == 'band':
            out = torbi_amd.forward_sample_banded(self.obs, self.frames, self.A, self.pi, u, case.band[0], case.band[1], case.bg)
        else:
            out = torbi_amd.forward_sample(self.obs, self.frames, self.A, self.pi, u)
        assert out[0].dtype == torch.int32 and out[1].dtype == torch.float32 and out[0].device == DEV
        return out[0].cpu(), out[1].cpu()

    def posterior_L(self):
        """L of the posterior call whose bits the sampler promises."""
        case = self.case
        if case.route == 'band':
            return torbi_amd.forward_backward_banded(self.obs, self.frames, self.A, self.pi, case.band[0], case.band[1],
                                                     case.bg)[1].cpu()
        return torbi_amd.forward_backward(self.obs, self.frames, self.A, self.pi)[1].cpu()


def check(label, case, draws_again=None):
    dev = OnDevice(case)
    indices, L = dev.run()
    verdict = ec.judge(case, indices)
    print(f'{label}: worst d = {verdict.worst:.3g} ({100 * verdict.worst / ec.BOUND:.2f} % of the bound), '
          f'{verdict.flips} of {verdict.edges} edge probes took another neighbour than float64')
    assert verdict.failures == [], verdict.failures[:10]
    assert verdict.worst <= ec.BOUND
    assert bool(torch.isfinite(L).all())
    if case.route != 'uniform':
        assert torch.equal(L, dev.posterior_L())
    if draws_again is not None:
        fewer, Ln = dev.run(draws_again)
        assert torch.equal(fewer, indices[:, :draws_again]) and torch.equal(Ln, L)
    return verdict


@pytest.mark.parametrize('S', list(ec.DENSE_SHAPES), ids=lambda S: f"{S}_{ec.DENSE_SHAPES[S].split(' (')[0].replace(' ', '_')}")
def test_dense_route_at_edges_and_zero_runs(S):
    check(f'dense {S} ({ec.DENSE_SHAPES[S]})', ec.dense_case(S))


@pytest.mark.parametrize('S', list(ec.UNIFORM_SHAPES), ids=lambda S: f"{S}_{ec.UNIFORM_SHAPES[S].replace(' ', '_')}")
def test_uniform_route_at_edges_and_zero_runs(S):
    check(f'uniform {S} ({ec.UNIFORM_SHAPES[S]})', ec.uniform_case(S))


@pytest.mark.parametrize('shape', ec.BAND_SHAPES, ids=ec.band_id)
def test_band_route_at_edges_seams_and_zero_runs(shape):
    check(f'band {ec.band_id(shape)}', ec.band_case(*shape))


LONG = [('dense', 37, None, None), ('dense', 64, None, None), ('band', 64, (2, 5), -math.inf), ('band', 64, (2, 5), -5.),
        ('uniform', 37, None, None)]


@pytest.mark.parametrize('route,S,band,bg', LONG, ids=['dense_37', 'dense_64', 'band_64_bg_inf', 'band_64_bg_5', 'uniform_37'])
def test_long_sequences_and_runs_of_64_frames(route, S, band, bg):
    """T = 200 with F = 200, 129, 128, 65, 64, 63 and 1: whole runs, a first run that is partial, tails longer than a wave."""
    check(f'long {route} {S} {bg}', ec.long_case(route, S, band, bg), draws_again=1)


def test_long_streamed_sequence():
    check('long dense 4100 streamed', ec.long_case('dense', 4100, B=1, T=70, frames=(70,)), draws_again=1)
