"""The test of tests/test_sample_edges_gpu.py's test: on the float64 host route alone (sampling._host, _host_banded) the
crafted rows of tests/sample_edge_cases.py do what they are built for -- steering holds, every heavy share and no-underflow
condition holds, every exact expectation is met with d = 0 --, and each mutant picker, which stands for a kernel bug, breaks
the checker on the probe made for it (SAMPLING.md, both accuracy sections)."""
import math

import pytest
import torch

from torbi_amd import sampling

import sample_edge_cases as ec


def check_on_host(case, whole_route=True):
    """The float64 rule's own draws pass the checker with d = 0 and meet every structural expectation."""
    assert ec.conditions(case) == []
    if whole_route:
        indices, L = ec.host(case)
        assert bool(torch.isfinite(L).all())
        for r in case.rows:                      # the route conditions on its own j_1: the same slots as the row's own draw
            assert torch.equal(indices[r.b, :, r.t], r.host), r.name
    else:                                        # (the largest rows: the draw rule on the float64 weights, row by row)
        indices = ec.with_picker(case, ec.pick_rule)
        for r in case.rows:
            assert torch.equal(indices[r.b, :, r.t], r.host), r.name
    verdict = ec.judge(case, indices)
    assert verdict.failures == []
    assert verdict.worst == 0. and verdict.flips == 0
    for r in case.rows:
        alive = torch.nonzero(r.w > 0)[:, 0]
        first, top, mid = (r.host_slot[r.kinds == k] for k in (ec.K_FIRST, ec.K_TOP, ec.K_MID))
        assert bool((first == alive[0]).all()), r.name
        if float(r.w[alive[-1]]) / r.Z >= ec.HEAVY_SHARE:
            assert bool((top == alive[-1]).all()), r.name
        assert mid.tolist() == r.heavy, r.name
        if r.seam is not None:                   # just above the seam: the first state with a_0 > 0; below it: a band slot
            at = r.kinds == ec.K_SEAM
            target = sampling.read_uniforms(r.u[at]) * r.Z
            above = target >= r.seam
            slot = r.host_slot[at]
            row_first = r.slots + int(torch.nonzero(r.w[r.slots:] > 0)[0, 0])
            within = above & (target < r.seam + float(r.w[row_first]))      # (a light first slot can lie below the next float32)
            assert bool((slot[within] == row_first).all()) and bool((slot[above] >= r.slots).all()), r.name
            assert bool((slot[~above] < r.slots).all()), r.name
    return verdict


@pytest.mark.parametrize('S', list(ec.DENSE_SHAPES))
def test_dense_rows_on_the_host_route(S):
    case = ec.dense_case(S)
    check_on_host(case, whole_route=S <= 4200)
    names = {r.name.split('/')[0].split('@')[0] for r in case.rows}
    assert {'boundaries', 'leading', 'trailing', 'dust', 'ties', 'random'} <= names
    assert any(bool((r.kinds == ec.K_TIE).any()) for r in case.rows)
    kinds = {r.name.split('/')[1] for r in case.rows}
    assert kinds == {'last', 'inner'}
    inner = [r for r in case.rows if r.jstar is not None]
    assert len({r.jstar for r in inner}) == len(inner)                      # each its own row of A
    for r in inner:                                                          # zeros of both makes in every pattern
        if r.heavy:
            dead = r.w == 0
            assert bool((dead & torch.isinf(case.obs[r.b, 0])).any()) and bool((dead & torch.isinf(case.A[r.jstar])).any())
            assert not bool((torch.isinf(case.obs[r.b, 0]) & torch.isinf(case.A[r.jstar])).any())


@pytest.mark.parametrize('S', list(ec.DENSE_SHAPES))
def test_dense_shapes_reach_the_instances_they_name(S):
    """`launch` of torbi_hip_sample: float4 loads at S % 4 == 0, a block of 256 or 64 states, held up to 4096 or 2048 states
    with NB the smallest power of two >= blocks, else streamed with block q in lane q & 63 of register q >> 6."""
    per, K = ec.geometry(S)
    blocks = -(-S // K)
    label = ec.DENSE_SHAPES[S]
    assert label.startswith('float4' if per == 4 else 'scalar')
    if S <= (4096 if per == 4 else 2048):
        NB = 1
        while NB < blocks:
            NB *= 2
        assert label.split(' (')[0] == f"{'float4' if per == 4 else 'scalar'} NB={NB}"
    else:
        assert 'streamed' in label and f'{blocks} blocks' in label
        assert (f'g={(blocks - 1) >> 6}' in label) == (blocks > 64)


def test_the_shapes_cover_every_instance():
    labels = {label.split(' (')[0] for label in ec.DENSE_SHAPES.values()}
    for NB in (1, 2, 4, 8, 16):
        assert f'float4 NB={NB}' in labels and f'scalar NB={NB}' in labels
    assert 'scalar NB=32' in labels and 'float4 streamed' in labels and 'scalar streamed' in labels
    assert {4161, 12353} <= set(ec.DENSE_SHAPES) and {4161, 8257, 16383} <= set(ec.UNIFORM_SHAPES)
    for S, label in ec.UNIFORM_SHAPES.items():
        assert label.startswith('float4' if S % 4 == 0 else 'scalar') and (('held' in label) == (S <= 2048))
    assert {S % 4 == 0 for S, _, _ in ec.BAND_SHAPES} == {True, False}


@pytest.mark.parametrize('S', list(ec.UNIFORM_SHAPES))
def test_uniform_rows_on_the_host_route(S):
    case = ec.uniform_case(S)
    check_on_host(case)
    assert int(torch.isinf(case.pi).sum()) == 1
    assert any(bool((r.kinds == ec.K_TIE).any()) for r in case.rows)
    assert all(float(r.w[torch.isinf(case.pi)]) == 0 for r in case.rows if r.t == 0)


@pytest.mark.parametrize('shape', ec.BAND_SHAPES, ids=ec.band_id)
def test_band_rows_on_the_host_route(shape):
    case = ec.band_case(*shape)
    check_on_host(case)
    S, band, bg = shape
    inner = [r for r in case.rows if r.jstar is not None]
    assert len({r.jstar for r in inner}) == len(inner)
    assert {0, S - 1, S // 2} <= {r.jstar for r in inner}
    if bg not in (-math.inf, ec.TINY):
        assert any(r.seam is not None for r in inner)
        if band[0] + band[1] + 1 < S:                                        # once the band part is empty
            assert any(float(r.w[:r.slots].sum()) == 0 for r in inner)
        assert not bool(torch.isinf(case.A).any())                          # zeros by obs = -inf alone
    for r in inner:                                                          # top under -inf or log(tiny): a band slot > 0
        if r.band_top is not None:
            top = r.host_slot[r.kinds == ec.K_TOP]
            assert bool((top < r.slots).all()) and bool((r.w[top] > 0).all()), r.name


LONG = [('dense', 37, None, None), ('dense', 64, None, None), ('band', 64, (2, 5), -math.inf), ('band', 64, (2, 5), -5.),
        ('uniform', 37, None, None)]


@pytest.mark.parametrize('route,S,band,bg', LONG, ids=['dense_37', 'dense_64', 'band_64_bg_inf', 'band_64_bg_5', 'uniform_37'])
def test_long_sequences_on_the_host_route(route, S, band, bg):
    case = ec.long_case(route, S, band, bg)
    indices, L = ec.host(case)
    verdict = ec.judge(case, indices)
    assert verdict.failures == [] and verdict.worst == 0. and bool(torch.isfinite(L).all())
    assert case.frames.tolist() == [200, 129, 128, 65, 64, 63, 1]


def test_long_streamed_sequence_on_the_host_route():
    case = ec.long_case('dense', 4100, B=1, T=70, frames=(70,))
    indices, L = ec.host(case)
    verdict = ec.judge(case, indices)
    assert verdict.failures == [] and verdict.worst == 0. and bool(torch.isfinite(L).all())


def test_the_rule_as_a_picker_passes():
    case = ec.dense_case(772)
    assert ec.judge(case, ec.with_picker(case, ec.pick_rule)).failures == []


@pytest.mark.parametrize('name', list(ec.MUTANTS))
def test_the_checker_catches_each_mutant(name):
    """Each mutant stands for a kernel bug; the checker names the pattern and the probe kind made for it."""
    picker, pattern, kind = ec.MUTANTS[name]
    case = ec.dense_case(772)                    # float4 loads, four blocks: every pattern exists
    failures = ec.judge(case, ec.with_picker(case, picker)).failures
    assert any(f.startswith(pattern + '/') and f' {kind} probe' in f for f in failures), failures[:5]
