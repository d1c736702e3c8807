"""Every feature that declares more than one band route (torbi_amd/band_route.py, `route`), on the device: the public entry
under `route=` gives, bit for bit, what the stated-band operator of the route its declaration sends the band to gives on the
prepared operands.  The bands: a narrow one; one only the wide routes take; and 65 entries in a row of 64 states, which the
posteriors, the counts and the sampler send to their narrow route (at most min(W, S) = 64 entries are in a row) and path
entropy sends to its wide one (W > 64)."""
import math

import pytest
import torch

import torbi_amd
from torbi_amd import entropy, inputs, viterbi

pytestmark = pytest.mark.gpu

DEV = torch.device('cuda', 0)
NINF = -math.inf
B, T, DRAWS = 2, 3, 3
# (kind, S, reach_left, reach_right, the look finds it); 64 states are the fewest `viterbi.band_over` answers for.  The look
# reads the background from the corner [next 0][prev S - 1], which reach 1/63 of 64 states holds inside the band: there the
# matrix keeps its promise for (1, 63, -inf), and the test answers the look with it.  Reach 63/1 is the same split as found.
CASES = [('narrow', 64, 1, 2, True), ('narrow', 128, 1, 2, True), ('wide', 128, 40, 30, True), ('split', 64, 1, 63, False),
         ('split', 64, 63, 1, True)]
# feature -> kind of band -> the stated-band operator `route='band'` runs
BANDED = {
    'posteriors': dict(narrow=torbi_amd.forward_backward_banded, wide=torbi_amd.forward_backward_wide_banded,
                       split=torbi_amd.forward_backward_banded),
    'log posteriors': dict.fromkeys(('narrow', 'wide', 'split'), torbi_amd.forward_backward_log_banded),
    'counts': dict(narrow=torbi_amd.forward_backward_counts_banded, wide=torbi_amd.forward_backward_counts_wide_banded,
                   split=torbi_amd.forward_backward_counts_banded),
    'entropy': dict(narrow=entropy.forward_entropy_banded, wide=entropy.forward_entropy_wide_banded,
                    split=entropy.forward_entropy_wide_banded),
    'sampling': dict(narrow=torbi_amd.forward_sample_banded, wide=torbi_amd.forward_sample_wide_banded,
                     split=torbi_amd.forward_sample_banded),
}
# 'auto' on the narrow band: the posteriors and the counts take every band their narrow route covers; 4 diagonals of 64 or
# 128 states are a larger share of the row than the 23 / 1440 entropy and sampling were measured on, so those stay dense
AUTO_STAYS_DENSE = {'entropy': entropy.forward_entropy, 'sampling': torbi_amd.forward_sample}


def problem(S, left, right):
    g = torch.Generator().manual_seed(S + left)
    obs = torch.log_softmax(torch.randn(B, T, S, generator=g), 2)
    nxt, prv = torch.arange(S)[:, None], torch.arange(S)[None, :]
    inside = (prv >= nxt - left) & (prv <= nxt + right)
    trans = torch.where(inside, -3. * torch.rand(S, S, generator=g), torch.tensor(NINF))
    init = torch.log_softmax(torch.randn(S, generator=g), 0)
    return obs, torch.tensor([T, T - 1], dtype=torch.int32), trans, init, torch.rand(B, DRAWS, T, generator=g)


def public(feature, obs, frames, trans, init, u, route):
    model = dict(log_probs=True, gpu=0, route=route)
    if feature == 'posteriors':
        return torbi_amd.state_posteriors(obs, frames, trans, init, **model)
    if feature == 'log posteriors':
        return torbi_amd.state_posteriors(obs, frames, trans, init, arithmetic='log', **model)
    if feature == 'counts':
        return torbi_amd.expected_counts(obs, frames, trans, init, **model)
    if feature == 'entropy':
        return entropy.path_entropy(obs, frames, trans, init, prefix=True, **model)
    return torbi_amd.sample_paths(obs, DRAWS, frames, trans, init, uniforms=u, **model)


def stated(feature, operator, operands, u, band):
    """The outputs of `operator` on the prepared operands, in the order of the public entry's."""
    if feature == 'counts':
        _, L, Xb, I = operator(*operands, *band)
        return torbi_amd.band_counts_to_dense(Xb, *band[:2]), I, L
    if feature == 'entropy':
        return operator(*operands, *band, prefix=True)
    if feature == 'sampling':
        return operator(*operands, u, *band)
    return operator(*operands, *band)


@pytest.mark.parametrize('kind,S,left,right,found', CASES)
@pytest.mark.parametrize('feature', list(BANDED))
def test_the_public_entry_runs_the_operator_its_declaration_names(monkeypatch, feature, kind, S, left, right, found):
    obs, frames, trans, init, u = problem(S, left, right)
    prepared, uniform, init_d = inputs.model(trans, init, True, S, DEV, plain=True)
    operands = (inputs.observation(obs, True, DEV), frames.to(DEV), prepared, init_d)
    band = (left, right, NINF)
    assert uniform is None and (viterbi.band_over(prepared, prepared, S) == band) == found
    if not found:
        monkeypatch.setattr(viterbi, 'band_over', lambda trans, original, states: band)
    want = stated(feature, BANDED[feature][kind], operands, u.to(DEV), band)
    got = public(feature, obs, frames, trans, init, u, 'band')
    assert len(got) == len(want) and all(torch.equal(g, w) for g, w in zip(got, want))
    assert not torch.isnan(got[2 if feature == 'counts' else 1]).any()          # (the log-likelihoods: a run, not a refusal)
    if kind == 'narrow':
        if feature in AUTO_STAYS_DENSE:
            want = stated(feature, AUTO_STAYS_DENSE[feature], operands, u.to(DEV), ())
        got = public(feature, obs, frames, trans, init, u, 'auto')
        assert len(got) == len(want) and all(torch.equal(g, w) for g, w in zip(got, want))
