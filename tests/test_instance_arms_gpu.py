"""Arms of the instance ladders of csrc/torbi_hip.hip (csrc/dispatch.hpp) that no other GPU test reaches."""
import math

import numpy as np
import pytest
import torch

import oracle
import torbi_amd
from torbi_amd import synth

pytestmark = pytest.mark.gpu

DISTINCT = 8        # different items of a batch; the batch repeats them


@pytest.mark.parametrize('S', [256, 260, 512, 516, 1024, 1028, 1536, 1540, 2048, 2052, 3072, 3076, 4096])
def test_uniform_entry_with_more_items_than_compute_units_at_every_instance_edge(S):
    """torbi_hip_viterbi_decode_uniform with more items than compute units runs uniform_rows_kernel<NQW, R, PROBS> in 4-wave
    workgroups (`test_uniform_entry_at_every_state_count_it_takes` has three items: the 16- and 8-wave instances only), NQW
    float4 of a row per lane: on and above every step of the ladder, scores and probabilities, against the oracle on the
    materialised matrix.  An instance too narrow for S ignores the states above 256 * NQW, so two items have their best state of
    either frame among the last four, which is asserted on the oracle's paths first."""
    dev = torch.device('cuda:0')
    B, T = torbi_amd.viterbi.compute_units(dev) + 1, 2
    obs, _, init = synth.problem(DISTINCT, T, S, seed=S)
    obs[0, 0, S - 1] += 64
    obs[0, 1, S - 3] += 64
    obs[DISTINCT - 1, 0, S - 4] += 64
    obs[DISTINCT - 1, 1, S - 2] += 64
    few_frames = np.array([2, 1, 2, 2, 1, 2, 2, 2], np.int32)
    c = np.float32(math.log(1. / S))
    full = np.full((S, S), c, np.float32)
    item = np.arange(B) % DISTINCT
    d_obs, d_frames = torch.tensor(obs[item], device=dev), torch.tensor(few_frames[item], device=dev)
    d_init = torch.tensor(init, device=dev)

    def check(want, got, what):
        assert want[0].tolist() == [S - 1, S - 3] and want[DISTINCT - 1].tolist() == [S - 4, S - 2], what
        np.testing.assert_array_equal(got.cpu().numpy(), want[item], err_msg=f'S = {S}, {what}')

    want = oracle.decode(obs, few_frames, full, init, num_threads=oracle.max_threads())
    check(want, torbi_amd.decode_uniform(d_obs, d_frames, float(c), d_init), 'scores')
    probs = torch.softmax(d_obs, dim=-1)
    scores = torch.log(probs[:DISTINCT])
    scores.exp_()
    scores += torch.finfo(torch.float32).tiny
    scores.log_()
    want = oracle.decode(scores.cpu().numpy(), few_frames, full, init, num_threads=oracle.max_threads())
    check(want, torbi_amd.decode_uniform(probs, d_frames, float(c), d_init, probabilities=True), 'probabilities')
