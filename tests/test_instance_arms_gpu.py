"""Arms of the instance ladders of csrc/torbi_hip.hip (csrc/dispatch.hpp) that no other GPU test reaches."""
import math
from collections import OrderedDict

import numpy as np
import pytest
import torch

import oracle
import torbi_amd
from torbi_amd import synth, viterbi
from conftest import CachedOracle
from instance_arm_cases import CASES, batch, label

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


# ---- every arm of the Viterbi ladders: tests/instance_arm_cases.py -------------------------------------------------------

SWITCHES = ('TORBI_HIP_SMALL_VALUE', 'TORBI_HIP_BLOCK_PAIRS', 'TORBI_HIP_BAND_FORM', 'TORBI_HIP_TILE_WAVES')
SEED_FLAGS = {None: 0, 'few': 512, 'many': 1024}
_oracle = CachedOracle(oracle)
_problems = OrderedDict()           # the few most recent (inputs, oracle answers): neighbouring cases share them


def arm_problem(distinct, T, S, band, ties):
    """Inputs of `distinct` different items and the oracle's indices and final value rows for them, computed once per
    (items, frames, states, band, ties) and never written to again.  synth.problem scores; a band keeps the matrix inside
    [next - left, next + right] and holds ONE value outside; the ties variant rounds everything to multiples of 0.5, so many
    candidates are exactly equal and the first-argmax rule decides.  The ragged lengths hold T, 1 and 2 in turn: the final
    rows are rows T - 1, 0 and 1 of the history (or either ping-pong buffer)."""
    key = (distinct, T, S, band, ties)
    if key in _problems:
        _problems.move_to_end(key)
        return _problems[key]
    obs, trans, init = synth.problem(distinct, T, S, seed=S)
    if band is not None:
        left, right, outside = band
        d = np.arange(S)[None, :] - np.arange(S)[:, None]              # prev - next
        trans = np.where((d >= -left) & (d <= right), trans, np.float32(outside)).astype(np.float32)
    if ties:
        obs, trans, init = (np.round(x * 2) / 2 for x in (obs, trans, init))
    frames = np.resize(np.array([T, 1, 2], np.int32), distinct)
    want, rows = _oracle.decode(obs, frames, trans, init, num_threads=oracle.max_threads(), return_posterior=True)
    for array in (obs, trans, init, frames, want, rows):
        array.setflags(write=False)
    _problems[key] = (obs, frames, trans, init, want, rows)
    while len(_problems) > 6:
        _problems.popitem(last=False)
    return _problems[key]


def decode_arm(case, ties, setenv, delenv):
    """The call of `case` on cuda:0: what it reported and returned, beside what the oracle says.  `setenv` / `delenv`:
    monkeypatch's (the library reads its switches per launch)."""
    dev = torch.device('cuda:0')
    B, T, S = batch(case, viterbi.compute_units(dev)), case.T, case.S
    distinct = 40 if B >= 40 else 24         # (neither a multiple of a tile's 16 or 8 items: neighbouring tiles differ)
    obs, frames, trans, init, want, rows = arm_problem(distinct, T, S, case.band, ties)
    item = np.arange(B) % distinct
    for name in SWITCHES:
        if name in case.env:
            setenv(name, case.env[name])
        else:
            delenv(name, raising=False)
    pick = torch.tensor(item, device=dev)
    d_obs, d_frames = torch.tensor(obs, device=dev)[pick], torch.tensor(frames, device=dev)[pick]
    d_trans, d_init = torch.tensor(trans, device=dev), torch.tensor(init, device=dev)
    if case.seeds is not None:               # a scan depth on record: shallow -> one seed per item, deep -> three
        viterbi._depth_record(d_trans, S)[0] = 0.0 if case.seeds == 'few' else float(S)
    assert viterbi._seed_flag(d_trans, S) == SEED_FLAGS[case.seeds]
    ws = torch.empty(viterbi.workspace_bytes(B, T, S), dtype=torch.uint8, device=dev)
    prof = []
    got = torbi_amd.decode(d_obs, d_frames, d_trans, d_init, workspace=ws, path=case.path, _profile=prof)
    gave_up = None
    if case.route in ('cluster', 'band', 'held'):        # workgroups that wait for each other inside the launch
        gave_up = int(viterbi.scan_stats(ws, B, T, S).cpu()[127])
    return {'shape': (B, T, S), 'kernel': viterbi.last_forward_kernel(), 'route': viterbi.ROUTES[int(prof[3])],
            'launches': int(prof[2]), 'gave_up': gave_up, 'indices': got.cpu().numpy(), 'want': want[item],
            'rows': viterbi.read_posterior(ws, d_frames, B, T, S).cpu().numpy(), 'want_rows': rows[item]}


@pytest.mark.parametrize('ties', [False, True], ids=['plain', 'ties'])
@pytest.mark.parametrize('case', CASES, ids=[label(c) for c in CASES])
def test_every_arm_of_the_viterbi_ladders_runs_its_instance_and_equals_the_oracle(case, ties, monkeypatch):
    """One call per arm of the instance ladders of csrc/torbi_hip.hip (tests/instance_arm_cases.py has the table and the
    arithmetic of every expected name): the smallest shape that reaches the arm, both sides of every threshold of
    launch_whole_tiles and of run_resident's cluster ladders.  Each call must

    1. report exactly the instance the rule's text names (torbi_hip_last_forward_kernel) -- a device on which the rule picks
       another instance fails here, it does not skip --,
    2. report the family's route and its number of forward launches, and no workgroup that gave up waiting for the others
       of its launch (clusters, split band tiles, the held kernel: the repair launch behind them would hide an instance that
       leaves part of a row to nobody -- its members wait a quarter of a second for the missing slice and give the tile up),
    3. return the oracle's indices, and
    4. leave the oracle's final value row of EVERY item, bit for bit (torbi_hip_read_posterior): all S values of frame
       F - 1 need every row group, every cluster member's slice and every exchange of the frames before it to be right, which
       the three indices of an item do not (an argmax shows a stale row only when the winning path runs through it).

    40 different items (24 below 40) repeated over the batch, lengths T, 1, 2 in turn; a plain variant and one with every score
    a multiple of 0.5 (exactly equal candidates: the first maximum has to win in every backtrace).

    Where the final rows lie: gather_final_kernel reads routes 0, 6 and 7 from the ping-pong buffers, every other route from
    row F - 1 of the history at the start of the workspace.  Both wavefront forms (small::decode_kernel, decode_value_kernel),
    the workgroup form (block_value_kernel) and the held kernel write their last row to `post0` / `post1` by the parity of
    F - 1, so no form needs planted winners: every case checks rows.

    The held family is pinned by state count alone: its note is 'held::held_forward_kernel' without template arguments, and
    tests/test_workspace_bounds_gpu.py (and the committed benchmark records) are keyed by that spelling, so the note stays;
    the table's `kernel` column names the instance held_instance(S) picks for the completeness test."""
    try:
        found = decode_arm(case, ties, monkeypatch.setenv, monkeypatch.delenv)
    finally:
        torbi_amd.reset_path_state()
    what = f'{label(case)} as {found["shape"]}'
    assert found['kernel'] == case.reported, what
    assert found['route'] == case.route, what
    assert case.launches is None or found['launches'] == case.launches, what
    assert not found['gave_up'], f'{what}: {found["gave_up"]} workgroups gave up waiting, the repair launch decoded their tiles'
    np.testing.assert_array_equal(found['indices'], found['want'], err_msg=what)
    got, want = found['rows'].view(np.uint32), found['want_rows'].view(np.uint32)
    wrong = np.flatnonzero((got != want).any(axis=1))
    assert wrong.size == 0, (f'{what}: final value rows of {wrong.size} items differ, the first: item {wrong[0]}, states '
                             f'{np.flatnonzero(got[wrong[0]] != want[wrong[0]])[:8].tolist()} ...')
