"""Path statistics on an MI355X (csrc/path_statistics.hpp behind torbi_hip_path_statistics): the device route against the
per-path Python loop of tests/path_cases.py -- score bits with equal NaN positions, unweighted and dyadic-weight counts by
==.

The kernel gives a path one wavefront and a workgroup four (ps::kWaves), and walks a path in chunks of 64 frames: T in
{1, 2, 63, 64, 65, 129} lies on and around one and two chunk edges, T = 200 with F = 150 ends mid-chunk; 3 x 3 and 3 x 5
paths leave the last workgroup part empty; one case runs 8 x 4 x 500 x 1440 on the pitch band matrix.  Contention (every
path in one state), voids and specials, the three entry forms, the round trips through `best_paths`, `from_probabilities`
and `sample_paths`, the caller-owned workspace, graph capture, another stream, operand forms and the gradients follow."""
import math

import numpy as np
import pytest
import torch

import torbi_amd
from torbi_amd import paths

import path_cases as pc
import stream_band_cases as sbc
from workspace_cases import DEV, assert_guards_intact, assert_same_bits, guarded

pytestmark = pytest.mark.gpu


def device(obs, frames, A, pi, indices, weights=None, **more):
    return paths.path_statistics(*pc.tensors(obs, frames, A, pi, indices, weights, device=DEV), **more)


def host_copy(out):
    return tuple(x.cpu() for x in out if x is not None)


def check(case, what, weights_seed=None):
    obs, frames, A, pi, indices, (scores, X, I, kept) = case
    B, K, T = indices.shape
    got = device(obs, frames, A, pi, indices)
    assert got[0].device == DEV and got[0].shape == (B, K)
    pc.same_scores(got[0], scores, what)
    pc.same_counts(got[1:], (X, I), what)
    if weights_seed is not None:
        w = pc.dyadic_weights(B, K, weights_seed)
        pc.same_counts(device(obs, frames, A, pi, indices, w)[1:], pc.weighted(indices, frames, obs.shape[2], w), what)


# ------------------------------------------------------------------------------------------------ against the loop
@pytest.mark.parametrize('T', [1, 2, 63, 64, 65, 129])
def test_chunk_edges(T):
    check(pc.case(5, 2, T, 7, 300 + T), T, weights_seed=T)


def test_frames_that_end_mid_chunk():
    obs, A, pi = pc.model(3, 200, 7, 41)
    frames = np.array([150, 200, 65], np.int32)
    indices = pc.random_paths(3, 2, 200, 7, 42)
    check((obs, frames, A, pi, indices, pc.loop(obs, frames, A, pi, indices)), 'mid-chunk', weights_seed=1)


@pytest.mark.parametrize('K', [3, 5])
@pytest.mark.parametrize('S', [1, 2, 7, 65])
def test_path_and_state_counts(K, S):
    check(pc.case(3, K, 70, S, 500 + 10 * S + K), (K, S), weights_seed=S)


def test_the_uniform_model():
    check(pc.case(3, 3, 70, 12, 77, False), 'uniform')


def test_the_pitch_band_at_1440_states():
    B, K, T, S = 8, 4, 500, 1440
    g = torch.Generator().manual_seed(5)
    obs = torch.log_softmax(3. * torch.randn(B, T, S, generator=g), 2).numpy()
    A = sbc.band_matrix(S, 87, 87, sbc.TINY, seed=3)
    pi = torch.log_softmax(torch.randn(S, generator=g), 0).numpy()
    rng = np.random.default_rng(6)
    steps = rng.integers(-87, 88, size=(B, K, T)) * (rng.random((B, K, T)) < .2)          # held notes, jumps inside the band
    indices = np.clip(np.cumsum(steps, axis=2) + rng.integers(0, S, size=(B, K, 1)), 0, S - 1).astype(np.int32)
    frames = np.array([500, 1, 499, 64, 65, 500, 333, 128], np.int32)
    want = pc.loop(obs, frames, A, pi, indices)
    assert np.isfinite(want[0]).all()
    check((obs, frames, A, pi, indices, want), 'pitch band', weights_seed=2)


def test_every_add_on_one_cell():
    B, K, T, S = 64, 4, 129, 3
    obs, A, pi = pc.model(B, T, S, 8)
    indices = np.full((B, K, T), 1, np.int32)
    frames = np.full((B,), T, np.int32)
    got = device(obs, frames, A, pi, indices)
    want = pc.loop(obs, frames, A, pi, indices)
    assert want[1][1, 1] == B * K * (T - 1) == want[1].sum() and want[2][1] == B * K
    pc.same_scores(got[0], want[0])
    pc.same_counts(got[1:], want[1:3])
    w = pc.dyadic_weights(B, K, 9)
    pc.same_counts(device(obs, frames, A, pi, indices, w)[1:], pc.weighted(indices, frames, S, w))


def test_general_weights_are_within_one_rounding_of_the_float64_loop():
    B, K, T, S = 16, 4, 129, 2
    q = pc.random_paths(B, K, T, S, 9)
    frames = np.full((B,), T, np.int32)
    w = pc.general_weights(B, K, 10)
    got = paths.count_paths(*pc.tensors(q, device=DEV), S, *pc.tensors(frames, w, device=DEV))
    pc.same_counts(got, pc.weighted(q, frames, S, w), relative=pc.ULP)


# ------------------------------------------------------------------------------------------------ voids and specials
def test_void_paths_score_minus_inf_and_count_nothing():
    obs, _, A, pi, indices, _ = pc.case(2, 3, 130, 7, 83)
    frames = np.array([66, 130], np.int32)
    q = np.array(indices)
    q[0, 0, 65] = -1                        # the last column item 0 reads, in its second chunk: void
    q[0, 1, 66] = 7                         # behind item 0's frames: ignored
    q[1, 2, 0] = 7                          # S itself, in the first column: void
    q[1, 0, 129] = 2 ** 31 - 1
    want = pc.loop(obs, frames, A, pi, q)
    assert sorted(set((b, k) for b in range(2) for k in range(3)) - set(want[3])) == [(0, 0), (1, 0), (1, 2)]
    got = device(obs, frames, A, pi, q)
    pc.same_scores(got[0], want[0])
    pc.same_counts(got[1:], want[1:3])


def test_minus_inf_and_nan_matter_on_the_path_and_nowhere_else():
    obs, frames, A, pi, q = pc.special_case()
    want = pc.loop(obs, frames, A, pi, q)
    assert want[0][0, 0] == pc.NINF and np.isnan(want[0][0, 1]) and np.isnan(want[0][0, 2]) and np.isfinite(want[0][0, 3])
    got = device(obs, frames, A, pi, q)
    pc.same_scores(got[0], want[0])
    pc.same_counts(got[1:], want[1:3])


# ------------------------------------------------------------------------------------------------ entry forms
def test_scores_only_without_a_workspace_and_counts_only_without_a_model():
    obs, frames, A, pi, indices, (scores, X, I, _) = pc.case(3, 3, 70, 7, 573)
    only = device(obs, frames, A, pi, indices, counts=False)
    assert only[1] is None and only[2] is None
    pc.same_scores(only[0], scores)
    q, f = pc.tensors(indices, frames, device=DEV)
    counted = paths.count_paths(q, 7, f)
    assert counted[0].device == DEV
    pc.same_counts(counted, (X, I))
    flat = paths.path_statistics(*pc.tensors(obs, frames, A, pi, device=DEV), q[:, 1])
    assert flat[0].shape == (3,)
    pc.same_scores(flat[0], scores[:, 1])
    empty = paths.path_statistics(torch.empty(0, 3, 4, device=DEV), None, None, torch.zeros(4, device=DEV),
                                  torch.empty(0, 2, 3, dtype=torch.int32, device=DEV))
    assert empty[0].shape == (0, 2) and float(empty[1].sum()) == 0.


# ------------------------------------------------------------------------------------------------ round trips
def _probabilities(B, T, S, seed, matrix=True):
    g = torch.Generator().manual_seed(seed)
    obs = torch.softmax(2. * torch.randn(B, T, S, generator=g), 2)
    A = torch.softmax(2. * torch.randn(S, S, generator=g), 0) if matrix else None
    pi = torch.softmax(torch.randn(S, generator=g), 0)
    return obs, A, pi


@pytest.mark.parametrize('matrix', [True, False], ids=['dense', 'uniform'])
def test_scoring_best_paths_gives_its_scores_at_every_rank(matrix):
    obs, A, pi = _probabilities(5, 70, 12, 21, matrix)
    frames = torch.tensor([70, 1, 65, 2, 64], dtype=torch.int32)
    indices, scores = torbi_amd.best_paths(obs, 4, frames, A, pi, gpu=0)
    assert torch.isfinite(scores).all()
    got = paths.score_paths(obs, indices, frames, A, pi, gpu=0)
    assert got.device == DEV
    pc.same_scores(got, scores.cpu().numpy(), matrix)
    path = torbi_amd.from_probabilities(obs.clone(), frames, A, pi, gpu=0)
    pc.same_scores(paths.score_paths(obs, path, frames, A, pi, gpu=0), scores[:, 0].cpu().numpy(), matrix)
    X, I, again = paths.viterbi_counts(obs, frames, A, pi, gpu=0)
    pc.same_scores(again, scores[:, 0].cpu().numpy(), matrix)
    pc.same_counts((X, I), pc.loop(None, frames.numpy(), 12, None, path.cpu().numpy()[:, None, :])[1:3])


def test_sampled_paths_score_below_the_best_and_count_every_step():
    obs, A, pi = _probabilities(5, 70, 12, 22)
    frames = torch.tensor([70, 1, 65, 2, 64], dtype=torch.int32)
    draws, _ = torbi_amd.sample_paths(obs, 16, frames, A, pi, gpu=0, generator=torch.Generator(device=DEV).manual_seed(1))
    scores = paths.score_paths(obs, draws, frames, A, pi, gpu=0)
    _, best = torbi_amd.best_paths(obs, 1, frames, A, pi, gpu=0)
    assert scores.shape == (5, 16) and bool(torch.isfinite(scores).all()) and bool((scores <= best).all())
    X, I = paths.count_paths(draws, 12, frames.to(DEV))
    assert float(X.double().sum()) == 16 * float((frames - 1).sum()) and float(I.sum()) == 16 * 5
    pc.same_counts((X, I), pc.loop(None, frames.numpy(), 12, None, draws.cpu().numpy())[1:3])


# ------------------------------------------------------------------------------------------------ the workspace
@pytest.mark.parametrize('offset', [0, 1])
def test_a_caller_owned_workspace_of_exactly_the_stated_size(offset):
    obs, frames, A, pi, indices, (scores, X, I, _) = pc.case(3, 3, 70, 65, 500 + 650 + 3)
    ops = pc.tensors(obs, frames, A, pi, indices, device=DEV)
    want = paths.path_statistics(*ops)
    ws = guarded(paths.path_statistics_workspace_bytes(3, 70, 65, 3), offset=offset, fill=0xFF)
    got = paths.path_statistics(*ops, workspace=ws)
    assert_guards_intact(ws)
    assert_same_bits(host_copy(got), host_copy(want), f'workspace at offset {offset}')
    pc.same_counts(got[1:], (X, I))
    again = paths.path_statistics(*ops, workspace=ws)              # over its own stale accumulators
    assert_same_bits(host_copy(again), host_copy(want), 'a second call in the same workspace')
    assert_guards_intact(ws)
    with pytest.raises(RuntimeError, match='workspace'):
        paths.path_statistics(*ops, workspace=ws[1:])


# ------------------------------------------------------------------------------------------------ graphs and streams
def test_graph_capture_and_replay_on_new_indices_and_a_new_observation():
    B, K, T, S = 3, 3, 70, 65
    first, frames, A, pi, q1, _ = pc.case(B, K, T, S, 500 + 650 + 3)
    second, q2 = pc.model(B, T, S, 99)[0], pc.random_paths(B, K, T, S, 98)
    obs, f, A_, pi_, q = pc.tensors(first, frames, A, pi, q1, device=DEV)
    ws = torch.full((paths.path_statistics_workspace_bytes(B, T, S, K),), 0xFF, dtype=torch.uint8, device=DEV)
    paths.path_statistics(obs, f, A_, pi_, q, workspace=ws)          # (loads the kernels outside the capture)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = paths.path_statistics(obs, f, A_, pi_, q, workspace=ws)
    obs.copy_(torch.from_numpy(second))
    q.copy_(torch.from_numpy(q2))
    graph.replay()
    torch.cuda.synchronize()
    once = host_copy(tuple(x.clone() for x in out))
    want = pc.loop(second, frames, A, pi, q2)
    pc.same_scores(once[0], want[0])
    pc.same_counts(once[1:], want[1:3])
    graph.replay()                                                   # the accumulators are zeroed inside the graph
    torch.cuda.synchronize()
    assert_same_bits(host_copy(out), once, 'a second replay on equal inputs')


def test_a_call_on_another_stream():
    obs, frames, A, pi, indices, (scores, X, I, _) = pc.case(3, 3, 70, 65, 500 + 650 + 3)
    ops = pc.tensors(obs, frames, A, pi, indices, device=DEV)
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        out = paths.path_statistics(*ops)
    stream.synchronize()
    pc.same_scores(out[0], scores)
    pc.same_counts(out[1:], (X, I))


# ------------------------------------------------------------------------------------------------ operand forms
def test_strided_offset_float64_and_int64_operands_give_the_bits_of_the_plain_call():
    B, K, T, S = 3, 3, 70, 7
    obs, frames, A, pi, indices, (scores, X, I, _) = pc.case(B, K, T, S, 573)
    o, f, a, p, q = pc.tensors(obs, frames, A, pi, indices, device=DEV)
    w = torch.from_numpy(pc.dyadic_weights(B, K, 3)).to(DEV)
    want = host_copy(paths.path_statistics(o, f, a, p, q, w))
    filler = lambda shape, dtype: torch.full(shape, 3, dtype=dtype, device=DEV)
    wide = filler((B, T, 2 * S + 1), torch.float32)
    wide[:, :, 1::2] = o                                               # strided in the state axis, one element in
    o_view = wide[:, :, 1::2]
    a_view = a.t().contiguous().t()                                    # transposed storage
    p_view = torch.cat([filler((1,), torch.float32), p])[1:]           # one element into its buffer
    q_wide = filler((B, K + 2, T + 3), torch.int32)
    q_wide[:, 1:K + 1, 3:] = q
    q_view = q_wide[:, 1:K + 1, 3:]
    f_view = torch.stack([f, f], 1)[:, 0]
    w_view = torch.stack([w, w], 2)[:, :, 1]
    assert not o_view.is_contiguous() and not a_view.is_contiguous() and not q_view.is_contiguous()
    got = paths.path_statistics(o_view, f_view, a_view, p_view, q_view, w_view)
    assert_same_bits(host_copy(got), want, 'views')
    got = paths.path_statistics(o.double(), f.long(), a.double(), p.double(), q.long(), w.double())
    assert_same_bits(host_copy(got), want, 'float64 and int64')
    assert torch.equal(wide[:, :, 0::2], filler((B, T, S + 1), torch.float32)) and torch.equal(o_view, o)     # nothing written


# ------------------------------------------------------------------------------------------------ gradients
def test_best_path_score_gradients_equal_the_hosts():
    obs, frames, A, pi, _, _ = pc.case(3, 2, 130, 65, 11 * 65 + 130)
    g = torch.tensor([1., .5, -2.])
    grads = []
    for dev in ('cpu', DEV):
        o, f, a, p = pc.tensors(obs, frames, A, pi, device=dev)
        o, a, p = o.requires_grad_(), a.requires_grad_(), p.requires_grad_()
        score = paths.best_path_score(o, f, a, p)
        (score * g.to(dev)).sum().backward()
        grads.append((score.detach().cpu(), o.grad.cpu(), a.grad.cpu(), p.grad.cpu()))
        assert o.grad.device == o.device and a.grad.shape == (65, 65)
    assert_same_bits(grads[1], grads[0], 'device against host')
    assert float(grads[1][1].sum()) == float((g * torch.from_numpy(pc.clamp(frames, 130)).float()).sum())
