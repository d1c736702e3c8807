"""Every entry that takes an observation, on an MI355X, with one operand at a time (and once all of them) in a form callers
hold -- a transposed or strided view, a slice of a longer tensor, a view one element into its buffer, float64 / float16 /
bfloat16 / int64, on the host, frames out of range -- against the same entry on plain copies, BIT FOR BIT, and the caller's
tensors and the bases they were cut from keep their bits.  tests/operand_form_cases.py has the forms, the table of entries
and what a row does not take; tests/test_operand_forms_cpu.py runs the table through the `gpu=None` routes and pins what
the fronts hand the band planner.  No tolerance is introduced here: every form is compared by `ofc.same`, and each entry
keeps ONE anchor, the plain call against the float64 host route (the oracle for the decoders) under the bound that entry's
own GPU test uses, so that form and plain copy cannot both be wrong alike.

The matrix.  Every front with a band planner looks at `inputs.device_matrix`'s tensor -- float32, contiguous, 16-byte
aligned -- and hands its kernels that object; `viterbi.band_over` refuses anything else.  Before that, `state_posteriors`,
`posterior_route`, `expected_counts` and `counts_route` handed the look the caller's strides and dtype: the transposed view
of a band of reach 3/2 was read as reach 2/3 and `state_posteriors(route='auto')` returned NaN everywhere.  The tests below
assert the routes, the band each `route='band'` takes, the note the look leaves and what a second feature makes of it.

An observation whose base is 4-byte aligned (`offset4`; also what `.contiguous()` leaves of a float32 view that is
contiguous already).  Observations are not copied for alignment by the entries below; what each C entry's kernels do with
the pointer, read off csrc/torbi_hip.hip and the kernels' headers:
* state_posteriors, expected_counts, best_paths, sample_paths, StreamDecoder.push, StreamPosteriors.push: never see such a
  pointer -- `inputs.observation` clones a float32 device observation (the caller's tensor is not written) and converts any
  other, so the kernels get a fresh allocation;
* torbi_hip_forward_backward, _counts (forward_backward, forward_backward_counts, log_likelihood, state_posteriors'
  dense route): fb_rowmax / fb_forward_first / fb_step / fb_backward_last read the observation, the matrix
  (fb_prepare_kernel), the initial row and the weights element by element; the step's 16-byte variant is chosen by the
  pointer of the posterior OUTPUT (torbi_hip.hip fb_dense `vec`) and reads rows of the outputs and the workspace only;
* torbi_hip_forward_backward_uniform, torbi_hip_sample_uniform: chosen by the pointer (`vec` over observation | posterior_out,
  observation | initial);
* torbi_hip_forward_backward_band, _counts_band, torbi_hip_sample_band, torbi_hip_k_best_band, torbi_hip_k_best,
  torbi_hip_stream_band_push, torbi_hip_stream_smooth_band_push: their kernels hold no 16-byte access to an operand
  (forward_backward_band.hpp, counts_band.hpp, sample_band.hpp, k_best_band.hpp, k_best.hpp, stream_band.hpp,
  stream_posterior_band.hpp);
* torbi_hip_sample: the forward half is torbi_hip_forward_backward's; the backward kernel's 16-byte reads are of the filter
  rows in the workspace (256-byte aligned), the uniforms are read element by element;
* torbi_hip_stream_push, torbi_hip_stream_posterior_push: the 16-byte variant is chosen by the pointer of the object's own
  transposed / exponentiated matrix and reads that matrix only; observation rows are read element by element;
* torbi_hip_viterbi_decode* (decode, from_probabilities, decode_uniform's fall-back): the band forms and the uniform entry
  choose by the pointer (decode_group `vec`, torbi_hip_viterbi_decode_uniform returns EUNSUPPORTED and `decode_uniform`
  materialises the matrix), the matrix is chosen by the pointer everywhere (tests/test_gpu_parity.py), but the dense,
  pruned, time-resident, held-matrix and small-state forward kernels read observation rows and the initial row in 16-byte
  pieces and were not all read to the end: NEITHER holds, so `decode`'s front copies an observation or an initial row whose
  base is off a 16-byte boundary (torbi_amd/viterbi.py) before its `offset4` case runs here.
"""
import math

import numpy as np
import pytest
import torch

import oracle
import torbi_amd
from torbi_amd import inputs, posterior, state, viterbi

import k_best_cases as kc
import operand_form_cases as ofc
import sample_cases as sc
import stream_posterior_cases as spc
from operand_form_cases import A, B, BY_NAME, DRAWS, F, K, NINF, O, PI, S, T, TINY, U, W

pytestmark = pytest.mark.gpu

DEV = torch.device('cuda', 0)
CPU = torch.device('cpu')
CASES = ofc.cases(DEV)
MATRIX_FORMS = [name for name in ofc.FORMS[A] if name != 'plain']
TRUE_BAND = {'band': (3, 2, NINF), 'band_tiny': (3, 2, TINY), 'symmetric': (2, 2, NINF)}        # (ofc.MODELS)
# the rows whose call looks at the matrix and leaves a note (`decode_k_best(route='dense')` and the dense stream routes never
# look; `log_likelihood` notes with a leaf the call makes itself)
LOOKING = ('state_posteriors', 'expected_counts', 'best_paths', 'sample_paths', 'StreamDecoder-band', 'StreamPosteriors-band',
           'routes')


def true_band(model, plain):
    """(reach_left, reach_right, background) the matrix was BUILT with; the background as the plain copy holds it in its
    corner (a half-precision form rounds log(tiny), a probability matrix's logarithm is taken on the device)."""
    left, right, background = TRUE_BAND[model]
    held = float(plain[0, S - 1])
    assert held == background or background == TINY
    return left, right, held


def loglik_close(got, want, frames):
    """tests/test_posterior_gpu.py::check's bound on a log-likelihood."""
    err = np.abs(numbers(got) - numbers(want))
    assert np.all(err <= spc.loglik_bound(numbers(want), np.asarray(frames))), err


def check_look(matrix, model='band', log_probs=True):
    """The plain copy's look and the note kept for the caller's tensor -- with the matrix that was prepared from it, never
    under the caller's object unless that IS the matrix -- name the true band."""
    plain = ofc.plain_copy(matrix if log_probs else torch.log(matrix), DEV)
    band = true_band(model, plain)
    assert viterbi.band_over(plain, plain, S) == band
    looked = inputs.device_matrix(matrix, log_probs, DEV)
    assert torch.equal(ofc.bits(looked), ofc.bits(plain))
    assert state.peek(looked)[('band_over', S)] == band
    if looked is not matrix:
        kept = state.peek(matrix)
        assert kept is None or ('band_over', S) not in kept


@pytest.mark.parametrize('name,operand,form_name', CASES, ids=['-'.join(c) for c in CASES])
def test_a_form_equals_its_plain_copy_and_nothing_is_written(name, operand, form_name):
    entry = BY_NAME[name]
    ops, got = ofc.check_forms(entry, DEV, 0, {operand: form_name})
    if operand == A and name in LOOKING:
        check_look(ops[A])


@pytest.mark.parametrize('name', [e.name for e in ofc.ENTRIES if e.gpu])
def test_every_operand_in_another_form_at_once(name):
    entry = BY_NAME[name]
    ops, _ = ofc.check_forms(entry, DEV, 0, {operand: ofc.TOGETHER[operand] for operand in entry.operands})
    if name in LOOKING:
        check_look(ops[A])


# ---------------------------------------------------------------------------------------- routes
def model_of(name, matrix):
    p = ofc.problem(name)
    return dict(batch_frames=p[F].to(DEV), transition=matrix, initial=p[PI].to(DEV), log_probs=True, gpu=0)


@pytest.mark.parametrize('form_name', ['plain'] + MATRIX_FORMS)
@pytest.mark.parametrize('model', list(TRUE_BAND))
def test_routes_and_bands_follow_the_values_not_the_form(model, form_name):
    """The six `*_route` answers for every form of three band matrices are the plain copy's; `route='band'` takes the TRUE
    band -- equal to the stated-band entry on the plain copy --; `route='auto'` equals the plain copy's call."""
    p = ofc.problem(model)
    matrix, base = ofc.form(form_name, p[A], DEV)
    plain = ofc.plain_copy(matrix, DEV)
    snapshot = ofc.Snapshot([matrix, base])
    routes = BY_NAME['routes']
    want = ofc.reference(routes, {A: plain}, 0)
    assert routes.call({A: matrix}, 0) == want
    check_look(matrix, model)
    left, right, background = true_band(model, plain)
    obs, x = p[O].to(DEV), inputs.observation(p[O].to(DEV), True, DEV)        # x: what the operator level is handed
    frames, pi, u = p[F].to(DEV), p[PI].to(DEV), p[U].to(DEV)
    given, copy = model_of(model, matrix), model_of(model, plain)
    ofc.same(torbi_amd.state_posteriors(obs, route='band', **given),
             torbi_amd.forward_backward_banded(x, frames, plain, pi, left, right, background))
    if background == NINF:
        _, L, Xb, I = torbi_amd.forward_backward_counts_banded(x, frames, plain, pi, left, right, background)
        ofc.same(torbi_amd.expected_counts(obs, route='band', **given), (torbi_amd.band_counts_to_dense(Xb, left, right), I, L))
    else:
        with pytest.raises(RuntimeError, match="route='band'"):
            torbi_amd.expected_counts(obs, route='band', **given)
    ofc.same(torbi_amd.best_paths(obs, K, route='band', **given),
             torbi_amd.decode_k_best_banded(x, frames, plain, pi, K, left, right, background))
    ofc.same(torbi_amd.sample_paths(obs, DRAWS, uniforms=u, route='band', **given),
             torbi_amd.forward_sample_banded(x, frames, plain, pi, u, left, right, background))
    for entry in (torbi_amd.state_posteriors, torbi_amd.expected_counts):
        ofc.same(entry(obs, route='auto', **given), entry(obs, route='auto', **copy))
    ofc.same(torbi_amd.best_paths(obs, K, route='auto', **given), torbi_amd.best_paths(obs, K, route='auto', **copy))
    ofc.same(torbi_amd.sample_paths(obs, DRAWS, uniforms=u, route='auto', **given),
             torbi_amd.sample_paths(obs, DRAWS, uniforms=u, route='auto', **copy))
    for stream in (torbi_amd.StreamDecoder, torbi_amd.StreamPosteriors):
        for route in ('band', 'auto'):
            mine = stream(B, S, matrix, pi, log_probs=True, gpu=0, route=route)
            theirs = stream(B, S, plain, pi, log_probs=True, gpu=0, route=route)
            assert mine.route == theirs.route and (route == 'auto' or mine.route == 'band')
            assert mine._band[:2] == (left, right) if mine.route == 'band' else mine._band is None
    check_look(matrix, model)
    snapshot.check((model, form_name))


# ---------------------------------------------------------------------------------------- memory across features
def feature_calls(matrix):
    p = ofc.problem('band')
    obs, u = p[O].to(DEV), p[U].to(DEV)
    model = model_of('band', matrix)

    def decoder():
        dec = torbi_amd.StreamDecoder(B, S, matrix, model['initial'], log_probs=True, gpu=0, route='auto')
        parts = [dec.push(chunk, frames) for chunk, frames in ofc._pushes(obs, torch.tensor(ofc.SECOND))] + [dec.flush()]
        return tuple(torch.cat(per_stream) for per_stream in zip(*parts)) + (dec.route,)

    return [('state_posteriors', lambda: torbi_amd.state_posteriors(obs, route='auto', **model)),
            ('best_paths', lambda: torbi_amd.best_paths(obs, K, route='auto', **model)),
            ('sample_paths', lambda: torbi_amd.sample_paths(obs, DRAWS, uniforms=u, route='auto', **model)),
            ('StreamDecoder', decoder)]


@pytest.mark.parametrize('order', ['forward', 'reverse'])
def test_what_one_feature_learns_about_a_view_serves_the_next(order):
    """`state_posteriors(route='auto')` with the transposed view of the asymmetric band, then `best_paths`, `sample_paths` and
    `StreamDecoder` with the SAME tensor object (and in the reverse order): each equals its call on the plain copy."""
    view, base = ofc.form('transposed', ofc.problem('band')[A], DEV)
    plain = ofc.plain_copy(view, DEV)
    want = dict((name, call()) for name, call in feature_calls(plain))
    calls = feature_calls(view)
    for name, call in (calls if order == 'forward' else calls[::-1]):
        ofc.same(call(), want[name], name)
        check_look(view)
    assert not torch.isnan(want['state_posteriors'][0]).any()


@pytest.mark.parametrize('entry', ['state_posteriors', 'expected_counts'])
def test_one_object_with_two_meanings(entry):
    """A positive matrix with one value outside a band, first with `log_probs=False` and then the SAME object with
    `log_probs=True`: each call equals its own `route='dense'` result within the entry's bound, neither returns NaN, and each
    meaning keeps its own look."""
    import test_counts_gpu
    import test_posterior_gpu
    p = ofc.problem('band_tiny')
    P = torch.exp(p[A]).to(DEV)
    pi = torch.exp(p[PI]).to(DEV)
    obs = torch.exp(p[O]).to(DEV)
    frames = p[F].to(DEV)
    call = getattr(torbi_amd, entry)
    for log_probs in (False, True):
        model = dict(batch_frames=frames, transition=P, initial=pi, log_probs=log_probs, gpu=0)
        auto, dense = call(obs, route='auto', **model), call(obs, route='dense', **model)
        assert not any(torch.isnan(t).any() for t in auto + dense)
        if entry == 'state_posteriors':
            test_posterior_gpu.check([numbers(t) for t in auto], [numbers(t) for t in dense], ofc.FRAMES)
        else:
            test_counts_gpu.check_counts(auto[0], auto[1], numbers(dense[0]), numbers(dense[1]), ofc.FRAMES, T)
            loglik_close(auto[2], dense[2], ofc.FRAMES)
        if log_probs:
            assert state.peek(P).get(('band_over', S)) is not None      # P itself was looked at: whatever it holds as a log matrix
        else:
            check_look(P, 'band_tiny', log_probs=False)


# ---------------------------------------------------------------------------------------- streams
@pytest.mark.parametrize('route', ['dense', 'band'])
def test_streams_take_chunks_cut_on_the_device(route):
    """Every chunk of a push is `device_obs[:, a:b]`, frames int64 on the host: the outputs are those of an object fed
    contiguous chunks, bit for bit, and for StreamDecoder the whole-sequence `from_probabilities`."""
    p = ofc.problem('band')
    obs, matrix, pi = p[O].to(DEV), p[A].to(DEV), p[PI].to(DEV)
    second = torch.tensor(ofc.SECOND, dtype=torch.int64)
    before = ofc.Snapshot([obs])
    whole = torbi_amd.from_probabilities(obs.clone(), torch.tensor(ofc.STREAMED), matrix, pi, log_probs=True, gpu=0)
    outputs = []
    for contiguous in (False, True):
        dec = torbi_amd.StreamDecoder(B, S, matrix, pi, log_probs=True, gpu=0, route=route)
        sp = torbi_amd.StreamPosteriors(B, S, matrix, pi, log_probs=True, gpu=0, lag=ofc.LAG, route=route)
        assert dec.route == route and sp.route == route
        out = []
        for chunk, frames in ofc._pushes(obs, second):
            assert not chunk.is_contiguous()
            chunk = chunk.contiguous() if contiguous else chunk
            out += [*dec.push(chunk, frames), *sp.push(chunk, frames), sp.filtered(), sp.log_likelihood]
        paths = [torch.cat([out[b], out[2 * B + 2 + b], rest]) for b, rest in enumerate(dec.flush())]
        rows, final = sp.flush()
        outputs.append((*out, *paths, *rows, final))
        for b, n in enumerate(ofc.STREAMED):
            assert torch.equal(paths[b], whole[b, :n])
    ofc.same(*outputs)
    before.check()


# ---------------------------------------------------------------------------------------- one anchor per entry
def host_ops(entry):
    return {name: t.clone() for name, t in entry.plain().items()}


def numbers(t):
    return t.detach().cpu().numpy().astype(np.float64)


def anchor_decode(entry, got, o):
    obs = o[O].numpy()
    if entry.name == 'from_probabilities':
        obs = kc.clamp(obs)
    matrix = o[A].numpy() if A in o else np.full((S, S), ofc.UNIFORM, dtype=np.float32)
    want = oracle.decode(obs, o[F].numpy(), matrix, o[PI].numpy())
    assert np.array_equal(got[0].cpu().numpy(), want)


def anchor_posteriors(entry, got, o):
    import test_posterior_gpu
    obs = inputs.observation(o[O], True, CPU) if entry.name == 'state_posteriors' else o[O]
    gamma, L, _, _ = posterior._host(obs, o[F], o[A], None, o[PI])
    test_posterior_gpu.check((numbers(got[0]), numbers(got[1])), (gamma.numpy(), L.numpy()), ofc.FRAMES)


def anchor_counts(entry, got, o):
    import test_counts_gpu
    anchor_posteriors(entry, got, o)
    _, _, X, I = posterior._host(o[O], o[F], o[A], None, o[PI], o[W], counts=True)
    mine = torbi_amd.band_counts_to_dense(got[2], *ofc.BAND[:2]) if entry.band else got[2]
    test_counts_gpu.check_counts(mine, got[3], X.numpy(), I.numpy(), ofc.FRAMES, T)


def anchor_expected_counts(entry, got, o):
    import test_counts_gpu
    X, I, L = torbi_amd.expected_counts(o[O], o[F], o[A], o[PI], log_probs=True, gpu=None)
    test_counts_gpu.check_counts(got[0], got[1], numbers(X), numbers(I), ofc.FRAMES, T)


def anchor_log_likelihood(entry, got, o):
    import test_counts_gpu
    want = entry.call({name: (t.double() if t.dtype.is_floating_point else t) for name, t in o.items()}, None)
    L, dobs, dA, dpi = (numbers(t) for t in want)
    loglik_close(got[0], want[0], ofc.FRAMES)
    assert np.abs(numbers(got[1]) - dobs).max() <= 1e-4                 # (test_log_likelihood_gradients_match_the_float64_route's)
    test_counts_gpu.check_counts(got[2], got[3], dA, dpi, ofc.FRAMES, T)


def anchor_k_best(entry, got, o):
    # (the round trip as the device takes it: the host's exp and log differ from it in a last bit, and the scores are compared
    # bit for bit)
    obs = inputs.observation(o[O].to(DEV), True, DEV).cpu() if entry.name == 'best_paths' else o[O]
    want = torbi_amd.decode_k_best(obs, o[F], o[A], o[PI], K)                         # host tensors: the host route
    kc.same([t.cpu().numpy() for t in got], [t.numpy() for t in want])


def anchor_sampling(entry, got, o):
    import test_sample_band_gpu
    import test_sample_gpu
    obs = inputs.observation(o[O], True, CPU) if entry.name == 'sample_paths' else o[O]
    a, E, L, Fr, _ = sc.reference(obs, o[F], o[A], o[PI])
    if entry.band:
        test_sample_band_gpu.check_draws(entry.name, got[0].cpu(), o[U], (a, E, L, Fr), ofc.BAND[:2], ofc.BAND[2])
    else:                                       # (`sample_paths` under 'auto' goes dense at this shape: anchor_routes)
        test_sample_gpu.check_draws(entry.name, got[0].cpu(), got[1].cpu(), o[U], (a, E, L, Fr, None), obs.shape[2])
    loglik_close(got[1], L, ofc.FRAMES)


def anchor_stream_decoder(entry, got, o):
    want = oracle.decode(kc.clamp(o[O].numpy()), np.asarray(ofc.STREAMED, dtype=np.int32), o[A].numpy(), o[PI].numpy())
    for b, n in enumerate(ofc.STREAMED):                                            # (max_lag=None: the exact decoder)
        assert np.array_equal(got[b].cpu().numpy(), want[b, :n])
    assert int(got[B].sum()) == 0


def anchor_stream_posteriors(entry, got, o):
    n = np.asarray(ofc.STREAMED)
    gamma, L = spc.reference(o[O], n, o[A], o[PI], True)
    rest, final = got[-B - 1:-1], got[-1]
    for b in range(B):
        rows = numbers(rest[b])
        spc.same(rows, gamma[b, n[b] - rows.shape[0]:n[b]], spc.DEVICE_GAMMA, f'rows of stream {b}')
        spc.same(numbers(final[b]), L[b], spc.loglik_bound(L[b], n[b]), f'log-likelihood of stream {b}')


def anchor_routes(entry, got, o):
    # reach 3/2 of 64 states, -inf outside: posteriors and counts take every covered band; 6 diagonals of 64 states are
    # 135 of 1440, inside k-best's 175 at k = 2 and outside the 23 of sampling and of streaming posteriors; streaming
    # decode takes every covered band (the tables in torbi_amd/k_best.py, sampling.py, stream_posterior.py)
    assert got == ('band', 'band', 'dense', 'band', 'band', 'dense')


ANCHORS = {'decode': anchor_decode, 'decode_uniform': anchor_decode, 'from_probabilities': anchor_decode,
           'forward_backward': anchor_posteriors, 'forward_backward_banded': anchor_posteriors,
           'state_posteriors': anchor_posteriors, 'forward_backward_counts': anchor_counts,
           'forward_backward_counts_banded': anchor_counts, 'expected_counts': anchor_expected_counts,
           'log_likelihood': anchor_log_likelihood, 'decode_k_best': anchor_k_best, 'decode_k_best_banded': anchor_k_best,
           'best_paths': anchor_k_best, 'forward_sample': anchor_sampling, 'forward_sample_banded': anchor_sampling,
           'sample_paths': anchor_sampling, 'StreamDecoder-dense': anchor_stream_decoder,
           'StreamDecoder-band': anchor_stream_decoder, 'StreamPosteriors-dense': anchor_stream_posteriors,
           'StreamPosteriors-band': anchor_stream_posteriors, 'routes': anchor_routes}


@pytest.mark.parametrize('name', [e.name for e in ofc.ENTRIES if e.gpu])
def test_the_plain_call_against_the_host_route(name):
    entry = BY_NAME[name]
    _, plain, _ = ofc.operands(entry, DEV)
    ANCHORS[name](entry, ofc.reference(entry, plain, 0), host_ops(entry))


def test_every_row_has_an_anchor():
    assert set(ANCHORS) == {e.name for e in ofc.ENTRIES if e.gpu}
