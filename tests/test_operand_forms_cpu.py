"""Operands as callers hold them -- strided, offset, float64 / float16 / bfloat16 / int64 -- through the `gpu=None` routes and
`decode_cpu`, against the same entry on plain copies, bit for bit (tests/operand_form_cases.py has the forms and the table of
entries); tests/test_operand_forms_gpu.py runs the same table on an MI355X.

Without a device this module also pins what the device fronts do BEFORE a kernel runs:
* `viterbi.band_over` / `band_reach` read S * S float32 words, row-major, behind a pointer, so they refuse any other tensor
  before they reach the device look.  A transposed view of an asymmetric band would otherwise be read as the mirrored band,
  a float64 matrix as pairs of float32 words, and a half-precision matrix past its end;
* every front with a band planner hands it `inputs.device_matrix`'s tensor -- float32, contiguous, 16-byte aligned, the
  values of the caller's matrix -- as the matrix AND as the tensor the look is remembered with, and hands its kernels the
  same object.  The fronts run here with the compute device substituted by the host and the kernel calls by recorders;
* one tensor object used with `log_probs=False` and then `log_probs=True` is looked at as two matrices;
* the table names every public entry that takes an observation.
"""
import gc
import weakref

import pytest
import torch

import torbi_amd
from torbi_amd import inputs, k_best, posterior, sampling, state, training, viterbi

import operand_form_cases as ofc
from operand_form_cases import A, B, BY_NAME, DRAWS, K, S, T

CPU = torch.device('cpu')
CASES = ofc.cases(CPU, cpu_only=True)
MATRIX_FORMS = [name for name in ofc.FORMS[A] if name not in ('plain', 'host')]


@pytest.mark.parametrize('name,operand,form_name', CASES, ids=['-'.join(c) for c in CASES])
def test_a_form_equals_its_plain_copy_and_nothing_is_written(name, operand, form_name):
    ofc.check_forms(BY_NAME[name], CPU, None, {operand: form_name})


@pytest.mark.parametrize('name', [e.name for e in ofc.ENTRIES if e.cpu])
def test_every_operand_in_another_form_at_once(name):
    entry = BY_NAME[name]
    ofc.check_forms(entry, CPU, None, {operand: ofc.TOGETHER[operand] for operand in entry.operands})


def test_the_table_names_every_public_entry_that_takes_an_observation():
    tabled = {name for entry in ofc.ENTRIES for name in entry.api}
    assert tabled <= set(torbi_amd.__all__) and set(ofc.NOT_TABLED) <= set(torbi_amd.__all__)
    for name in torbi_amd.__all__:
        if ofc.takes_an_observation(getattr(torbi_amd, name)):
            assert name in tabled or name in ofc.NOT_TABLED, f'{name} takes an observation and has no row in ENTRIES'
    for entry in ofc.ENTRIES:                                    # a row states what it does not take, not a test body
        assert set(entry.operands) <= set(ofc.KINDS) and set(entry.raises) <= set(entry.operands)
        assert entry.cpu or entry.gpu


# ---------------------------------------------------------------------------------------- the look refuses what it cannot read
@pytest.mark.parametrize('device', ['cpu', 'meta'])
@pytest.mark.parametrize('form_name', MATRIX_FORMS)
@pytest.mark.parametrize('look', ['band_over', 'band_reach'])
def test_the_look_refuses_what_it_cannot_read(monkeypatch, look, form_name, device):
    def never(*args):
        pytest.fail('the device look was reached')
    monkeypatch.setattr(viterbi, '_device_look', never)
    matrix, _ = ofc.form(form_name, ofc.problem('band')[A], CPU)
    if device == 'meta':                                         # (strides, offset and dtype of the form on a device without memory)
        matrix = torch.empty_strided(matrix.shape, matrix.stride(), dtype=matrix.dtype, device='meta')
    if matrix.dtype == torch.float32 and matrix.is_contiguous():
        assert getattr(viterbi, look)(matrix, matrix, S) is None           # offset4: readable, and asked of aligned device tensors only
        return
    with pytest.raises(RuntimeError, match=f'viterbi.{look} reads a contiguous float32 matrix'):
        getattr(viterbi, look)(matrix, matrix, S)


# ---------------------------------------------------------------------------------------- what the fronts hand the planner
class Recorder:
    """`viterbi.band_over` recorded, then asked for real (so its refusal is part of the test), and the kernel calls of the
    fronts replaced by recorders of the matrix they were handed."""

    def __init__(self, monkeypatch):
        self.looked, self.ran = [], []
        real = viterbi.band_over
        monkeypatch.setattr(inputs, '_compute_device', lambda gpu: CPU)
        monkeypatch.setattr(viterbi, '_device_look', lambda *args: pytest.fail('the device look was reached'))

        def band_over(trans, original, states):
            self.looked.append((trans, original))
            return real(trans, original, states)

        monkeypatch.setattr(viterbi, 'band_over', band_over)
        for module, name, at in ((posterior, '_run', 2), (posterior, '_run_band', 2), (training, '_run', 2),
                                 (training, '_run_band_counts', 2), (k_best, '_run', 2), (k_best, '_run_band', 2),
                                 (sampling, '_run', 2), (sampling, '_run_band', 2)):
            monkeypatch.setattr(module, name, self.runner(at))

    def runner(self, at):
        def run(*args, **kwargs):
            self.ran.append(args[at])
            zero = torch.zeros(())
            return zero, zero, zero, zero
        return run


def fronts(matrix, log_probs=True):
    """name -> a call of every front that has a band planner and can be run without a device."""
    obs = ofc.problem('band')[ofc.O]
    if not log_probs:
        obs = torch.exp(obs)
    model = dict(transition=matrix, log_probs=log_probs, gpu=0)
    return {
        'state_posteriors': lambda: torbi_amd.state_posteriors(obs, route='auto', **model),
        'posterior_route': lambda: torbi_amd.posterior_route(matrix, B, T, S, gpu=0, log_probs=log_probs),
        'expected_counts': lambda: torbi_amd.expected_counts(obs, route='auto', **model),
        'counts_route': lambda: torbi_amd.counts_route(matrix, B, T, S, gpu=0, log_probs=log_probs),
        'best_paths': lambda: torbi_amd.best_paths(obs, K, route='auto', **model),
        'k_best_route': lambda: torbi_amd.k_best_route(matrix, B, T, S, K, gpu=0, log_probs=log_probs),
        'sample_paths': lambda: torbi_amd.sample_paths(obs, DRAWS, route='auto', **model),
        'sample_route': lambda: torbi_amd.sample_route(matrix, B, T, S, draws=DRAWS, gpu=0, log_probs=log_probs),
        'stream_route': lambda: torbi_amd.stream_route(matrix, B, S, gpu=0, log_probs=log_probs),
        'stream_posterior_route': lambda: torbi_amd.stream_posterior_route(matrix, B, S, gpu=0, log_probs=log_probs),
    }


FRONTS = list(fronts(None))


def check_looked(recorder, want, front):
    """One look, at a float32, contiguous, 16-byte aligned tensor with the values `want`, remembered with that tensor; the
    kernel call, if the front makes one, is handed the same object."""
    assert len(recorder.looked) == 1, (front, len(recorder.looked))
    trans, original = recorder.looked[0]
    assert original is trans, front
    assert trans.dtype == torch.float32 and trans.is_contiguous() and trans.data_ptr() % 16 == 0, front
    assert torch.equal(ofc.bits(trans), ofc.bits(want)), front
    assert all(ran is trans for ran in recorder.ran) and len(recorder.ran) == int(not front.endswith('_route')), front


@pytest.mark.parametrize('form_name', ['plain'] + MATRIX_FORMS)
@pytest.mark.parametrize('front', FRONTS)
def test_fronts_hand_the_planner_and_the_kernels_one_plain_matrix(monkeypatch, front, form_name):
    recorder = Recorder(monkeypatch)
    matrix, base = ofc.form(form_name, ofc.problem('band')[A], CPU)
    snapshot = ofc.Snapshot([matrix, base])
    fronts(matrix)[front]()
    check_looked(recorder, ofc.plain_copy(matrix, CPU), front)
    if form_name == 'plain':
        assert recorder.looked[0][0] is matrix                       # a plain matrix is looked at where it is
    snapshot.check(front)


@pytest.mark.parametrize('front', FRONTS)
def test_one_object_with_two_meanings_is_looked_at_as_two_matrices(monkeypatch, front):
    """`log_probs=False`, then the same tensor object with `log_probs=True`: the look -- and the note it leaves -- belongs to
    the matrix that was prepared, log(P) first and P itself second, never to the caller's object under one key."""
    recorder = Recorder(monkeypatch)
    P = torch.exp(ofc.problem('band_tiny')[A])                        # positive, one value outside the band
    fronts(P, log_probs=False)[front]()
    check_looked(recorder, torch.log(P), front)
    first = recorder.looked[0][0]
    recorder.looked.clear(), recorder.ran.clear()
    fronts(P, log_probs=True)[front]()
    check_looked(recorder, P, front)
    assert recorder.looked[0][0] is P and first is not P
    recorder.looked.clear(), recorder.ran.clear()
    fronts(P, log_probs=False)[front]()                                # ... and the first meaning's matrix is still the same object
    assert recorder.looked[0][0] is first


# ---------------------------------------------------------------------------------------- inputs.plain_matrix
def test_plain_matrix_copies_once_and_keeps_what_is_plain():
    plain = ofc.problem('band')[A].clone()
    assert inputs.plain_matrix(plain) is plain and inputs.device_matrix(plain, True, CPU) is plain
    for form_name in MATRIX_FORMS:
        matrix, _ = ofc.form(form_name, plain, CPU)
        copy = inputs.plain_matrix(matrix)
        assert copy is not matrix and copy.dtype == torch.float32 and copy.is_contiguous() and copy.data_ptr() % 16 == 0
        assert torch.equal(ofc.bits(copy), ofc.bits(ofc.plain_copy(matrix, CPU))), form_name
        assert inputs.plain_matrix(matrix) is copy                     # remembered with the tensor ...
        if matrix.dtype == torch.float32:
            matrix[0, 0] = -1.                                         # ... at this version
            again = inputs.plain_matrix(matrix)
            assert again is not copy and float(again[0, 0]) == -1.
    grad = plain.clone().requires_grad_()
    assert not inputs.plain_matrix(grad.t()).requires_grad


def test_a_matrix_is_not_kept_alive_by_its_own_notes():
    """`_prepared_transition` used to note a log matrix that is already on the device under itself: tensor -> notes -> tensor."""
    plain = ofc.problem('band')[A].clone()
    assert inputs.device_matrix(plain, True, CPU) is plain
    assert state.peek(plain) == {}
    gone = weakref.ref(plain)
    del plain
    gc.collect()
    assert gone() is None
