"""A decode workspace that is not 256-byte aligned is an error code, not undefined behaviour (include/torbi_hip.h): every
decode entry point answers TORBI_HIP_EINVAL before it touches a device.  The other routes take any base, and all of them
refuse a workspace one byte short of their size query.

No device is needed and none is used: the pointers are dummy addresses that nothing dereferences, and the device index is
one no machine has, so a call whose arguments pass ends where it selects its device, with a HIP error code -- on a machine
with devices as on one without."""
import ctypes

import pytest

from torbi_amd import _lib

EINVAL, EWORKSPACE = -1, -2
ALIGNED = 1 << 20               # a 256-byte aligned dummy address
PTR = 1 << 16                   # ... and one for every other pointer argument
NO_DEVICE = 63                  # inside the library's table of devices, beyond any machine's
B, T, S = 17, 5, 64
PLENTY = 1 << 40                # workspace_bytes: more than any layout of this shape


def calls(lib, base):
    """(name, thunk) of every entry point that takes a decode workspace, with `base` as that workspace."""
    table = (_lib.Batch * 1)(_lib.Batch(PTR, PTR, PTR, base, PLENTY, B, T))
    phases = (ctypes.c_float * 6)()
    filled = ctypes.c_int(0)
    one = (PTR, PTR, PTR, PTR, PTR, base, PLENTY, B, T, S, NO_DEVICE, None)
    group = (table, 1, PTR, PTR, S)
    return [
        ('torbi_hip_viterbi_decode', lambda: lib.torbi_hip_viterbi_decode(*one)),
        ('torbi_hip_viterbi_decode_ex', lambda: lib.torbi_hip_viterbi_decode_ex(*one, 0)),
        ('torbi_hip_viterbi_decode_profiled', lambda: lib.torbi_hip_viterbi_decode_profiled(*one, 0, phases)),
        ('torbi_hip_viterbi_decode_batches', lambda: lib.torbi_hip_viterbi_decode_batches(*group, NO_DEVICE, None, 0, phases)),
        ('torbi_hip_viterbi_decode_banded',
         lambda: lib.torbi_hip_viterbi_decode_banded(*group, 2, 1, NO_DEVICE, None, 0, phases)),
        ('torbi_hip_viterbi_decode_banded_over',
         lambda: lib.torbi_hip_viterbi_decode_banded_over(*group, 2, 1, ctypes.c_float(-20.), NO_DEVICE, None, 0, phases)),
        ('torbi_hip_viterbi_decode_batches_prepared',
         lambda: lib.torbi_hip_viterbi_decode_batches_prepared(*group, NO_DEVICE, None, 0, phases, None, 0,
                                                               ctypes.byref(filled))),
    ]


NAMES = [name for name, _ in calls(_lib.load(), ALIGNED)]


@pytest.mark.parametrize('name', NAMES)
@pytest.mark.parametrize('off', [4, 1, 128, 255])
def test_a_misaligned_decode_workspace_is_an_invalid_argument(name, off):
    lib = _lib.load()
    assert dict(calls(lib, ALIGNED + off))[name]() == EINVAL


@pytest.mark.parametrize('name', NAMES)
def test_an_aligned_decode_workspace_gets_past_the_argument_checks(name):
    lib = _lib.load()
    rc = dict(calls(lib, ALIGNED))[name]()
    assert rc not in (EINVAL, EWORKSPACE), rc
    assert rc > 0, rc                   # a HIP error code: the device index does not exist


def test_the_size_is_looked_at_first():
    """A workspace that is too small is TORBI_HIP_EWORKSPACE wherever it lies, as it was before the alignment was checked;
    exactly the size the query names is enough for the alignment to be looked at."""
    lib = _lib.load()
    need = lib.torbi_hip_workspace_bytes(B, T, S)
    args = lambda base, nbytes: (PTR, PTR, PTR, PTR, PTR, base, nbytes, B, T, S, NO_DEVICE, None)
    assert lib.torbi_hip_viterbi_decode(*args(ALIGNED, need - 1)) == EWORKSPACE
    assert lib.torbi_hip_viterbi_decode(*args(ALIGNED + 4, need - 1)) == EWORKSPACE
    assert lib.torbi_hip_viterbi_decode(*args(ALIGNED + 4, need)) == EINVAL
    assert lib.torbi_hip_viterbi_decode(*args(ALIGNED, need)) > 0
    # an empty batch brings no workspace
    assert lib.torbi_hip_viterbi_decode(PTR, PTR, PTR, PTR, PTR, ALIGNED + 4, 0, 0, T, S, NO_DEVICE, None) == 0


def test_python_raises_its_usual_error():
    lib = _lib.load()
    rc = lib.torbi_hip_viterbi_decode(PTR, PTR, PTR, PTR, PTR, ALIGNED + 4, PLENTY, B, T, S, NO_DEVICE, None)
    with pytest.raises(RuntimeError, match='256-byte aligned'):
        _lib.check(rc, 'torbi_hip_viterbi_decode')


def test_the_other_routes_take_any_base_and_refuse_one_byte_less_than_their_size():
    """Forward-backward, counts, k-best, sampling and their band routes round the caller's base up themselves: an odd base is
    no error, and with exactly the bytes their size query names they get past the argument checks; with one byte less they
    answer TORBI_HIP_EWORKSPACE."""
    lib = _lib.load()
    B, T, S, left, right, k, draws = 3, 6, 72, 2, 1, 3, 5
    p, dev, bg, value = PTR, NO_DEVICE, ctypes.c_float(-20.), ctypes.c_float(-4.)
    calls = [
        (lib.torbi_hip_forward_backward_workspace_bytes(B, T, S),
         lambda w, n: lib.torbi_hip_forward_backward(p, p, p, p, p, p, w, n, B, T, S, dev, None)),
        (lib.torbi_hip_forward_backward_workspace_bytes(B, T, S),
         lambda w, n: lib.torbi_hip_forward_backward_uniform(p, p, value, p, p, p, w, n, B, T, S, dev, None)),
        (lib.torbi_hip_forward_backward_counts_workspace_bytes(B, T, S),
         lambda w, n: lib.torbi_hip_forward_backward_counts(p, p, p, p, None, p, p, p, p, w, n, B, T, S, dev, None)),
        (lib.torbi_hip_forward_backward_band_workspace_bytes(B, T, S, left, right),
         lambda w, n: lib.torbi_hip_forward_backward_band(p, p, p, p, left, right, bg, p, p, w, n, B, T, S, dev, None)),
        (lib.torbi_hip_forward_backward_counts_band_workspace_bytes(B, T, S, left, right),
         lambda w, n: lib.torbi_hip_forward_backward_counts_band(p, p, p, p, left, right, bg, None, p, p, p, p, w, n, B, T, S,
                                                                 dev, None)),
        (lib.torbi_hip_k_best_workspace_bytes(B, T, S, k),
         lambda w, n: lib.torbi_hip_k_best(p, p, p, p, p, p, w, n, B, T, S, k, dev, None)),
        (lib.torbi_hip_k_best_workspace_bytes(B, T, 1, k),
         lambda w, n: lib.torbi_hip_k_best_uniform(p, p, value, p, p, p, w, n, B, T, S, k, dev, None)),
        (lib.torbi_hip_k_best_band_workspace_bytes(B, T, S, k, left, right),
         lambda w, n: lib.torbi_hip_k_best_band(p, p, p, p, left, right, bg, p, p, w, n, B, T, S, k, dev, None)),
        (lib.torbi_hip_sample_workspace_bytes(B, T, S, draws, 0),
         lambda w, n: lib.torbi_hip_sample(p, p, p, p, p, p, p, w, n, B, T, S, draws, dev, None)),
        (lib.torbi_hip_sample_workspace_bytes(B, T, S, draws, 1),
         lambda w, n: lib.torbi_hip_sample_uniform(p, p, value, p, p, p, p, w, n, B, T, S, draws, dev, None)),
        (lib.torbi_hip_sample_band_workspace_bytes(B, T, S, draws, left, right),
         lambda w, n: lib.torbi_hip_sample_band(p, p, p, p, left, right, bg, p, p, p, w, n, B, T, S, draws, dev, None)),
    ]
    for need, call in calls:
        assert need > 256
        for base in (ALIGNED, ALIGNED + 1, ALIGNED + 4):
            assert call(base, need - 1) == EWORKSPACE
            assert call(base, need) > 0             # a HIP error code: the device index does not exist
