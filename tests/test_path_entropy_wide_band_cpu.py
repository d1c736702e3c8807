"""The C-ABI surface, the Python front and the routing of the wide band route of path entropy
(torbi_hip_path_entropy_wide_band*, entropy.forward_entropy_wide_banded, entropy.path_entropy(route=)) without a device."""
import math
import os
import re

import numpy as np
import pytest
import torch

import torbi_amd
from torbi_amd import _lib, band_route, entropy, inputs, viterbi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NINF = -math.inf
TINY = float(np.log(np.finfo(np.float32).tiny))
NAMES = ('torbi_hip_path_entropy_wide_band_covers', 'torbi_hip_path_entropy_wide_band_workspace_size',
         'torbi_hip_path_entropy_wide_band_tile', 'torbi_hip_path_entropy_wide_band')


def test_symbols_and_exports():
    header = open(os.path.join(ROOT, 'include', 'torbi_hip.h')).read()
    lib = _lib.load()
    for name in NAMES:
        assert re.search(r'\b(?:int|size_t) ' + name + r'\s*\(', header), name
        assert name in _lib.SYMBOLS and callable(getattr(lib, name)) and not name.endswith('_bytes')
    for name in ('forward_entropy_wide_banded', 'path_entropy_wide_banded_workspace_bytes'):
        assert name in entropy.__all__ and callable(getattr(entropy, name)) and name not in torbi_amd.__all__


@pytest.mark.parametrize('case,want', [
    ((512, 500, 1440, 87, 87, NINF), 1), ((512, 500, 1440, 87, 87, TINY), 1), ((4, 10, 4096, 255, 256, NINF), 1),
    ((3, 5, 37, 1000, 1000, -3.0), 1),                                      # clamped to the matrix
    ((3, 12, 64, 2, 5, NINF), 1),                                            # a narrow band: one kernel, not a patch
    ((4, 10, 4096, 256, 256, NINF), 0),                                      # W = 513
    ((4, 10, 4097, 8, 8, NINF), 0), ((4, 10, 1440, 87, 87, math.nan), 0), ((4, 10, 1440, 87, 87, math.inf), 0),
    ((4, 10, 1440, -1, 87, NINF), 0), ((4, 10, 1440, 87, -1, NINF), 0), ((0, 10, 1440, 87, 87, NINF), 0)])
def test_covers(case, want):
    assert _lib.load().torbi_hip_path_entropy_wide_band_covers(*case, -1) == want


def test_workspace_size():
    need = _lib.load().torbi_hip_path_entropy_wide_band_workspace_size
    sizes = [need(8, 60, 1440, reach, reach) for reach in (11, 40, 87, 255)]
    assert all(n > 0 and n % 256 == 0 for n in sizes) and sizes == sorted(set(sizes))
    assert sizes[2] == entropy.path_entropy_wide_banded_workspace_bytes(8, 60, 1440, 87, 87)
    # both packs of 6 blocks x 44 dquads x 4 KiB; m, c and the prefix of 8 x 60 floats up to 256 bytes; the flag; room to
    # align the base
    assert sizes[2] == 2 * 6 * 44 * 4096 + 3 * 2048 + 256 + 256


@pytest.mark.parametrize('route', band_route.ROUTES)
@pytest.mark.parametrize('band,runner', [((40, 30, -20.), 'wide'), ((1, 2, -20.), 'narrow')])
def test_routing(monkeypatch, route, band, runner):
    """A band of more than 64 entries goes to the wide runner under 'band', a narrower one to the narrow runner; 'dense' asks
    for no plan; one plan, one look and one question to the covers of the band's own route per call."""
    asked = {'plan': 0, 'look': 0, 'narrow': 0, 'wide': 0}
    plan = band_route.plan

    def count(key, answer):
        def counted(*args, **kwargs):
            asked[key] += 1
            return answer(*args, **kwargs) if callable(answer) else answer
        return counted

    monkeypatch.setattr(band_route, 'plan', count('plan', plan))
    monkeypatch.setattr(viterbi, 'band_over', count('look', band))
    monkeypatch.setattr(entropy, '_covered', count('narrow', True))
    monkeypatch.setattr(entropy, '_wide_covered', count('wide', True))
    monkeypatch.setattr(inputs, '_compute_device', lambda gpu: torch.device('cpu'))
    monkeypatch.setattr(entropy, '_run', lambda *args: 'dense')
    monkeypatch.setattr(entropy, '_run_band', lambda *args: 'narrow')
    monkeypatch.setattr(entropy, '_run_wide_band', lambda *args: 'wide')
    g = torch.Generator().manual_seed(1)
    obs, A = torch.softmax(torch.randn(2, 4, 72, generator=g), 2), torch.softmax(torch.randn(72, 72, generator=g), 0)
    got = entropy.path_entropy(obs, transition=A, gpu=0, route=route)
    if route == 'dense':
        assert got == 'dense' and not any(asked.values())
        return
    pays = (entropy._wide_band_pays if runner == 'wide' else entropy._band_pays)(2, 72, *band[:2])
    assert got == (runner if route == 'band' or pays else 'dense')
    assert asked == {'plan': 1, 'look': 1, 'narrow': int(runner == 'narrow'), 'wide': int(runner == 'wide')}
    assert entropy.path_entropy_route(A, 2, 4, 72, gpu=0) == ('band' if pays else 'dense')


def test_the_wide_refusal_names_the_wide_entry(monkeypatch):
    monkeypatch.setattr(viterbi, 'band_over', lambda *args: (40, 30, -20.))
    monkeypatch.setattr(inputs, '_compute_device', lambda gpu: torch.device('cpu'))
    monkeypatch.setattr(entropy, '_wide_covered', lambda *args: False)
    monkeypatch.setattr(entropy, '_run', lambda *args: 'dense')
    obs, A = torch.full((2, 4, 72), 1 / 72), torch.full((72, 72), 1 / 72)
    with pytest.raises(RuntimeError) as raised:
        entropy.path_entropy(obs, transition=A, gpu=0, route='band')
    assert str(raised.value) == ("path_entropy(route='band'): torbi_hip_path_entropy_wide_band_covers turns down batch=2, "
                                 'frames=4, states=72, reach 40/30, background -20.0')
    assert entropy.path_entropy(obs, transition=A, gpu=0, route='auto') == 'dense'


def test_auto_classes_lie_inside_what_was_measured():
    """tools/path_entropy_wide_band_probe.py measured 1 to 4096 items on the 175 diagonals of 1440 states."""
    for low, high, diagonals in entropy._AUTO_WIDE_BAND:
        assert 1 <= low <= high <= 4096 and diagonals <= 175
    assert not entropy._wide_band_pays(4097, 1440, 87, 87) and not entropy._wide_band_pays(1, 1440, 88, 87)
