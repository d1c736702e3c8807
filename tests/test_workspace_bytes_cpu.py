"""Every byte query of the C ABI answers what tests/golden/workspace_bytes.json recorded (the commit named in the file,
tests/golden/generate_workspace_bytes.py): a change of a workspace layout's size shows here without a device."""
import json
import os

import pytest

from torbi_amd import _lib

RECORD = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'workspace_bytes.json')))
QUERIES = ('torbi_hip_workspace_bytes', 'torbi_hip_preparation_bytes', 'torbi_hip_stream_state_bytes',
           'torbi_hip_forward_backward_workspace_bytes', 'torbi_hip_forward_backward_band_workspace_bytes',
           'torbi_hip_k_best_workspace_bytes', 'torbi_hip_forward_backward_counts_workspace_bytes',
           'torbi_hip_forward_backward_counts_band_workspace_bytes', 'torbi_hip_k_best_band_workspace_bytes',
           'torbi_hip_sample_workspace_bytes', 'torbi_hip_sample_band_workspace_bytes',
           'torbi_hip_stream_band_diagonals_bytes')


def test_the_record_holds_every_byte_query_and_nothing_else():
    assert sorted(RECORD) == sorted(QUERIES + ('commit', 'compute_units'))
    assert RECORD['compute_units'] == 256 and len(RECORD['commit']) == 40
    assert all(len(RECORD[name]) > 0 for name in QUERIES)
    # ... and the record names every export of the library that answers in bytes
    assert sorted(QUERIES) == sorted(name for name, (restype, _) in _lib.SYMBOLS.items() if name.endswith('_bytes'))


@pytest.mark.parametrize('name', QUERIES)
def test_byte_counts_are_the_recorded_ones(name):
    lib = _lib.load()
    # the decode workspace alone depends on the device (the dense plan and the cluster exchange follow its compute units):
    # its entries hold where no device is visible (the library then assumes 256 units) and on a device with the recorded count
    if name == 'torbi_hip_workspace_bytes' and lib.torbi_hip_device_count() > 0:
        units = {lib.torbi_hip_compute_units(d) for d in range(lib.torbi_hip_device_count())}
        if units != {RECORD['compute_units']}:
            pytest.skip(f'devices with {sorted(units)} compute units; recorded with {RECORD["compute_units"]}')
    query = getattr(lib, name)
    wrong = [(args, want, query(*args)) for *args, want in RECORD[name] if query(*args) != want]
    assert not wrong, f'{len(wrong)} of {len(RECORD[name])} differ; first (arguments, recorded, now): {wrong[:5]}'
