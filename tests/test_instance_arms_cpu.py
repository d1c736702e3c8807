"""The table of tests/instance_arm_cases.py against the record of profiles/launch_sequence_ab.txt, without a device."""
import os
import re

from instance_arm_cases import CASES, FORWARD_FAMILIES, HELD_NOTE, batch, is_forward_instance, label

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RECORD = os.path.join(ROOT, 'profiles', 'launch_sequence_ab.txt')


def recorded_names():
    """The kernel names of the record's list `dispatches per kernel of the library ... 211 names:` (count, two spaces, name)."""
    with open(RECORD) as f:
        text = f.read()
    head = re.search(r'^dispatches per kernel of the library.*?(\d+) names:\n', text, re.M)
    names = re.findall(r'^\s+\d+  (\S.*?)\s*$', text[head.end():], re.M)
    assert len(names) == int(head.group(1)) == 211
    return names


def test_the_table_names_every_forward_instance_of_the_record_and_no_other():
    """profiles/launch_sequence_ab.txt lists the 211 kernels that one call per arm of every ladder dispatched.  The set of
    instances the table expects must EQUAL the forward kernels of that list -- the two wavefront forms, the workgroup form, the
    dense step, the time-resident forward instances (not the repair instances `<..., true>` behind a cluster launch), both
    band forms and the held kernel: an arm nobody wrote a case for shows here, and so does a case whose name no call ever
    dispatched.  The boundary shapes of the table map onto names that are in the set already.

    A new instance therefore needs a new row in tests/instance_arm_cases.py AND a new line in the record (from a kernel trace
    of a call that reaches it) together; either alone fails this test."""
    recorded = {n for n in recorded_names() if is_forward_instance(n)}
    assert all(n.startswith(FORWARD_FAMILIES) for n in recorded)
    expected = {c.kernel for c in CASES}
    assert expected - recorded == set(), 'cases whose instance the record does not list'
    assert recorded - expected == set(), 'recorded forward instances without a case'
    assert len(recorded) == 18 + 10 + 3 + 10 + 18 + 10 + 6      # small, block, dense, whole tiles, clusters, band, held


def test_the_table_is_well_formed():
    """Every record names a route and a path the host layer knows, reports its own instance (the held family: the note
    without template arguments), and its ids are distinct; the rules for the item count give the record's shapes at 256
    compute units (profiles/launch_sequence_ab.txt, `arm -> shape`)."""
    assert len({label(c) for c in CASES}) == len(CASES)
    for c in CASES:
        assert c.path in ('auto', 'dense', 'resident', 'cluster', 'band', 'held') and c.T == 3 and c.S >= 3
        assert c.reported == (HELD_NOTE if c.family == 'held' else c.kernel)
        assert (c.band is not None) == (c.family == 'band')
        assert all(k.startswith('TORBI_HIP_') and isinstance(v, str) for k, v in c.env.items())
    at_256 = {(c.family, batch(c, 256), c.S) for c in CASES}
    listed = {('dense', 32, 64), ('dense', 4160, 64), ('dense', 6400, 96), ('whole', 1, 64), ('whole', 1, 4096),
              ('cluster', 16, 2048), ('cluster', 512, 2048), ('cluster', 1024, 2048), ('cluster', 2048, 2048),
              ('cluster', 8, 4096), ('cluster', 256, 4096), ('cluster', 512, 3072), ('cluster', 512, 4096),
              ('cluster', 1024, 4096), ('band', 16, 256), ('band', 16, 1024), ('band', 16, 1440), ('band', 640, 1440),
              ('held', 1, 512), ('held', 1, 4096), ('small', 5, 3), ('block', 5, 256)}
    assert listed - at_256 == set()
