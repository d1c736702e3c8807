"""One record per arm of the Viterbi instance ladders of csrc/torbi_hip.hip (csrc/dispatch.hpp): the smallest call that
reaches the arm, and the instance that has to run.  Plain data, no device; tests/test_instance_arms_gpu.py decodes every record
and tests/test_instance_arms_cpu.py compares the names with the list of profiles/launch_sequence_ab.txt.

The names are written by hand from the rules' text (launch_small, launch_block, launch_dense_forward, launch_whole_tiles,
run_resident, run_band, held_instance; DESIGN.md sections 4-5), never asked of the library.  The arithmetic behind each is
beside the record: nrg = row groups of a posterior row (16 next-states each on 16-item tiles, 32 on 8-item tiles above 2048
states), R = members of a cluster (compute units // tiles, at most 16), share = ceil(nrg / R), passes = ceil(share / 12).

A NEW INSTANCE NEEDS A NEW RECORD HERE AND A NEW LINE IN profiles/launch_sequence_ab.txt TOGETHER: the completeness test fails
on either alone.

Item counts that depend on the device are written as a rule of its compute units (`batch`): the listed shape comes out at 256
units, and on any other device the same tiles per unit.  A device on which the rule still picks another instance fails the
case; nothing skips."""
from collections import namedtuple

Case = namedtuple('Case', 'family kernel reported path route env seeds band items T S launches')
# family    the ladder ('small', 'block', 'dense', 'whole', 'cluster', 'band', 'held')
# kernel    the instance as rocprofv3 spells it in profiles/launch_sequence_ab.txt
# reported  what torbi_hip_last_forward_kernel says behind the call: `kernel`, except for the held family (its note carries no
#           template arguments and tests/test_workspace_bounds_gpu.py is keyed by the short name, so it stays as it is)
# path      decode(path=...)
# route     viterbi.ROUTES name the profile has to report
# env       environment switches of the library, read per launch
# seeds     None (the library's default), 'few' (TORBI_HIP_FEW_SEEDS: KR = 1) or 'many' (TORBI_HIP_MANY_SEEDS: KR = 3), set
#           through viterbi._depth_record
# band      None, or (reach_left, reach_right, value outside the band)
# items     how many items: ('items', n) | ('tiles', items per tile, R): n = items per tile * (units // R)
#           | ('dense', a, b, c): 64 * (units * a // b + c) | ('band', c): 16 * (units // 8 + c)
# launches  forward launches the profile has to report, or None

INF = float('-inf')
HELD_NOTE = 'held::held_forward_kernel'


def batch(case, units):
    """Items of `case` on a device with `units` compute units."""
    rule = case.items
    if rule[0] == 'items':
        return rule[1]
    if rule[0] == 'tiles':
        return rule[1] * (units // rule[2])
    if rule[0] == 'dense':
        return 64 * (units * rule[1] // rule[2] + rule[3])
    if rule[0] == 'band':
        return 16 * (units // 8 + rule[1])
    raise ValueError(rule)


def label(case):
    """A readable pytest id: family, shape at 256 units, what distinguishes the call."""
    name = case.kernel.split('::')[1].replace(' ', '')
    extra = ''.join(f'-{k[10:].lower()}={v}' for k, v in sorted(case.env.items()))
    if case.seeds:
        extra += '-' + case.seeds
    return f'{case.family}-{batch(case, 256)}x{case.T}x{case.S}-{name}{extra}'


CASES = []


def _add(family, kernel, path, route, S, items=('items', 1), T=3, env=None, seeds=None, band=None, launches=None, reported=None):
    CASES.append(Case(family, kernel, reported or kernel, path, route, dict(env or {}), seeds, band, items, T, S, launches))


# ---- up to 64 states: launch_small.  SP = padded_states(S) (4, else the next multiple of 8); CH = 16 up to SP 16, 8 up to 40,
# else 4; TORBI_HIP_SMALL_VALUE picks the form
for S, SP, CH in ((3, 4, 16), (8, 8, 16), (16, 16, 16), (24, 24, 8), (32, 32, 8), (40, 40, 8), (48, 48, 4), (56, 56, 4),
                  (64, 64, 4)):
    _add('small', f'small::decode_kernel<{SP}, {CH}>', 'auto', 'small', S, ('items', 5), env={'TORBI_HIP_SMALL_VALUE': '0'},
         launches=1)
    _add('small', f'small::decode_value_kernel<{SP}, {CH}>', 'auto', 'small', S, ('items', 5), env={'TORBI_HIP_SMALL_VALUE': '1'},
         launches=1)

# ---- 65 .. 256 states: launch_block.  PQ = ceil(S / 64) pieces of the prev-states; L = 48 row registers where a piece holds
# at most 48 states (and PQ < 4), else 64; NSEQ = 2 with TORBI_HIP_BLOCK_PAIRS=1
for S, PQ, L in ((96, 2, 48), (128, 2, 64), (144, 3, 48), (192, 3, 64), (256, 4, 64)):
    for pairs in (0, 1):
        _add('block', f'small::block_value_kernel<{PQ}, {L}, {pairs + 1}>', 'auto', 'small', S, ('items', 5),
             env={'TORBI_HIP_BLOCK_PAIRS': str(pairs)}, launches=2)         # (the forward launch and the backtrace's)

# ---- dense: launch_dense_forward, JL of dense::make_plan = the JL in 6, 4, 2 with the least rounds * 8 JL, rounds =
# ceil(batch tiles of 64 items x ceil(S / 8 JL) / units), the larger JL on a draw
#   one batch tile, 64 states: one round whatever JL -> 2
_add('dense', 'dense::step_dense_kernel<8, 2, 8, 12, 8>', 'dense', 'dense', 64, ('items', 32), launches=2)
#   units // 4 + 1 batch tiles, 64 states: JL 6 and 4 one round (2 state tiles), JL 2 two (4 state tiles) -> 4
_add('dense', 'dense::step_dense_kernel<8, 4, 8, 12, 8>', 'dense', 'dense', 64, ('dense', 1, 4, 1), launches=2)
#   25/64 units batch tiles, 96 states: JL 6 one round (2 state tiles: 48), JL 4 two (3: 64), JL 2 three (6: 48, a draw) -> 6
_add('dense', 'dense::step_dense_kernel<8, 6, 8, 12, 8>', 'dense', 'dense', 96, ('dense', 25, 64, 0), launches=2)

# ---- whole tiles: launch_whole_tiles, one item, path 'resident'.  16-item tiles: MAXP 6 up to nrg 72, 8 up to 96, else 11;
# 8-item tiles: 8 up to nrg 96, else 11.  The arms with KR 1 and 3, the thresholds and the lane quad above them with one each.
FEW, MANY = ('few', 1), ('many', 3)
for S, MAXP, NI, kept in ((64, 6, 16, (FEW, MANY)),          # nrg 4
                          (1152, 6, 16, (FEW,)),             # nrg 72: the last one of MAXP 6
                          (1156, 8, 16, (MANY,)),            # nrg 73
                          (1536, 8, 16, (FEW, MANY)),        # nrg 96: the last one of MAXP 8
                          (1540, 11, 16, (FEW,)),            # nrg 97
                          (2048, 11, 16, (FEW, MANY)),       # nrg 128
                          (3072, 8, 8, (FEW, MANY)),         # nrg 96 of 32 next-states: the last one of MAXP 8
                          (3076, 11, 8, (MANY,)),            # nrg 97
                          (4096, 11, 8, (FEW, MANY))):       # nrg 128
    for seeds, KR in kept:
        _add('whole', f'resident::resident_forward_kernel<12, {MAXP}, true, {KR}, false, {NI}, false>', 'resident', 'resident',
             S, seeds=seeds, launches=1)

# ---- clusters: run_resident, path 'cluster', items per tile x (units // R) items -> R = 8, 4, 2 members.
# 16-item tiles: twelve waves, MAXP 1 | 2 | 4 | 6 for passes <= 1 | 2 | 4 | more.
# 8-item tiles: eight waves with MAXP 1 | 2 for share <= 8 | 16, else twelve with MAXP 2 | 4 | 6 for passes <= 2 | 4 | more.
# The arms with KR 1 (the cluster form's default) and KR 3; both sides of every step of the ladders with KR 1.
CLUSTER = (
    # (S, NI, R, KW, MAXP, both KR); R 16: ONE tile, which has min(units, 16) members
    (2048, 16, 16, 12, 1, True),       # nrg 128, share 8, one pass
    (1536, 16, 8, 12, 1, False),       # nrg 96, share 12: the last one of one pass
    (1552, 16, 8, 12, 2, False),       # nrg 97, share 13, two passes (ceil(97 / 8) is 13 from 1537 states; the next multiple of 16)
    (2048, 16, 8, 12, 2, True),        # share 16, two passes
    (1536, 16, 4, 12, 2, False),       # share 24: the last one of two passes
    (1552, 16, 4, 12, 4, False),       # share 25, three passes
    (2048, 16, 4, 12, 4, True),        # share 32, three passes
    (1536, 16, 2, 12, 4, False),       # share 48: the last one of four passes
    (1552, 16, 2, 12, 6, False),       # share 49, five passes
    (2048, 16, 2, 12, 6, True),        # share 64, six passes
    (4096, 8, 16, 8, 1, True),         # nrg 128, share 8: the last one of <8, 1>
    (2080, 8, 8, 8, 2, False),         # nrg 65, share 9 (share 8 on 8 members would be 2048 states: 16-item tiles)
    (4096, 8, 8, 8, 2, True),          # share 16: the last one of <8, 2>
    (2176, 8, 4, 12, 2, False),        # nrg 68, share 17, two passes of twelve
    (3072, 8, 4, 12, 2, True),         # nrg 96, share 24: the last one of two passes
    (3104, 8, 4, 12, 4, False),        # nrg 97, share 25, three passes
    (4096, 8, 4, 12, 4, True),         # share 32, three passes
    (3072, 8, 2, 12, 4, False),        # share 48: the last one of four passes
    (3104, 8, 2, 12, 6, False),        # share 49, five passes
    (4096, 8, 2, 12, 6, True),         # share 64, six passes
)
for S, NI, R, KW, MAXP, both in CLUSTER:
    for seeds, KR in ((None, 1), ('many', 3)) if both else ((None, 1),):
        _add('cluster', f'resident::resident_forward_kernel<{KW}, {MAXP}, true, {KR}, true, {NI}, false>', 'cluster', 'cluster',
             S, ('tiles', NI, R) if R < 16 else ('items', NI), seeds=seeds, launches=1)

# ---- band, whole tiles (TORBI_HIP_BAND_FORM=tile): run_band, bpw = ceil(64-state blocks / waves), waves 4 | 8 up to 4 | 8
# blocks, else 12 (TORBI_HIP_TILE_WAVES=8: 8); the twelve-wave instance for bpw 1 and for bpw 2 on twelve waves
for S, reach, BPW, NW, waves in ((256, (10, 3), 1, 12, None),          # 4 blocks on 4 waves
                                 (1440, (87, 87), 2, 12, None),        # 23 blocks on 12 waves
                                 (1024, (5, 60), 2, 8, '8'),           # 16 blocks on 8 waves
                                 (1440, (87, 87), 3, 8, '8')):         # 23 blocks on 8 waves
    for outside, BG in ((INF, 'false'), (-50.0, 'true')):
        env = {'TORBI_HIP_BAND_FORM': 'tile'}
        if waves:
            env['TORBI_HIP_TILE_WAVES'] = waves
        _add('band', f'band::band_tile_kernel<{BPW}, {NW}, {BG}>', 'band', 'band', S, ('items', 16), env=env,
             band=reach + (outside,), launches=1)
# ---- band, tiles split over members (TORBI_HIP_BAND_FORM=split): one tile in one launch; units // 8 + 8 tiles at 1440 states
# and reach 87 have 8 members each (the fewest the LDS allows), 8 * (units // 8 // 8) tiles per launch: two launches
for outside, BG in ((INF, 'false'), (-50.0, 'true')):
    for items, launches in ((('items', 16), 1), (('band', 8), 2)):
        _add('band', f'band::band_forward_kernel<{BG}>', 'band', 'band', 1440, items, env={'TORBI_HIP_BAND_FORM': 'split'},
             band=(87, 87, outside), launches=launches)

# ---- held: held_instance, one item, path 'held'.  K = ceil(S / 512) prev-states per thread with 8 rows per workgroup up to
# 2048 states, ceil(S / 1024) with 16 above.  Pinned by state count: the note names no instance (see `reported`).
for S, K in ((512, 1), (516, 2), (1024, 2), (1028, 3), (1536, 3), (1540, 4), (2048, 4)):
    _add('held', f'held::held_forward_kernel<{K}, 8, 512, true>', 'held', 'held', S, launches=1, reported=HELD_NOTE)
for S, K in ((2052, 3), (3072, 3), (4096, 4)):
    _add('held', f'held::held_forward_kernel<{K}, 16, 1024, false>', 'held', 'held', S, launches=1, reported=HELD_NOTE)

# the families of forward kernels the list of profiles/launch_sequence_ab.txt is compared on (the repair instances of the
# time-resident kernel end in `true>`)
FORWARD_FAMILIES = ('small::decode_kernel<', 'small::decode_value_kernel<', 'small::block_value_kernel<',
                    'dense::step_dense_kernel<', 'resident::resident_forward_kernel<', 'band::band_tile_kernel<',
                    'band::band_forward_kernel<', 'held::held_forward_kernel<')


def is_forward_instance(name):
    return name.startswith(FORWARD_FAMILIES) and not (name.startswith('resident::') and name.endswith(', true>'))
