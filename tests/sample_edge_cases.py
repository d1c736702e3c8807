"""Weight rows whose interval edges and zero runs the test decides, probe uniforms built from their float64 prefix sums, the
checker of a route's draws against them, and mutant pickers that stand for kernel bugs (SAMPLING.md, both accuracy sections).
Shared by tests/test_sample_edges_cpu.py and tests/test_sample_edges_gpu.py.

A *row* is one weight vector the test controls: frame 0 of an item whose later frame is steered (`inner`: obs[b, 1] is -inf
except at j*, so j_1 = j* for every uniform and w = a_0 * E[j*]), the only frame of an item with one frame (`last`: w = a_0), or
any frame of the uniform route (w = exp(x - max x)).  On the band route the row is the concatenated vector
[v[lo .. hi], ebg * a_0] and a *slot* of it belongs to a state.  Every draw n of an item carries one probe uniform for the row:
the values outside [0, 1) and NaN (`first`, `top`), the float32 neighbours of the edges between heavy states (`edge`) and of
the band's seam (`seam`), the midpoints of the heavy states (`mid`), and on rows of 2^k unit weights the uniforms whose target
lies exactly on an edge (`tie`).
"""
import functools
import math
from types import SimpleNamespace

import numpy as np
import torch

from torbi_amd import sampling

import sample_cases as sc
import sample_band_cases as sbc

BOUND = 1e-4                    # the project's bound on a normalised fp32 row against float64 (tests/test_sample_gpu.py)
HEAVY_SHARE = 1e-2              # a heavy state's share of Z: a neighbour taken by mistake costs d >= 1e-2, 100 x the bound
MAX_HEAVY = 24                  # heavy weights lie in [0.5, 2]: at most 24 of them keep every share >= 0.5 / 48 > 1e-2
FLOOR = 1e-30                   # every positive float64 weight is >= FLOOR * Z: no positive weight underflows in fp32
DUST = -60.                     # log of a dust weight against a heavy one: positive, absorbed by a float32 prefix
TINY = float(np.log(np.finfo(np.float32).tiny))

FIRST = (0., -0., -3., -math.inf, math.nan, 1e-45)          # all read as the first state of weight > 0
TOP = (1. - 2. ** -24, 1., 7., math.inf)                    # all read as 1 - 2^-24
KINDS = ('first', 'top', 'edge', 'mid', 'seam', 'pad', 'tie')
K_FIRST, K_TOP, K_EDGE, K_MID, K_SEAM, K_PAD, K_TIE = range(7)

# S -> the instance of sample_backward_kernel the launcher takes (NB = the smallest power of two >= blocks; a block is 256
# states with float4 loads, S % 4 == 0, and 64 with scalar ones); for the streamed form the registers of `Streamed` it fills
DENSE_SHAPES = {
    64: 'float4 NB=1', 512: 'float4 NB=2', 772: 'float4 NB=4', 1440: 'float4 NB=8 (two padding blocks)',
    4096: 'float4 NB=16', 4100: 'float4 streamed (17 blocks)',
    37: 'scalar NB=1', 127: 'scalar NB=2', 203: 'scalar NB=4', 257: 'scalar NB=8', 1023: 'scalar NB=16',
    2047: 'scalar NB=32', 2049: 'scalar streamed (33 blocks)', 4161: 'scalar streamed (66 blocks, g=1)',
    12353: 'scalar streamed (194 blocks, g=3)',
}
# where the patterns sit: the boundary between blocks at - 1 | at
DENSE_AT = {4161: (64,), 12353: (64, 128, 192)}
UNIFORM_SHAPES = {
    37: 'scalar held', 64: 'float4 held', 1440: 'float4 held', 2048: 'float4 held (last)', 2052: 'float4 streamed',
    2049: 'scalar streamed', 4161: 'scalar streamed g=1', 8257: 'scalar streamed g=2', 16383: 'scalar streamed g=3',
}
UNIFORM_AT = {4161: (1, 64), 8257: (64, 128), 16383: (64, 128, 192)}
# (S, (reach_left, reach_right), background)
BAND_SHAPES = [
    (64, (2, 5), -math.inf), (64, (5, 2), -4.), (128, (31, 32), -math.inf), (128, (31, 32), -3.), (37, (36, 36), -3.),
    (1441, (12, 12), -20.), (64, (2, 2), TINY),
]
LONG_FRAMES = (200, 129, 128, 65, 64, 63, 1)


def band_id(shape):
    S, band, bg = shape
    name = 'inf' if bg == -math.inf else 'tiny' if bg == TINY else f'{-bg:g}'
    return f'{S}_{band[0]}_{band[1]}_bg_{name}'


def geometry(S):
    """(states per lane, states per block) of a row of S states: float4 loads at S % 4 == 0."""
    return (4, 256) if S % 4 == 0 else (1, 64)


def patterns(S, at=(1,)):
    """[(name, heavy states, dust states)]: the sets of positive states of the issue, every other state exactly 0.  `at`:
    the block boundaries at - 1 | at the patterns sit at.  'random' has heavy = None: every state positive."""
    per, K = geometry(S)
    blocks = -(-S // K)
    out, seen = [], set()

    def add(name, heavy, dust=()):
        heavy = sorted({s for s in heavy if 0 <= s < S})
        dust = sorted({s for s in dust if 0 <= s < S} - set(heavy))
        key = (tuple(heavy), tuple(dust), name == 'ties')
        if heavy and key not in seen:
            assert len(heavy) <= MAX_HEAVY
            seen.add(key)
            out.append((name, heavy, dust))

    for k, qb in enumerate(at):
        tag = '' if qb == 1 else f'@{qb}'
        edge = qb * K
        bnd = [edge - 1, edge]
        for base in (edge - K, edge):
            bnd += [base + 3 * per - 1, base + 3 * per, base + 16 * per - 1, base + 16 * per]
        add('boundaries' + tag, bnd)
        first = edge + 1 if edge + 1 < S else 16 * per if 16 * per < S else per
        add('leading' + tag, [first, first + per, first + 5 * per + 1, S - 1])
        last = min(edge - 2, S - 2)
        add('trailing' + tag, [last - 7 * per - 1, last - per, last])
        if blocks - 1 >= qb + 1:
            add('hole' + tag, [edge - K + 1, edge - 1, (blocks - 1) * K, S - 1])
        for s in ((0, S - 1) if k == 0 else ()) + (edge - 1, edge):
            add(f'single_{s}', [s])
        if k == 0:
            if per == 4:                         # lane 5 of block 0 (states 20 .. 23) beside one state of lanes 3 and 9
                add('lane_v0', [14, 20, 37])
                add('lane_v3', [14, 23, 37])
                add('lane_v0_v3', [14, 20, 23, 37])
            heavy = [s for s in bnd if 0 <= s < S]
            add('dust' + tag, heavy, [0, S - 1] + [s + 1 for s in heavy])
            add('ties', _power_of_two(sorted(set(heavy))))
    out.append(('random', None, ()))
    return out


def _power_of_two(states):
    """The first 2^k of `states`, k as large as they allow."""
    return states[:1 << (len(states).bit_length() - 1)] if states else states


def _log_weights(S, heavy, dust, g, unit=False):
    """(S,) float64 log weights of a pattern: heavy ones drawn from [0.5, 2] (`unit`: all exactly 1), dust at exp(-60) of a
    heavy one, -inf else."""
    x = torch.full((S,), -math.inf, dtype=torch.float64)
    h = torch.log(0.5 + 1.5 * torch.rand(len(heavy), generator=g, dtype=torch.float64))
    if unit:
        h = torch.zeros_like(h)
    x[heavy] = h
    if len(dust):
        x[list(dust)] = h[torch.arange(len(dust)) % len(heavy)] + DUST
    return x


def _neighbours(x):
    """float32(x) and its two float32 neighbours on each side."""
    x = np.float32(x)
    out, lo, hi = [x], x, x
    for _ in range(2):
        lo, hi = np.nextafter(lo, np.float32(-np.inf)), np.nextafter(hi, np.float32(np.inf))
        out += [lo, hi]
    return [float(v) for v in sorted(out)]


def make_row(name, b, t, w, heavy, state=None, seam=None, band_top=None, jstar=None, ties=False):
    """The probes of one weight row w (C,) float64 with heavy slots `heavy`: `values` float32 uniforms, `kinds`, and `target`,
    the slot a probe must return exactly (-1: only validity and the bound are judged).  `state` (C,): the state of each slot."""
    C = w.shape[0]
    P = torch.cumsum(w, 0)
    Z = float(P[-1])
    positive = torch.nonzero(w > 0)[:, 0]
    share = w / Z
    heavy = sorted(int(s) for s in heavy)
    values = list(FIRST) + list(TOP)
    kinds = [K_FIRST] * len(FIRST) + [K_TOP] * len(TOP)
    last = int(positive[-1])
    target = [int(positive[0])] * len(FIRST) + [last if float(share[last]) >= HEAVY_SHARE else -1] * len(TOP)
    for upper in heavy[1:]:                      # the edge between two consecutive heavy slots (dust lies below it)
        near = _neighbours(float(P[upper - 1]) / Z)
        values += near
        kinds += [K_EDGE] * len(near)
        target += [-1] * len(near)
    for s in heavy:
        values.append(float(np.float32((float(P[s]) - 0.5 * float(w[s])) / Z)))
        kinds.append(K_MID)
        target.append(s)
    if ties:
        # n = 2^k weights of exactly 1: Z = n, u = i / n and the target i are exact in fp32 and in float64, in any summation
        # tree, and u Z lies ON the edge between two states; the rule's `>` takes the state behind the edge
        n = len(heavy)
        assert n >= 2 and n & (n - 1) == 0 and bool((w[heavy] == 1).all()) and Z == n
        for i in range(1, n):
            values.append(i / n)
            kinds.append(K_TIE)
            target.append(heavy[i])
    if seam is not None:
        near = _neighbours(seam / Z)
        values += near
        kinds += [K_SEAM] * len(near)
        target += [-1] * len(near)
    return SimpleNamespace(name=name, b=b, t=t, w=w, Z=Z, heavy=heavy, seam=seam, band_top=band_top, jstar=jstar,
                           state=torch.arange(C) if state is None else state, values=values, kinds=kinds, target=target)


def _finish(case, rows):
    """Pads every row's probes to the same count N with plain uniforms, lays them into case.u (B, N, T) and records the float64
    rule's own answer to every probe."""
    B, T = case.obs.shape[:2]
    N = max(len(r.values) for r in rows)
    g = torch.Generator().manual_seed(77)
    u = torch.rand((B, N, T), generator=g)
    for r in rows:
        n = len(r.values)
        u[r.b, :n, r.t] = torch.tensor(r.values, dtype=torch.float32)
        if case.route != 'uniform':              # the steered frame reads the probes too, one draw on
            u[r.b, :, 1] = torch.roll(u[r.b, :, 0], 1)
        r.kinds = torch.tensor(r.kinds + [K_PAD] * (N - n))
        r.target = torch.tensor(r.target + [-1] * (N - n))
        r.u = u[r.b, :, r.t].clone()
        slot, ok = sampling.draw(r.w[None].expand(N, -1), sampling.read_uniforms(r.u))
        assert bool(ok.all())
        r.host_slot = slot
        r.host = r.state[slot]
        r.expected = torch.where(r.target >= 0, r.state[r.target.clamp(0)], torch.full_like(r.target, -1))
    case.u, case.rows, case.N = u, rows, N
    return case


# ---------------------------------------------------------------------------------------------------------------------------
# dense route

@functools.lru_cache(maxsize=None)
def dense_case(S):
    """Items of T = 2 frames for forward_sample: every pattern as a last-frame item (frames = 1, w = a_0) and as an
    inner-frame item (w = a_0 * E[j*], zeros made in turn by a zero filter entry and by a zero matrix entry under a live
    one), each inner item with its own j* and so its own row of A.  Above 4200 states the two kinds take turns."""
    pats = patterns(S, DENSE_AT.get(S, (1,)))
    plan = [(p, kind) for k, p in enumerate(pats)
            for kind in (('last',) if p[0] == 'ties' else ('last', 'inner') if S <= 4200 else (('last', 'inner')[k % 2],))]
    B, T = len(plan), 2
    obs, A, pi = sc.problem(B, T, S, seed=S)
    g = torch.Generator().manual_seed(S)
    jstars = torch.randperm(S, generator=g)[:B].tolist()
    frames = torch.tensor([1 if kind == 'last' else 2 for _, kind in plan], dtype=torch.int32)
    pi64 = pi.double()
    for b, ((name, heavy, dust), kind) in enumerate(plan):
        j = jstars[b]
        if kind == 'inner':
            obs[b, 1] = -math.inf
            obs[b, 1, j] = 0.
        if heavy is None:
            continue
        x = _log_weights(S, heavy, dust, g, unit=name == 'ties')
        if kind == 'last':
            obs[b, 0] = (x - pi64).float()
        else:
            dead = torch.nonzero(x == -math.inf)[:, 0]
            by_matrix = dead[1::2]                                   # a zero matrix entry under a filter entry of weight 1
            alive = torch.nonzero(x > -math.inf)[:, 0]
            x[by_matrix] = 0.
            o = x - pi64
            o[alive] -= A[j, alive].double()
            obs[b, 0] = o.float()
            A[j, by_matrix] = -math.inf
    case = SimpleNamespace(route='dense', S=S, obs=obs, frames=frames, A=A, pi=pi, band=None, bg=None)
    a, E, L, F = sampling._filter(obs, frames, A, None, pi)
    case.ref = (a, E, L, F)
    rows = []
    for b, ((name, heavy, dust), kind) in enumerate(plan):
        w = a[b, 0] if kind == 'last' else a[b, 0] * E[jstars[b]]
        rows.append(make_row(f'{name}/{kind}', b, 0, w.clone(), heavy or [], jstar=jstars[b] if kind == 'inner' else None,
                             ties=name == 'ties'))
    return _finish(case, rows)


# ---------------------------------------------------------------------------------------------------------------------------
# uniform route

@functools.lru_cache(maxsize=None)
def uniform_case(S):
    """Items of T = 4 independent frames for the uniform route, one pattern per frame; frame 0 has pi added, and pi holds one
    -inf at a state the frame-0 patterns would otherwise keep alive."""
    pats = patterns(S, UNIFORM_AT.get(S, (1,)))
    T = 4
    B = -(-len(pats) // T)
    obs, _, pi = sc.problem(B, T, S, seed=S + 1)
    g = torch.Generator().manual_seed(S + 1)
    dead_pi = 3 * geometry(S)[0]                 # the upper side of the lane boundary of `boundaries`
    pi[dead_pi] = -math.inf
    spec = {}
    for k, (name, heavy, dust) in enumerate(pats):
        b, t = divmod(k, T)
        if heavy is not None:
            if t == 0:                           # pi's -inf takes its state out of the pattern, under a live observation
                heavy, dust = [s for s in heavy if s != dead_pi], [s for s in dust if s != dead_pi]
                heavy = _power_of_two(heavy) if name == 'ties' else heavy
            x = _log_weights(S, heavy, dust, g, unit=name == 'ties')
            if t == 0:
                x = x - torch.where(torch.isinf(pi), torch.zeros_like(pi), pi).double()
                x[dead_pi] = 0.
            obs[b, t] = x.float()
        spec[(b, t)] = (name, heavy)
    frames = torch.full((B,), T, dtype=torch.int32)
    case = SimpleNamespace(route='uniform', S=S, obs=obs, frames=frames, A=None, pi=pi, band=None, bg=None)
    uniform = float(torch.tensor(math.log(1. / S), dtype=torch.float32))
    a, E, L, F = sampling._filter(obs, frames, None, uniform, pi)
    case.ref = (a, None, L, F)
    rows = []
    for b in range(B):
        for t in range(T):
            name, heavy = spec.get((b, t), ('random', None))
            w = a[b, t].clone()
            rows.append(make_row(f'{name}/frame{t}', b, t, w, heavy or [], ties=name == 'ties'))
    return _finish(case, rows)


# ---------------------------------------------------------------------------------------------------------------------------
# band route

def _band_slots(Wc):
    """Patterns over the Wc slots of a clipped band window (lane k of the wave owns slot k)."""
    out = [('boundaries', [k for k in (2, 3, 15, 16, 31, 32, 47, 48, Wc - 1) if k < Wc])]
    first = 17 if Wc > 19 else 1
    out.append(('leading', [k for k in (first, first + 2, Wc - 1) if k < Wc]))
    out.append(('trailing', sorted({0, max(0, Wc - 5), max(0, Wc - 2)})))
    out.append(('single_first', [0]))
    out.append(('single_last', [Wc - 1]))
    return out


@functools.lru_cache(maxsize=None)
def band_case(S, band, bg):
    """Items of T = 2 frames for forward_sample_banded.  Inner-frame items: j* near 0, near S - 1 and in the middle, a
    pattern over the window's slots (v = a_0 * (E[j*] - ebg) is the heavy weight) and, with a finite background, one over the
    states outside the window (a_0 is the heavy weight, so the whole-row part is ebg * a_0); once the band part is all 0.
    Zeros: obs = -inf, and with -inf outside the band in turn A[j*][i] = -inf.  Last-frame items: the patterns on a_0."""
    left, right = min(band[0], S - 1), min(band[1], S - 1)
    ebg = sbc.ebg_of(bg)
    finite = bg != -math.inf
    row_pats = [p for p in patterns(S) if p[1] is not None and not p[0].startswith(('single', 'lane', 'dust', 'ties'))]
    plan = []                                    # (name, j* or None, slot pattern or None, row pattern or None)
    for where in range(3):
        slot_pats = None
        for p in range(6 if finite and bg != TINY else 5):
            j = (p, S - 1 - p, S // 2 + p)[where]
            lo, hi = max(0, j - left), min(S - 1, j + right)
            slot_pats = _band_slots(hi - lo + 1) + [('empty', [])]
            sname, slots = slot_pats[p]
            rname, rheavy, _ = row_pats[(p + where) % len(row_pats)]
            if not slots and hi - lo + 1 == S:   # (the window is the whole row: nothing is left behind an empty band)
                continue
            plan.append((f'{sname}+{rname}/inner{j}', j, [lo + k for k in slots], rheavy if finite else None))
    for name, heavy, dust in patterns(S):
        plan.append((f'{name}/last', None, None, (heavy, dust)))
    B, T = len(plan), 2
    obs, A, pi = sbc.problem(B, T, S, seed=S + left, band=band, background=bg)
    g = torch.Generator().manual_seed(S + left)
    frames = torch.tensor([1 if j is None else 2 for _, j, _, _ in plan], dtype=torch.int32)
    pi64 = pi.double()
    for b, (name, j, inband, rest) in enumerate(plan):
        if j is None:
            heavy, dust = rest
            if heavy is not None:
                obs[b, 0] = (_log_weights(S, heavy, dust, g, unit=name == 'ties/last') - pi64).float()
            continue
        obs[b, 1] = -math.inf
        obs[b, 1, j] = 0.
        lo, hi = max(0, j - left), min(S - 1, j + right)
        window = torch.arange(lo, hi + 1)
        if rest is None:                         # -inf outside the band: the states out of the window carry no weight
            x = obs[b, 0].double() + pi64
        else:
            outside = [s for s in rest if s < lo or s > hi] or [s for s in (lo - 2, hi + 2) if 0 <= s < S]
            x = _log_weights(S, outside, (), g) if outside else torch.full((S,), -math.inf, dtype=torch.float64)
        x[window] = -math.inf
        if inband:
            x[inband] = _log_weights(S, inband, (), g)[inband] - torch.log(torch.exp(A[j, inband].double()) - ebg)
        if not finite:
            dead = window[torch.isinf(x[window])][1::2]
            x[dead] = 0.
            A[j, dead] = -math.inf
        obs[b, 0] = (x - pi64).float()
    case = SimpleNamespace(route='band', S=S, obs=obs, frames=frames, A=A, pi=pi, band=band, bg=bg)
    a, E, L, F = sampling._filter(obs, frames, A, None, pi)
    case.ref = (a, E, L, F)
    rows = []
    for b, (name, j, inband, rest) in enumerate(plan):
        if j is None:
            w = a[b, 0].clone()
            heavy = [] if rest[0] is None else rest[0]
            rows.append(make_row(name, b, 0, w, heavy, ties=name == 'ties/last'))
            continue
        lo, hi = max(0, j - left), min(S - 1, j + right)
        window = torch.arange(lo, hi + 1)
        v = a[b, 0, window] * (E[j, window] - ebg).clamp_min(0.)
        w = torch.cat([v, ebg * a[b, 0]])
        state = torch.cat([window, torch.arange(S)])
        heavy = torch.nonzero(w / w.sum() >= HEAVY_SHARE)[:, 0].tolist()
        Zband = float(v.sum())
        seam = Zband if finite and bg != TINY and Zband > 0 else None
        rows.append(make_row(name, b, 0, w, heavy[:MAX_HEAVY], state=state, seam=seam,
                             band_top=window if bg in (-math.inf, TINY) else None, jstar=j))
        rows[-1].slots = len(window)
    return _finish(case, rows)


# ---------------------------------------------------------------------------------------------------------------------------
# long sequences

@functools.lru_cache(maxsize=None)
def long_case(route, S, band=None, bg=None, B=7, T=200, frames=LONG_FRAMES):
    """Random inputs, N = 5 draws (a workgroup of four and a tail), ragged lengths around the 64-frame runs of `IndexRun`."""
    if route == 'band':
        obs, A, pi = sbc.problem(B, T, S, seed=S + T, band=band, background=bg)
    else:
        obs, A, pi = sc.problem(B, T, S, seed=S + T)
    fr = torch.tensor(frames, dtype=torch.int32)
    case = SimpleNamespace(route=route, S=S, obs=obs, frames=fr, A=None if route == 'uniform' else A, pi=pi, band=band, bg=bg,
                           rows=[], N=5, u=sc.uniforms(B, 5, T, seed=S + T))
    uniform = float(torch.tensor(math.log(1. / S), dtype=torch.float32)) if route == 'uniform' else None
    a, E, L, F = sampling._filter(obs, fr, case.A, uniform, pi)
    case.ref = (a, E, L, F)
    return case


def host(case):
    """The float64 host route on the whole case: (indices int64, L float64)."""
    if case.route == 'band':
        return sbc.host(case.obs, case.frames, case.A, case.pi, case.u, case.band, case.bg)
    return sc.host(case.obs, case.frames, case.A, case.pi, case.u)


# ---------------------------------------------------------------------------------------------------------------------------
# the checker

def judge(case, indices):
    """What the draws `indices` (B, N, T) of a route break: SimpleNamespace(failures [str], worst d, flips = how many `edge`
    and `seam` probes chose another state than the float64 rule, edges = how many there are)."""
    a, E, _, F = case.ref
    S = case.S
    j = indices.to(torch.int64)
    fails = []
    B, N, T = j.shape
    live = (torch.arange(T)[None, None, :] < F[:, None, None]).expand_as(j)
    if not bool(((j >= 0) & (j < S))[live].all()):
        fails.append(f'an index outside [0, {S})')
        return SimpleNamespace(failures=fails, worst=math.inf, flips=0, edges=0)
    flips = edges = 0
    for r in case.rows:
        got = j[r.b, :, r.t]
        if r.jstar is not None and not bool((j[r.b, :, 1] == r.jstar).all()):
            fails.append(f'{r.name}: j_1 is not the steered state {r.jstar}')
            continue
        per_state = torch.zeros(S, dtype=torch.float64).index_add_(0, r.state, r.w)
        for n in torch.nonzero(per_state[got] <= 0)[:, 0].tolist():
            fails.append(f'{r.name}: {KINDS[int(r.kinds[n])]} probe u = {float(r.u[n])!r} returned state {int(got[n])} of weight 0')
        wrong = (r.target >= 0) & (got != r.expected)
        for n in torch.nonzero(wrong)[:, 0].tolist():
            fails.append(f'{r.name}: {KINDS[int(r.kinds[n])]} probe u = {float(r.u[n])!r} returned state {int(got[n])}, '
                         f'expected {int(r.expected[n])}')
        for kind in (K_FIRST, K_TOP):
            group = got[r.kinds == kind]
            if not bool((group == group[0]).all()):
                fails.append(f'{r.name}: the {KINDS[kind]} probes disagree: {group.tolist()}')
        if r.band_top is not None:               # -inf or log(tiny) outside the band: the top of the row is a band slot > 0
            n_slots = r.slots
            for s in got[r.kinds == K_TOP].tolist():
                at = torch.nonzero(r.state[:n_slots] == s)[:, 0]
                if len(at) == 0 or not float(r.w[int(at[0])]) > 0:
                    fails.append(f'{r.name}: a top probe returned state {s}, which has no band slot of weight > 0')
        near = (r.kinds == K_EDGE) | (r.kinds == K_SEAM)
        edges += int(near.sum())
        flips += int((got != r.host)[near].sum())
    worst = 0.
    for b in range(B):                           # (item by item: the float64 weights of all draws of one item at a time)
        one = slice(b, b + 1)
        if case.route == 'band':
            d = sbc.draw_errors(j[one], case.u[one], a[one], E, F[one], case.band, case.bg)[0]
        else:
            d, positive = sc.draw_errors(j[one], case.u[one], a[one], E, F[one])
            if not positive:
                fails.append(f'item {b}: a chosen state has float64 weight 0')
        if not d <= BOUND:
            fails.append(f'item {b}: d = {d:.3g} > {BOUND}')
        worst = max(worst, d)
    if not sc.tails_repeat(j, F):
        fails.append('a tail column does not repeat j_{F-1}')
    return SimpleNamespace(failures=fails, worst=worst, flips=flips, edges=edges)


def conditions(case):
    """What the construction promises, on the float64 weights: [str] of what does not hold.  Every heavy state's share of Z
    is >= HEAVY_SHARE (band route: heavy slots are chosen by it), every positive weight is >= FLOOR * Z (the whole-row part
    of a log(tiny) background aside: it lies below fp32 by design), L is finite."""
    fails = []
    if not bool(torch.isfinite(case.ref[2]).all()):
        fails.append('L is not finite')
    for r in case.rows:
        if not (r.Z > 0 and math.isfinite(r.Z)):
            fails.append(f'{r.name}: Z = {r.Z}')
            continue
        share = r.w / r.Z
        if r.heavy and float(share[r.heavy].min()) < HEAVY_SHARE:
            fails.append(f'{r.name}: a heavy share of {float(share[r.heavy].min()):.3g}')
        part = share[:r.slots] if case.route == 'band' and case.bg == TINY and r.jstar is not None else share
        if bool(((part > 0) & (part < FLOOR)).any()):
            fails.append(f'{r.name}: a positive weight below {FLOOR} Z')
    return fails


def with_picker(case, picker):
    """The (B, N, T) indices a route would return if it drew every controlled row of a dense case with `picker(w, u)`."""
    B, T = case.obs.shape[:2]
    out = torch.zeros((B, case.N, T), dtype=torch.int64)
    for r in case.rows:
        w = r.w.numpy()
        col = torch.tensor([picker(w, float(x)) for x in r.u])
        out[r.b, :, 0] = col
        out[r.b, :, 1] = col if r.jstar is None else r.jstar
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# pickers (w64, u) -> state: the rule, and mutants that stand for kernel bugs

def _read(u, nan_as_zero=True, clamp_top=True):
    if math.isnan(u):
        return 0. if nan_as_zero else u
    u = max(float(np.float32(u)), 0.)
    return min(u, 1. - 2. ** -24) if clamp_top else u


def _first_or(mask, fallback):
    at = np.nonzero(mask)[0]
    return int(at[0]) if len(at) else int(fallback)


def pick_rule(w, u):
    P = np.cumsum(w)
    alive = np.nonzero(w > 0)[0]
    return _first_or((w > 0) & (P > _read(u) * P[-1]), alive[-1])


def mutant_ge_without_weight_test(w, u):
    """`>=` for `>` in the ballot and no `w > 0` test: state 0 of a zero run at u = 0."""
    P = np.cumsum(w)
    return _first_or(P >= _read(u) * P[-1], len(w) - 1)


def mutant_ge_with_weight_test(w, u):
    """`>=` for `>` with the weight test kept: wrong only where u Z lies exactly on an edge."""
    P = np.cumsum(w)
    alive = np.nonzero(w > 0)[0]
    return _first_or((w > 0) & (P >= _read(u) * P[-1]), alive[-1])


def mutant_nan_not_zero(w, u):
    """NaN is not read as 0: every comparison fails and the fallback takes the last state of weight > 0."""
    P = np.cumsum(w)
    alive = np.nonzero(w > 0)[0]
    with np.errstate(invalid='ignore'):
        return _first_or((w > 0) & (P > _read(u, nan_as_zero=False) * P[-1]), alive[-1])


def mutant_no_upper_clamp(w, u):
    """No clamp to 1 - 2^-24, and a fallback to state S - 1 instead of the last state of weight > 0."""
    P = np.cumsum(w)
    with np.errstate(invalid='ignore', over='ignore'):
        return _first_or((w > 0) & (P > _read(u, clamp_top=False) * P[-1]), len(w) - 1)


def mutant_block_by_total_before(w, u):
    """The block search compares the cumulative total BEFORE a block with the target, zero blocks included: a target inside
    block 0 lands in the block behind it, and the block's first state is returned where it holds no weight."""
    K = geometry(len(w))[1]
    P = np.cumsum(w)
    target = _read(u) * P[-1]
    blocks = -(-len(w) // K)
    before = np.array([P[q * K - 1] if q else 0. for q in range(blocks)])
    q = _first_or(before >= target, blocks - 1)
    lo, hi = q * K, min(len(w), (q + 1) * K)
    return lo + _first_or((w[lo:hi] > 0) & (P[lo:hi] > target), 0)


def mutant_lane_first_state(w, u):
    """The lane is found, but its first state is returned instead of the search among the lane's four values."""
    per = geometry(len(w))[0]
    return pick_rule(w, u) // per * per


def mutant_off_by_one(w, u):
    """The state behind the right one."""
    return min(pick_rule(w, u) + 1, len(w) - 1)


MUTANTS = {
    # name -> (picker, the pattern and probe kind it must break)
    'ge_without_weight_test': (mutant_ge_without_weight_test, 'leading', 'first'),
    'ge_with_weight_test': (mutant_ge_with_weight_test, 'ties', 'tie'),
    'nan_not_zero': (mutant_nan_not_zero, 'boundaries', 'first'),
    'no_upper_clamp': (mutant_no_upper_clamp, 'trailing', 'top'),
    'block_by_total_before': (mutant_block_by_total_before, 'hole', 'mid'),
    'lane_first_state': (mutant_lane_first_state, 'lane_v3', 'mid'),
    'off_by_one': (mutant_off_by_one, 'boundaries', 'mid'),
}
