"""What a caller who owns the workspace may rely on, for every route but decode (tests/test_workspace_bounds_gpu.py has
decode): posteriors, counts, k-best, sampling, their uniform and band routes, and the streaming state.

Such a caller hands the library memory that is pooled, cut out of a larger buffer at any offset, and full of what the last
call left there.  Every case below is one row of a route's smallest shapes that reach each branch of its layout, and is put
through four properties, each against the reference and at the tolerance of the route's own test file:

    (a) exactly the bytes the size query names, at a 256-byte aligned base and at base + 1 (after the layouts' round-up by 255
        the last region then ends on the caller's last byte): the result is right and the 65536 bytes on either side of the
        workspace are untouched
    (b) a workspace full of 0x00 and one full of 0xFF (NaN as a float, -1 as an int) give the same bits
    (c) after calls that raise every flag the route keeps on the device -- an item with a NaN inside its frames, an initial
        distribution of -inf, a +inf in the matrix, an entry just outside the stated band -- a clean call in the SAME workspace
        gives the bits it gives in a fresh one, and so does a smaller clean problem (fewer items and frames, another padding)
    (d) one byte less than the size query names raises before anything is launched

(b) and (c) stand on what each route's own tests assert: identical calls give identical bits.
"""
import functools
import math
import types

import numpy as np
import pytest
import torch

import torbi_amd
from torbi_amd import _lib, inputs, posterior, sampling, synth
from torbi_amd.stream import INITIAL_CAPACITY, StreamDecoder

import k_best_band_cases as kbc
import sample_band_cases as sbc
import sample_cases as sc
import stream_band_cases as stbc
import stream_cases
import stream_lag_cases
import test_counts_band_gpu as counts_band_cases
import test_counts_gpu as counts_cases
import test_k_best_band_gpu as k_best_band_tests
import test_k_best_gpu as k_best_cases
import test_posterior_band_gpu as band_cases
import test_posterior_gpu as posterior_cases
import test_sample_band_gpu as sample_band_tests
import test_sample_gpu as sample_tests
from workspace_cases import DEV, assert_guards_intact, assert_same_bits, bits, guarded, ragged, smaller

pytestmark = pytest.mark.gpu

NINF = -math.inf
K = 3               # ranks of the k-best cases
DRAWS = 5           # draws per item of the sampling cases


def units():
    return int(_lib.load().torbi_hip_compute_units(0))


def dev(*arrays):
    return [torch.from_numpy(np.array(a)).to(DEV) for a in arrays]


def f64(*tensors):
    return tuple(t.cpu().numpy().astype(np.float64) for t in tensors)


def band_items(B):
    """Items per workgroup of the band kernels of posteriors, counts and sampling: 8, halved while there are fewer workgroups
    than compute units (the rows of 8 items of these cases' state counts fit the LDS)."""
    G = 8
    while G > 1 and -(-B // G) < units():
        G //= 2
    return G


# ------------------------------------------------------------------------------------------------ inputs that raise flags
def dirty_numpy(obs, frames, trans, init, band=None):
    """The calls that go in front of a clean one in property (c), all of defined behaviour (each route's tests of non-finite
    inputs and of a broken promise use them): item 0, which has every frame, reads a NaN; every item starts from -inf; the
    matrix holds a +inf (on the diagonal: inside every band); one entry just right of the stated band differs from the
    background."""
    T, S = obs.shape[1], obs.shape[2]
    nan_item = np.array(obs)
    nan_item[0, min(1, T - 1), 5 % S] = np.nan
    out = [(nan_item, frames, trans, init), (obs, frames, trans, np.full_like(np.array(init), -np.inf))]
    if trans is not None:
        bad = np.array(trans)
        bad[4, 4] = np.inf
        out.append((obs, frames, bad, init))
    if band is not None:
        stray = np.array(trans)
        stray[20, 20 + band[1] + 1] = -1.5
        out.append((obs, frames, stray, init))
    return out


def dirty_torch(obs, frames, A, pi, u, band=None):
    numpy = dirty_numpy(obs.numpy(), frames, None if A is None else A.numpy(), pi.numpy(), band)
    return [(torch.from_numpy(o), f, None if a is None else torch.from_numpy(a), torch.from_numpy(np.array(p)), u)
            for o, f, a, p in numpy]


# ------------------------------------------------------------------------------------------------ the routes
# A case: need (the size query's answer), clean (its inputs), run(inputs, workspace) -> the outputs on the device,
# check(outputs) against the route's reference for the clean inputs, dirty (inputs of the same shape that raise flags),
# route() asserting the branch the case is about, small() -> the case of the smaller problem (need, clean, run).

def posterior_case(B, T, S, uniform=False, small=True):
    """forward_backward as test_workspace_bounds_gpu.py calls it (the model and the observation prepared as state_posteriors
    prepares them), or with `uniform` the uniform route as state_posteriors(transition=None) reaches it."""
    obs, trans, init = synth.problem(B, T, S, seed=B + T + S)
    trans = None if uniform else trans
    frames = ragged(B, T, seed=S)

    def run(x, ws):
        o, f, a, p = x
        transition, value, initial = inputs.model(None if a is None else torch.as_tensor(a), torch.as_tensor(np.array(p)), True, S, DEV)
        o = inputs.observation(torch.as_tensor(np.array(o)), True, DEV)
        if a is None:
            return posterior._run(o, torch.as_tensor(f).to(DEV), None, value, initial, ws)
        return torbi_amd.forward_backward(o, torch.as_tensor(f).to(DEV), transition, initial, workspace=ws)

    def check(out):
        posterior_cases.check(f64(*out), posterior_reference(B, T, S, uniform), frames)

    def route():
        matrix = None if uniform else torch.as_tensor(trans)
        assert torbi_amd.posterior_route(matrix, B, T, S, gpu=0, log_probs=True) == ('uniform' if uniform else 'dense')
        if uniform:
            return
        tiles = -(-S // 32) * -(-B // 32)               # the step kernels stage their operands from two tiles per unit on
        assert (tiles >= 2 * units()) == (B > 32), (tiles, units())
        if B > 32:
            assert -(-S // 32) * (B // 32 - 1) < 2 * units()        # ... and B is the smallest multiple of 32 that does

    return types.SimpleNamespace(
        need=torbi_amd.forward_backward_workspace_bytes(B, T, S), clean=(obs, frames, trans, init), run=run, check=check,
        dirty=dirty_numpy(obs, frames, trans, init), route=route,
        small=(lambda: posterior_case(*smaller(B, T, S), uniform=uniform, small=False)) if small else None)


@functools.lru_cache(maxsize=None)
def posterior_reference(B, T, S, uniform):
    obs, trans, init = synth.problem(B, T, S, seed=B + T + S)
    return posterior_cases.host(obs, ragged(B, T, seed=S), None if uniform else trans, init)


def counts_case(B, T, S, small=True):
    obs, trans, init = synth.problem(B, T, S, seed=B + T + S)
    frames = ragged(B, T, seed=S)

    def run(x, ws):
        return torbi_amd.forward_backward_counts(*dev(*x), workspace=ws)

    def check(out):
        post, L, X, I = (t.to(DEV) for t in out)
        rX, rI = counts_reference(B, T, S)
        counts_cases.check_counts(X, I, rX, rI, frames, T)
        post2, L2 = torbi_amd.forward_backward(*dev(obs, frames, trans, init))      # (the dense route's, bit for bit)
        assert torch.equal(post, post2) and torch.equal(L, L2)
        posterior_cases.check(f64(post, L), counts_posterior_reference(B, T, S), frames)

    def route():
        assert torbi_amd.counts_route(torch.as_tensor(trans), B, T, S, gpu=0, log_probs=True) == 'dense'
        assert (-(-S // 32) * -(-B // 32) >= 2 * units()) == (B > 32)

    return types.SimpleNamespace(
        need=torbi_amd.training.expected_counts_workspace_bytes(B, T, S), clean=(obs, frames, trans, init), run=run,
        check=check, dirty=dirty_numpy(obs, frames, trans, init), route=route,
        small=(lambda: counts_case(*smaller(B, T, S), small=False)) if small else None)


@functools.lru_cache(maxsize=None)
def _counts_host(B, T, S):
    obs, trans, init = synth.problem(B, T, S, seed=B + T + S)
    gamma, L, X, I = torbi_amd.training._host_counts(torch.as_tensor(obs), torch.as_tensor(ragged(B, T, seed=S)),
                                                     torch.as_tensor(trans), torch.as_tensor(init), None)
    return gamma.numpy(), L.numpy(), X.numpy(), I.numpy()


def counts_reference(B, T, S):
    """test_counts_gpu.host's X and I (the float64 route on the log inputs as they are)."""
    return _counts_host(B, T, S)[2:]


def counts_posterior_reference(B, T, S):
    return _counts_host(B, T, S)[:2]


def staged_batch(S):
    """The smallest multiple of 32 items at which forward_backward stages its step kernels at S states."""
    return 32 * -(-2 * units() // -(-S // 32))


def band_case(B, T, S, left, right, background, G, small=True):
    key = (B, T, S, left, right, background)
    obs, frames, trans, init = band_cases.problem(*key)

    def run(x, ws):
        o, f, a, p = x
        o = inputs.observation(torch.from_numpy(np.array(o)), True, DEV)            # (as test_posterior_band_gpu.banded)
        return torbi_amd.forward_backward_banded(o, *dev(f, a, p), left, right, background, workspace=ws)

    def check(out):
        band_cases.check(f64(*out), band_cases.reference(*key), frames)

    def route():
        assert posterior._covered(B, T, S, left, right, background)
        assert band_items(B) == G and (G == 1 or B % G != 0)           # (a partial last tile)

    return types.SimpleNamespace(
        need=torbi_amd.forward_backward_banded_workspace_bytes(B, T, S, left, right), clean=(obs, frames, trans, init), run=run,
        check=check, dirty=dirty_numpy(obs, frames, trans, init, (left, right)), route=route,
        small=(lambda: band_case(*smaller(B, T, S), left, right, background, 1, small=False)) if small else None)


def counts_band_case(B, T, S, left, right, background, G, small=True):
    key = (B, T, S, left, right, background)
    obs, frames, trans, init = counts_band_cases.problem(*key)

    def run(x, ws):
        return counts_band_cases.device(*x, left, right, background, workspace=ws)

    def check(out):
        post, L, X, I = (t.to(DEV) for t in out)
        rX, rI, rL = counts_band_cases.reference(*key)
        assert np.isfinite(rL).all()
        counts_band_cases.check_counts(X, I, rX, rI, frames, T, 'x'.join(str(v) for v in key))
        post2, L2 = torbi_amd.forward_backward_banded(*dev(obs, frames, trans, init), left, right, background)
        assert torch.equal(post, post2) and torch.equal(L, L2)      # (forward_backward_banded's, bit for bit)

    def route():
        assert posterior._counts_covered(B, T, S, left, right, background)
        assert band_items(B) == G and (G == 1 or B % G != 0)
        # one plane per workgroup, at most 512: 4100 items are 513 tiles, so a workgroup goes round its loop twice
        assert (-(-B // G) > 512) == (B == 4100)

    return types.SimpleNamespace(
        need=torbi_amd.training.expected_counts_banded_workspace_bytes(B, T, S, left, right), clean=(obs, frames, trans, init),
        run=run, check=check, dirty=dirty_numpy(obs, frames, trans, init, (left, right)), route=route,
        small=(lambda: counts_band_case(*smaller(B, T, S), left, right, background, 1, small=False)) if small else None)


def k_best_case(B, T, S, uniform=False, small=True):
    obs, trans, init = synth.problem(B, T, S, seed=B + T + S + K)
    trans = None if uniform else trans
    frames = ragged(B, T, seed=S + K)

    def run(x, ws):
        return k_best_cases.device(*x, K, workspace=ws)

    def check(out):
        k_best_cases.same(out, k_best_cases.host(obs, frames, trans, init, K))

    def route():
        matrix = None if uniform else torch.as_tensor(trans)
        assert torbi_amd.k_best_route(matrix, B, T, S, K, gpu=0, log_probs=True) == ('uniform' if uniform else 'dense')
        assert frames[0] == T and frames[B - 1] == 1

    return types.SimpleNamespace(
        need=torbi_amd.decode_k_best_workspace_bytes(B, T, S, K, uniform=uniform), clean=(obs, frames, trans, init), run=run,
        check=check, dirty=dirty_numpy(obs, frames, trans, init), route=route,
        small=(lambda: k_best_case(*smaller(B, T, S), uniform=uniform, small=False)) if small else None)


def k_best_band_case(B, T, S, left, right, background, small=True):
    obs, trans, init = kbc.model(B, T, S, B + T + S, (left, right), background)
    frames = ragged(B, T, seed=S)

    def run(x, ws):
        i, s = torbi_amd.decode_k_best_banded(*dev(*x), K, left, right, background, workspace=ws)
        return i.cpu().numpy(), s.cpu().numpy()

    def check(out):
        k_best_band_tests.same(out, k_best_band_tests.host(obs, frames, trans, init, K))

    def route():
        assert kbc.covered(S, K, left, right, background) and torbi_amd.k_best._covered(B, T, S, K, left, right, background)
        assert kbc.instance(B, S, K, left, right) == (4, 1)
        if background == NINF:                                   # (what 'auto' finds in this matrix and where it sends it)
            A = torch.as_tensor(trans).to(DEV)
            assert torbi_amd.viterbi.band_over(A, A, S) == (left, right, background)
            assert torbi_amd.k_best_route(A, B, T, S, K, gpu=0, log_probs=True) == 'band'

    return types.SimpleNamespace(
        need=torbi_amd.decode_k_best_banded_workspace_bytes(B, T, S, K, left, right), clean=(obs, frames, trans, init), run=run,
        check=check, dirty=dirty_numpy(obs, frames, trans, init, (left, right)), route=route,
        small=(lambda: k_best_band_case(*smaller(B, T, S), left, right, background, small=False)) if small else None)


def sample_case(B, T, S, uniform=False, small=True):
    obs, A, pi = sc.problem(B, T, S, B + T + S)
    A = None if uniform else A
    frames = torch.from_numpy(ragged(B, T, seed=S))
    u = sc.uniforms(B, DRAWS, T, B + T + S)

    def run(x, ws):
        o, f, a, p, v = x
        if a is None:                                            # (as test_sample_gpu.run: the value sample_paths passes)
            value = float(torch.tensor(math.log(1. / S), dtype=torch.float32))
            return sampling._run(o.to(DEV).contiguous(), f.to(DEV), None, value, p.to(DEV), v.to(DEV), ws)
        return torbi_amd.forward_sample(o.to(DEV), f.to(DEV), a.to(DEV), p.to(DEV), v.to(DEV), ws)

    def check(out):
        indices, L = out[0].cpu(), out[1].cpu()
        ref = sample_reference(B, T, S, uniform)
        L64, F = sample_tests.check_draws(f'{B} x {T} x {S}', indices, L, u, ref, S)
        if uniform:
            err = torch.abs(L.double() - L64)
            assert bool((err <= 1e-6 * torch.abs(L64) + 4e-6 * F).all()), (err, L64)
        else:                                                    # L: the bits of forward_backward
            assert torch.equal(L, torbi_amd.forward_backward(obs.to(DEV), frames.to(DEV), A.to(DEV), pi.to(DEV))[1].cpu())

    def route():
        matrix = None if uniform else A.clone()      # (what a look remembers hangs off the tensor it was given: a temporary)
        assert torbi_amd.sample_route(matrix, B, T, S, draws=DRAWS, gpu=0, log_probs=True) == ('uniform' if uniform else 'dense')
        assert int(frames[0]) == T and int(frames[B - 1]) == 1

    return types.SimpleNamespace(
        need=torbi_amd.forward_sample_workspace_bytes(B, T, S, DRAWS, uniform=uniform), clean=(obs, frames, A, pi, u), run=run,
        check=check, dirty=dirty_torch(obs, frames, A, pi, u), route=route,
        small=(lambda: sample_case(*smaller(B, T, S), uniform=uniform, small=False)) if small else None)


@functools.lru_cache(maxsize=None)
def sample_reference(B, T, S, uniform):
    obs, A, pi = sc.problem(B, T, S, B + T + S)
    return sc.reference(obs, torch.from_numpy(ragged(B, T, seed=S)), None if uniform else A, pi)


def sample_band_case(B, T, S, left, right, background, small=True):
    band = (left, right)
    obs, A, pi = sbc.problem(B, T, S, B + T + S, band, background)
    frames = torch.from_numpy(ragged(B, T, seed=S))
    u = sc.uniforms(B, DRAWS, T, B + T + S)

    def run(x, ws):
        o, f, a, p, v = x
        return torbi_amd.forward_sample_banded(o.to(DEV), f.to(DEV), a.to(DEV), p.to(DEV), v.to(DEV), left, right, background, ws)

    def check(out):
        indices, L = out[0].cpu(), out[1].cpu()
        ref = torbi_amd.sampling._filter(obs, frames, A, None, pi)
        sample_band_tests.check_draws(f'{B} x {T} x {S}, {left}/{right}, {background}', indices, u, ref, band, background)
        assert torch.equal(L, sample_band_tests.band_L(obs, frames, A, pi, band, background))

    def route():
        assert sampling._covered(B, T, S, DRAWS, left, right, background) and band_items(B) == 1

    return types.SimpleNamespace(
        need=torbi_amd.forward_sample_banded_workspace_bytes(B, T, S, DRAWS, left, right), clean=(obs, frames, A, pi, u),
        run=run, check=check, dirty=dirty_torch(obs, frames, A, pi, u, band), route=route,
        small=(lambda: sample_band_case(*smaller(B, T, S), left, right, background, small=False)) if small else None)


# name -> how to build the case (built once, on first use: the inputs of the large ones take a moment)
CASES = {
    # forward_backward, forward_backward_counts: the direct step (Sp = 96, Mp = 128, three partials) and the staged one
    'posteriors-3x6x70': lambda: posterior_case(3, 6, 70),
    'posteriors-staged-Bx3x1441': lambda: posterior_case(staged_batch(1441), 3, 1441),     # 384 items at 256 units
    'counts-3x6x70': lambda: counts_case(3, 6, 70),
    'counts-staged-Bx3x1441': lambda: counts_case(staged_batch(1441), 3, 1441),
    # the uniform posterior route: the scalar and the vector row kernel
    'posteriors-uniform-3x6x70': lambda: posterior_case(3, 6, 70, uniform=True),
    'posteriors-uniform-3x6x72': lambda: posterior_case(3, 6, 72, uniform=True),
    # forward_backward_banded: G = 1; G = 8 with a partial last tile and a finite background
    'band-3x6x70-2.1-inf': lambda: band_case(3, 6, 70, 2, 1, NINF, 1),
    'band-2050x3x33-0.3-9': lambda: band_case(2050, 3, 33, 0, 3, -9.0, 8),
    # forward_backward_counts_banded: planes = B; G = 2 with a partial last tile; 512 planes for 513 tiles (the persistent
    # loop over the planes behind the band layout)
    'band-counts-3x6x70-2.1-inf': lambda: counts_band_case(3, 6, 70, 2, 1, NINF, 1),
    'band-counts-515x4x65-2.1-6': lambda: counts_band_case(515, 4, 65, 2, 1, -6.0, 2),
    'band-counts-4100x3x33-1.2-inf': lambda: counts_band_case(4100, 3, 33, 1, 2, NINF, 8),
    # decode_k_best, k = 3: the general and the uniform route, ragged lengths with an item of one frame
    'k-best-3x6x70': lambda: k_best_case(3, 6, 70),
    'k-best-uniform-3x6x70': lambda: k_best_case(3, 6, 70, uniform=True),
    # decode_k_best_banded, k = 3: -inf and a finite background
    'k-best-band-3x6x72-2.1-inf': lambda: k_best_band_case(3, 6, 72, 2, 1, NINF),
    'k-best-band-3x6x72-1.2-20': lambda: k_best_band_case(3, 6, 72, 1, 2, -20.0),
    # forward_sample, 5 draws: scalar rows; float4 rows (the held instance); the uniform route
    'sample-3x6x70': lambda: sample_case(3, 6, 70),
    'sample-3x6x72': lambda: sample_case(3, 6, 72),
    'sample-uniform-3x6x70': lambda: sample_case(3, 6, 70, uniform=True),
    # forward_sample_banded, 5 draws: -inf and a finite background
    'sample-band-3x6x70-2.1-inf': lambda: sample_band_case(3, 6, 70, 2, 1, NINF),
    'sample-band-3x6x72-1.2-20': lambda: sample_band_case(3, 6, 72, 1, 2, -20.0),
}


@functools.lru_cache(maxsize=None)
def case_of(name):
    return CASES[name]()


def to_host(out):
    torch.cuda.synchronize()
    return tuple(t.cpu() if isinstance(t, torch.Tensor) else t for t in out)


@functools.lru_cache(maxsize=None)
def fresh(name, small=False):
    """The clean problem of a case (or its smaller one) in a workspace of its own that held zeros: what (b) and (c) compare
    with, computed once."""
    case = case_of(name).small() if small else case_of(name)
    return to_host(case.run(case.clean, guarded(case.need, fill=0x00)))


# ------------------------------------------------------------------------------------------------ the four properties
@pytest.mark.parametrize('offset', [0, 1])
@pytest.mark.parametrize('name', list(CASES))
def test_exact_size_at_any_base(name, offset):
    case = case_of(name)
    case.route()
    ws = guarded(case.need, offset=offset)
    out = case.run(case.clean, ws)
    case.check(out)
    assert_guards_intact(ws)


@pytest.mark.parametrize('name', list(CASES))
def test_stale_bytes_do_not_matter(name):
    case = case_of(name)
    results = []
    for fill in (0x00, 0xFF):
        ws = guarded(case.need, offset=1, fill=fill)
        out = case.run(case.clean, ws)
        case.check(out)
        assert_guards_intact(ws)
        results.append(to_host(out))
    assert_same_bits(results[1], results[0], 'a workspace of 0xFF against one of 0x00')
    assert_same_bits(results[0], fresh(name), 'base + 1 against an aligned base')


@pytest.mark.parametrize('name', list(CASES))
def test_a_dirty_predecessor_does_not_matter(name):
    case = case_of(name)
    ws = guarded(case.need, offset=1, fill=0xFF)
    for bad in case.dirty:
        flagged = to_host(case.run(bad, ws))
        assert any(not torch.equal(bits(a), bits(b)) for a, b in zip(flagged, fresh(name)))      # (the flag showed)
    assert_same_bits(to_host(case.run(case.clean, ws)), fresh(name), 'after calls that raise every flag')
    case.check(fresh(name))
    little = case.small()
    assert little.need <= case.need
    assert_same_bits(to_host(little.run(little.clean, ws)), fresh(name, small=True), 'a smaller problem in the same workspace')
    # ... and the first problem again, behind the smaller one's layout
    assert_same_bits(to_host(case.run(case.clean, ws)), fresh(name), 'after a smaller problem')
    assert_guards_intact(ws)


@pytest.mark.parametrize('name', list(CASES))
def test_one_byte_short_raises(name):
    case = case_of(name)
    ws = guarded(case.need, fill=0x5A)
    with pytest.raises(RuntimeError, match='workspace'):
        case.run(case.clean, ws[:case.need - 1])
    torch.cuda.synchronize()
    assert bool((ws == 0x5A).all())                              # nothing was launched
    assert_guards_intact(ws)


# ------------------------------------------------------------------------------------------------ the streaming state
def pushes_that_grow_the_ring(B, seed):
    """Ragged pushes whose widths 20 and 40 need more than the ring's 16 and then 32 slots (every push has a stream that takes
    the whole width and one that takes nothing), small ones between them; and the frames the longest stream needs."""
    rng = np.random.default_rng(seed)
    out = []
    for k, Tc in enumerate((5, 20, 3, 7, 40, 1, 8, 6)):
        f = rng.integers(0, Tc + 1, size=B)
        f[k % B], f[(k + 1) % B] = Tc, 0
        out.append((Tc, f.astype(np.int64)))
    return out, int(np.sum([f for _, f in out], axis=0).max())


@pytest.mark.parametrize('kind', ['dense', 'max_lag_5', 'band'])
def test_streaming_state_of_exactly_its_size_at_base_plus_4(kind, monkeypatch):
    """The decoder's state is the caller's at the C ABI, "no alignment beyond 4" (include/torbi_hip.h): every state the
    decoder allocates is moved, contents included, into exactly torbi_hip_stream_state_bytes at base + 4 over 0xFF.  The
    ring grows twice; the outputs are those of the whole-sequence decode (with a maximum lag: of the brute-force rule of
    tests/stream_lag_cases.py, push by push), and no state was written outside."""
    B, S = (3, 72) if kind == 'band' else (3, 70)
    held = []
    grow = StreamDecoder._grow

    def guarded_grow(self, capacity):
        grow(self, capacity)
        assert self._state_bytes == _lib.load().torbi_hip_stream_state_bytes(B, S, self._capacity) == self._state.numel()
        state = guarded(self._state_bytes, offset=4, fill=0xFF)
        state.copy_(self._state)
        self._state = state
        held.append(state)

    monkeypatch.setattr(StreamDecoder, '_grow', guarded_grow)
    pushes, T = pushes_that_grow_the_ring(B, seed=S)
    obs, trans, init = synth.problem(B, T, S, seed=S)
    if kind == 'band':
        trans = stbc.band_matrix(S, 2, 1, NINF, seed=S)
        assert torbi_amd.stream_route(torch.from_numpy(trans).to(DEV), B, S, gpu=0, log_probs=True) == 'band'
    source = [obs[b] for b in range(B)]
    dec = StreamDecoder(B, S, torch.from_numpy(trans).to(DEV), torch.from_numpy(init).to(DEV), log_probs=True, gpu=0,
                        max_lag=5 if kind == 'max_lag_5' else None)
    assert dec.route == ('band' if kind == 'band' else 'dense') and dec.capacity == INITIAL_CAPACITY and len(held) == 1
    if kind == 'max_lag_5':
        clamp = lambda x: inputs.observation(torch.from_numpy(np.ascontiguousarray(x)), True, DEV).cpu().numpy()
        stream_lag_cases.feed_bounded(dec, source, trans, init, pushes, prepare=clamp, device=DEV)
    else:
        got, n = stream_cases.feed(dec, source, pushes, device=DEV)
        want = torbi_amd.from_probabilities(torch.from_numpy(obs).to(DEV), torch.from_numpy(n.astype(np.int32)).to(DEV),
                                            torch.from_numpy(trans).to(DEV), torch.from_numpy(init).to(DEV), True, gpu=0)
        want = want.cpu().numpy()
        for b in range(B):
            assert n[b] >= 1 and np.array_equal(got[b], want[b, :n[b]]), (b, np.flatnonzero(got[b] != want[b, :n[b]])[:10])
    assert len(held) >= 3 and dec.capacity >= 64, (len(held), dec.capacity)            # the ring grew twice
    for state in held:
        assert_guards_intact(state)
