"""torbi_amd.StreamDecoder(max_lag=...) on the HIP route: stream_walk_kernel<false, true> behind torbi_hip_stream_push_lag,
at the smallest shapes where the bounded arm can go wrong.  Every push is checked against the brute-force rule of
tests/stream_lag_cases.py (numpy float32, fed the epsilon round trip computed by torch ops ON THE DEVICE) and, where a host
decoder runs alongside, against the host route bit for bit."""
import numpy as np
import pytest
import torch

import torbi_amd
from torbi_amd import _lib, synth
from torbi_amd.stream import INITIAL_CAPACITY
from stream_lag_cases import feed_bounded, identity, nonfinite_scenario, flush_scenario

pytestmark = pytest.mark.gpu

DEV = torch.device('cuda:0')


def clamp(obs):
    """log(exp(x) + tiny) by torch ops on the device."""
    x = torch.from_numpy(np.ascontiguousarray(obs, dtype=np.float32)).to(DEV)
    torch.exp_(x)
    x += torch.finfo(torch.float32).tiny
    torch.log_(x)
    return x.cpu().numpy()


def decoder(B, S, trans, init, max_lag, gpu=0):
    where = DEV if gpu is not None else 'cpu'
    return torbi_amd.StreamDecoder(B, S, torch.from_numpy(trans).to(where), torch.from_numpy(init).to(where), log_probs=True,
                                   gpu=gpu, max_lag=max_lag)


def ragged(B, pushes, seed, lowest=0):
    """`pushes` pushes of Tc = 1 .. 8 frames, per-stream counts lowest .. Tc with a 0 and a full count in every push (a 1 in
    place of the 0 where lowest = 1); and the frames the longest stream needs."""
    rng = np.random.default_rng(seed)
    out = []
    for k in range(pushes):
        Tc = int(rng.integers(1, 9))
        f = rng.integers(lowest, Tc + 1, size=B)
        if B > 1:
            f[k % B], f[(k + 1) % B] = lowest, Tc
        out.append((Tc, f.astype(np.int64)))
    return out, int(np.sum([f for _, f in out], axis=0).max())


def problem(kind, B, T, S, seed):
    """dense: a random matrix that favours staying (+6 on the diagonal keeps frames undecided for longer, so that the
    bound binds); zero: every score 0, so that every argmax -- backpointers and final states -- is a tie."""
    obs, trans, init = synth.problem(B, T, S, seed=seed)
    if kind == 'dense':
        trans = trans.copy()
        trans[np.arange(S), np.arange(S)] += np.float32(6.)
    else:
        obs, trans, init = np.zeros_like(obs), np.zeros_like(trans), np.zeros_like(init)
    return [obs[b] for b in range(B)], trans, init


def state_bytes(B, S, capacity):
    return 4 * (B * capacity * S + B * capacity + B * S)


# ------------------------------------------------------------------------------------------------ 1: the prefix property
@pytest.mark.parametrize('kind', ['dense', 'zero'])
@pytest.mark.parametrize('max_lag', [0, 1, 5, 15])
@pytest.mark.parametrize('S', [2, 3, 63, 64, 65, 257])
def test_every_push_is_a_span_of_the_whole_decode_of_the_frames_so_far(S, max_lag, kind):
    """Wave and workgroup edges of the final state and the backpointers; outputs, `pending`, `forced` by brute force and
    equal to the host route's after every push; the ring within its bound."""
    B = 5
    pushes, T = ragged(B, 12, seed=S + max_lag)
    source, trans, init = problem(kind, B, T, S, seed=S)
    dec, twin = decoder(B, S, trans, init, max_lag), decoder(B, S, trans, init, max_lag, gpu=None)
    total = [0]

    def after(k, d):
        total[0] = int(d.forced.sum())
        assert d.capacity <= max(INITIAL_CAPACITY, 1 << (max_lag + 8).bit_length())     # the power of two >= max_lag + Tc + 1
    feed_bounded(dec, source, trans, init, pushes, prepare=clamp, device=DEV, twin=twin, after=after)
    print(f'S = {S}, max_lag = {max_lag}, {kind}: {total[0]} frames forced')
    if kind == 'zero':                                         # one frame stays pending naturally: only max_lag = 0 forces
        assert (total[0] > 0) == (max_lag == 0)
    elif max_lag <= 1:
        assert total[0] > 0


# ---------------------------------------------------------------------------------------------------------- 2: ring wrap
def test_ring_stays_at_its_first_capacity_while_the_window_wraps():
    """Identity matrix: nothing is ever decided, every returned frame is forced.  Sixty pushes of 1 .. 8 frames move the
    window round the 16 slots many times; the ring never grows."""
    B, S, max_lag = 17, 64, 5
    pushes, T = ragged(B, 60, seed=2, lowest=1)
    obs, _, init = synth.problem(B, T, S, seed=9)
    source, eye = [obs[b] for b in range(B)], identity(S)
    dec = decoder(B, S, eye, init, max_lag)
    assert dec.capacity == INITIAL_CAPACITY == 16
    seen = []

    def after(k, d):
        assert d.capacity == 16 and int(d.pending.max()) <= max_lag and d._state_bytes == state_bytes(B, S, 16)
        seen.append((d.forced.clone(), d.frames.clone(), d.pending.clone()))
    feed_bounded(dec, source, eye, init, pushes, prepare=clamp, device=DEV, after=after)
    forced, frames, pending = seen[-1]
    assert torch.equal(forced, frames - pending) and int(frames.min()) >= 60 and int(frames.max()) > 4 * 16


# --------------------------------------------------------------------------------------------------------- 3: mixed tile
def test_streams_without_frames_beside_neighbours_with_five():
    B, S, max_lag, Tc = 17, 64, 4, 5
    pushes = [(Tc, np.where((np.arange(B) + k) % 3 == 0, 0, Tc).astype(np.int64)) for k in range(12)]
    T = int(np.sum([f for _, f in pushes], axis=0).max())
    obs, _, init = synth.problem(B, T, S, seed=13)
    band = synth.banded_transition(S, 5)
    dec, twin = decoder(B, S, band, init, max_lag), decoder(B, S, band, init, max_lag, gpu=None)
    # (feed_bounded: a stream that took 0 frames returns nothing and its `forced` does not move)
    feed_bounded(dec, [obs[b] for b in range(B)], band, init, pushes, prepare=clamp, device=DEV, twin=twin)


# ------------------------------------------------------------------------------------------- 4: the workload's state count
def test_pitch_band_of_1440_states_in_one_frame_pushes():
    B, S, T, max_lag = 1, 1440, 60, 8
    obs, _, init = synth.problem(B, T, S, seed=21)
    band = synth.banded_transition(S, 87.2)
    total = [0]

    def after(k, d):
        total[0] = int(d.forced.sum())
    feed_bounded(decoder(B, S, band, init, max_lag), [obs[0]], band, init, [(1, np.ones(1, dtype=np.int64))] * T,
                 prepare=clamp, device=DEV, after=after)
    print(f'1440 states, max_lag = {max_lag}: {total[0]} of {T} frames forced')


# ------------------------------------------------------------------------------------------------- 5: NaN, -inf and flush
@pytest.mark.parametrize('max_lag', [0, 2])
def test_forced_path_starts_at_the_first_nan_and_ties_of_minus_infinity_go_to_state_0(max_lag):
    nonfinite_scenario(decoder, max_lag, prepare=clamp, device=DEV)


def test_flush_of_one_stream_half_way_restarts_it_and_leaves_its_neighbours():
    flush_scenario(decoder, prepare=clamp, device=DEV)


# ---------------------------------------------------------------------------------------------- 6: a lag that never binds
def test_a_huge_lag_is_the_unbounded_decoder():
    B, S = 5, 65
    pushes, T = ragged(B, 12, seed=S + 5)
    source, trans, init = problem('dense', B, T, S, seed=S)
    exact, bounded = decoder(B, S, trans, init, None), decoder(B, S, trans, init, 10 ** 6)
    sizes = []

    def after(k, d):
        sizes.append((d.capacity, d._state_bytes))
        assert int(d.forced.sum()) == 0
        assert d._state_bytes == state_bytes(B, S, d.capacity) == _lib.load().torbi_hip_stream_state_bytes(B, S, d.capacity)
    a, _ = feed_bounded(exact, source, trans, init, pushes, prepare=clamp, device=DEV, after=after)
    mark = len(sizes)
    b, _ = feed_bounded(bounded, source, trans, init, pushes, prepare=clamp, device=DEV, after=after)
    assert sizes[:mark] == sizes[mark:]
    for k, (x, y) in enumerate(zip(a, b)):
        assert all(np.array_equal(p, q) for p, q in zip(x, y)), k
    assert max(len(o) for out in a[:-1] for o in out) > 0
