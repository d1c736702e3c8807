"""What the tests that look at a caller-owned workspace as MEMORY share (tests/test_workspace_bounds_gpu.py,
tests/test_workspace_contract_gpu.py): a workspace cut out of a larger allocation, at any offset, over any previous content,
with 65536 guarded bytes in front of it and behind it; the comparison of two results bit for bit; ragged lengths."""
import numpy as np
import torch

from torbi_amd import synth

DEV = torch.device('cuda:0')
GUARD = 65536


def guarded(need, offset=0, fill=0xC3):
    """A uint8 workspace of exactly `need` bytes: the slice [GUARD + offset : GUARD + offset + need] of ONE allocation of
    GUARD + offset + need + GUARD bytes that holds `fill` everywhere.  offset = 0 is 256-byte aligned (the allocator's
    alignment), offset = 1 the base that leaves a layout which rounds up by 255 the least room."""
    whole = torch.full((GUARD + offset + need + GUARD,), fill, dtype=torch.uint8, device=DEV)
    assert whole.data_ptr() % 256 == 0
    ws = whole[GUARD + offset:GUARD + offset + need]
    assert ws.numel() == need and ws.data_ptr() % 256 == offset % 256
    ws.guards = (whole, offset, fill)           # (the allocation lives as long as the slice; read by assert_guards_intact)
    return ws


def assert_guards_intact(ws):
    """Every byte of the allocation in front of `ws` and behind it still holds the fill."""
    whole, offset, fill = ws.guards
    torch.cuda.synchronize()
    front, back = whole[:GUARD + offset], whole[-GUARD:]
    touched = torch.nonzero(back != fill).flatten()
    assert touched.numel() == 0, (f'{touched.numel()} bytes written behind the workspace, the first {int(touched[0])} bytes '
                                  f'behind its end (offset {offset}, {ws.numel()} bytes)')
    touched = torch.nonzero(front != fill).flatten()
    assert touched.numel() == 0, (f'{touched.numel()} bytes written in front of the workspace, the last '
                                  f'{GUARD + offset - int(touched[-1])} bytes in front of its base (offset {offset})')


def bits(t):
    """A float32 or int32 tensor (or array) as int32, so that NaN equals NaN and -0 differs from 0."""
    if isinstance(t, np.ndarray):
        assert t.dtype in (np.float32, np.int32), t.dtype
        return torch.from_numpy(np.ascontiguousarray(t).view(np.int32))
    assert t.dtype in (torch.float32, torch.int32), t.dtype
    return t.contiguous().view(torch.int32)


def assert_same_bits(got, want, what):
    """Two results (tuples of tensors or arrays) are bit-identical, output by output."""
    assert len(got) == len(want)
    for k, (a, b) in enumerate(zip(got, want)):
        a, b = bits(a), bits(b)
        assert a.shape == b.shape
        differ = torch.nonzero((a != b).flatten()).flatten()
        assert differ.numel() == 0, f'{what}: output {k} differs in {differ.numel()} of {a.numel()} words, first at {int(differ[0])}'


def ragged(B, T, seed):
    """Lengths in 1 .. T with frames[0] = T and, where there is a second item, one item of 1 frame (the last): frames the
    kernels never write lie inside every region of the workspace that has a frame axis."""
    frames = np.clip(synth.lengths(B, 1, T, seed=seed), 1, T).astype(np.int32)
    frames[0] = T
    if B >= 2:
        frames[B - 1] = 1
    return frames


def smaller(B, T, S):
    """The shape of the second clean problem in a workspace that served (B, T, S): fewer items, fewer frames and a state count
    whose padding differs (37 -> 64 / 96 / 128 where the layouts pad to 64, 32 and 128; 68 where the route needs S % 4 == 0),
    so that every region of its layout starts somewhere else."""
    assert B >= 3 and T >= 3
    return 2, min(4, T - 1), 68 if S % 4 == 0 else 37
