"""Shared by tests/test_stream_posterior_cpu.py and tests/test_stream_posterior_gpu.py: problems, ragged push plans, the
float64 reference (`state_posteriors(prefix, gpu=None)`) and the check of the prefix property after every push.

The prefix property: a stream with n frames (the first `base` returned) that receives f >= 1 frames returns, with n' = n + f,
rows base .. n' - 1 - lag, each row t of `state_posteriors` on the stream's first n' frames; f == 0 changes nothing."""
import math

import numpy as np
import torch

import torbi_amd

# the project's bounds against float64 (tests/test_posterior_gpu.py::check, POSTERIOR.md)
DEVICE_GAMMA = 1e-4
HOST_GAMMA = 1e-6          # a float64 recurrence (within ~1e-9) behind a float32 cast (<= 6e-8)
ROW_SUM = 1e-4


def loglik_bound(ref, frames):
    return 1e-6 * np.abs(ref) + 4e-6 * frames


def problem(B, T, S, kind, log_probs, seed):
    """(observation (B, T, S), transition (S, S) or None, initial (S,)) float32 tensors; probabilities unless `log_probs`.
    kind: 'none' (transition=None), 'dense', 'band' (|next - prev| <= 1, zero probability outside: -inf in log space)."""
    rng = np.random.default_rng(seed)
    obs = rng.random((B, T, S)) ** 3 + 1e-3
    obs /= obs.sum(-1, keepdims=True)
    init = rng.random(S) + 0.1
    init /= init.sum()
    trans = None
    if kind != 'none':
        trans = rng.random((S, S)) + 0.05                       # [next, prev]
        if kind == 'band':
            x = np.arange(S)
            trans = np.where(np.abs(x[:, None] - x[None, :]) <= 1, trans, 0.)
        trans /= trans.sum(0, keepdims=True)
    def as_input(p):
        if p is None:
            return None
        with np.errstate(divide='ignore'):
            return torch.from_numpy((np.log(p) if log_probs else p).astype(np.float32))
    return as_input(obs), as_input(trans), as_input(init)


def ragged_plan(B, T, seed, largest=7):
    """Pushes [(Tc, frames (B,))] with Tc in 0 .. `largest` that deliver at most T frames to any stream.  With B >= 2
    every push has one stream taking 0 frames and one taking all Tc (the two rotate); a single stream takes all Tc."""
    rng = np.random.default_rng(seed)
    plan, n, k = [], np.zeros(B, dtype=np.int64), 0
    sizes = [3, 0, 1, largest, 2, 1, 5, 4, 6, 1, 2, 3]
    while True:
        Tc = sizes[k % len(sizes)]
        f = rng.integers(0, Tc + 1, size=B)
        if B >= 2:
            f[k % B], f[(k + 1) % B] = 0, Tc
        else:
            f[0] = Tc
        if (n + f).max() > T:
            return plan
        plan.append((Tc, f.astype(np.int64)))
        n += f
        k += 1


def reference(obs, n, trans, init, log_probs):
    """Float64-route posteriors of every stream's first n[b] frames: (gamma (B, max n, S), L (B,)) as float64 arrays (rows of
    a stream with n[b] == 0 are not meaningful)."""
    T = max(int(n.max()), 1)
    g, L = torbi_amd.state_posteriors(obs[:, :T], torch.from_numpy(np.maximum(n, 1)), trans, init, log_probs=log_probs, gpu=None)
    return g.numpy().astype(np.float64), L.numpy().astype(np.float64)


def same(got, want, bound, what):
    """NaN exactly where the reference has NaN, infinities equal, everything else within `bound`."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert np.array_equal(np.isnan(got), np.isnan(want)), what
    inf = np.isinf(want)
    assert np.array_equal(got[inf], want[inf]), what
    ok = ~np.isnan(want) & ~inf
    err = np.abs(got[ok] - want[ok])
    assert np.all(err <= np.broadcast_to(bound, want.shape)[ok]), (what, float(err.max()) if err.size else 0.)
    return float(err.max()) if err.size else 0.


def cpu(t):
    return t.detach().cpu().numpy()


class Feeder:
    """Feeds a (B, T, S) observation to a StreamPosteriors push by push and checks the prefix property after every push
    against the float64 reference.  `worst` collects the largest errors seen."""

    def __init__(self, sp, obs, trans, init, log_probs, gamma_bound, record=True):
        self.sp, self.obs, self.trans, self.init, self.log_probs = sp, obs, trans, init, log_probs
        self.record = record                              # keep a host copy of every returned row in `returned`
        self.bound = gamma_bound
        self.n = np.zeros(sp.batch, dtype=np.int64)
        self.base = np.zeros(sp.batch, dtype=np.int64)
        self.worst = {'gamma': 0., 'sum': 0., 'loglik_share': 0.}
        self.returned = []                                # (stream, frame, n', row) of every row a push returned

    def chunk(self, Tc, f):
        """(B, Tc, S): stream b's next f[b] frames; the frames beyond them hold NaN, which no stream may read."""
        B, S = self.sp.batch, self.sp.states
        out = torch.full((B, Tc, S), math.nan, dtype=self.obs.dtype)
        for b in range(B):
            out[b, :f[b]] = self.obs[b, self.n[b]:self.n[b] + f[b]]
        return out

    def push(self, Tc, f=None, check=True):
        sp, B, lag = self.sp, self.sp.batch, self.sp.lag
        f = np.full(B, Tc, dtype=np.int64) if f is None else np.asarray(f, dtype=np.int64)
        chunk = self.chunk(Tc, f).to(sp.device)
        rows = sp.push(chunk, None if (f == Tc).all() else torch.from_numpy(f))
        pending = self.n - self.base
        count = np.where(f > 0, np.maximum(pending + f - lag, 0), 0)
        self.n = self.n + f
        assert len(rows) == B
        for b in range(B):
            assert tuple(rows[b].shape) == (count[b], sp.states) and rows[b].dtype == torch.float32, (b, rows[b].shape, count[b])
            assert rows[b].device.type == sp.device.type
            if self.record and count[b]:
                got = cpu(rows[b])
                self.returned += [(b, int(self.base[b] + r), int(self.n[b]), got[r].copy()) for r in range(count[b])]
        if check:
            self.check_rows(rows, count)
        self.base = self.base + count
        expect = np.where(f > 0, np.minimum(pending + f, lag), pending)
        assert np.array_equal(sp.pending.numpy(), expect) and np.array_equal(sp.frames.numpy(), self.n)
        if check:
            self.check_now()
        return rows

    def check_rows(self, rows, count, n=None):
        n = self.n if n is None else n
        if not count.any():
            return
        g, _ = reference(self.obs, n, self.trans, self.init, self.log_probs)
        for b in range(self.sp.batch):
            if count[b] == 0:
                continue
            got, want = cpu(rows[b]), g[b, self.base[b]:self.base[b] + count[b]]
            self.worst['gamma'] = max(self.worst['gamma'], same(got, want, self.bound, f'rows of stream {b}'))
            if not np.isnan(want).any():
                err = float(np.abs(got.astype(np.float64).sum(-1) - 1).max())
                assert err <= ROW_SUM, (b, err)
                self.worst['sum'] = max(self.worst['sum'], err)

    def check_now(self):
        """`filtered()` and `log_likelihood` against the reference on the frames so far."""
        sp, n = self.sp, self.n
        now, score = cpu(sp.filtered()), cpu(sp.log_likelihood)
        assert now.shape == (sp.batch, sp.states) and now.dtype == np.float32 and score.shape == (sp.batch,)
        assert score.dtype == np.float32
        g, L = reference(self.obs, n, self.trans, self.init, self.log_probs)
        for b in range(sp.batch):
            if n[b] == 0:
                assert (now[b] == 0).all() and score[b] == 0
                continue
            self.worst['gamma'] = max(self.worst['gamma'], same(now[b], g[b, n[b] - 1], self.bound, f'filtered row of stream {b}'))
            bound = loglik_bound(L[b], n[b])
            err = same(score[b], L[b], bound, f'log-likelihood of stream {b}')
            if bound > 0:
                self.worst['loglik_share'] = max(self.worst['loglik_share'], err / bound)

    def flush(self, items=None, check=True):
        sp = self.sp
        chosen = list(range(sp.batch)) if items is None else list(items)
        before = cpu(sp.log_likelihood)
        rest, final = sp.flush(items)
        assert len(rest) == len(chosen) and tuple(final.shape) == (len(chosen),) and final.dtype == torch.float32
        count = np.zeros(sp.batch, dtype=np.int64)
        rows = [None] * sp.batch
        for k, b in enumerate(chosen):
            count[b] = self.n[b] - self.base[b]
            rows[b] = rest[k]
            assert tuple(rest[k].shape) == (count[b], sp.states) and rest[k].dtype == torch.float32
            assert np.array_equal(cpu(final)[k], before[b], equal_nan=True)
            if self.record and count[b]:
                got = cpu(rest[k])
                self.returned += [(b, int(self.base[b] + r), int(self.n[b]), got[r].copy()) for r in range(count[b])]
        if check:
            self.check_rows(rows, count)
        for b in set(chosen):
            self.n[b] = self.base[b] = 0
        assert np.array_equal(sp.frames.numpy(), self.n) and np.array_equal(sp.pending.numpy(), self.n - self.base)
        return rest, final

    def restart(self, b, obs_b):
        """Stream b continues with the frames `obs_b` (T', S) from its frame 0 (after a flush)."""
        self.obs = self.obs.clone()
        self.obs[b] = math.nan
        self.obs[b, :obs_b.shape[0]] = obs_b
