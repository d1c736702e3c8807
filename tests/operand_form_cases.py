"""What tests/test_operand_forms_gpu.py and tests/test_operand_forms_cpu.py share: the FORMS an operand can arrive in
(strided, offset, another dtype, on the host), the ENTRIES that take an observation, each described once, and the comparison
`same`: bit equality against the same entry on plain copies.

The plain copy of an operand is `x.detach().to(torch.float32).contiguous().clone()` on the compute device -- for
`batch_frames` the int32 tensor, clamped to [1, T] where the entry says it clamps.  That copy is the contract of
`_lib.run`, `inputs.observation`, `inputs.plain_matrix` and `stream_ring.model`, and every route is deterministic, so a
form's outputs equal the plain copy's bit for bit.

Which form applies to which operand is FORMS; what an entry does NOT take is in its row (`raises`, `out_of_range`, `cpu`),
not in a test body:
* `decode`, `decode_cpu`, `decode_uniform` raise 'expected scalar type' for every operand of another dtype, and
  `from_probabilities` for `transition` and `initial` (its observation and frames are converted), like upstream;
* frames outside [1, T] are clamped by every entry that documents it; `decode` and its kin do not document it and the
  stream classes refuse them, so the out-of-range form is not theirs;
* `log_likelihood` returns its value and its gradients in the dtypes of its operands: a form's outputs are compared in the
  narrower of the two dtypes.
"""
import functools
import inspect
import math

import torch

import torbi_amd

import stream_band_cases as sbc

B, T, S, S_ODD = 3, 6, 64, 65          # 64: the fewest states viterbi.band_over answers for; 65: odd rows, unaligned
K = DRAWS = LAG = MAX_LAG = 2
FRAMES = (6, 4, 1)
PUSH = 3                               # a stream gets frames 0 .. 2 of every item, then SECOND[b] of the 3 that follow
SECOND = (3, 1, 0)
STREAMED = tuple(PUSH + n for n in SECOND)
WEIGHTS = (1., .5, 1.5)                # (within the 0.5 .. 1.5 of tests/test_counts_gpu.py, whose bounds the anchors use)
NINF = -math.inf
TINY = float(sbc.TINY)
# name -> (states, reach_left, reach_right, background): 3/2 is asymmetric, so a mirrored look is another band; 2/2 the control
MODELS = {'band': (S, 3, 2, NINF), 'band_tiny': (S, 3, 2, TINY), 'symmetric': (S, 2, 2, NINF), 'dense': (S_ODD, None, None, None)}
KINDS = ('observation', 'batch_frames', 'transition', 'initial', 'item_weights', 'uniforms')
FORMS = {
    'observation': ('plain', 'every_other', 'time_slice', 'offset4', 'float64', 'float16', 'bfloat16'),
    'batch_frames': ('plain', 'every_other', 'offset4', 'int64', 'host', 'out_of_range'),
    'transition': ('plain', 'transposed', 'every_other', 'offset4', 'float64', 'float16', 'bfloat16', 'host'),
    'initial': ('plain', 'every_other', 'offset4', 'expanded', 'float64', 'float16', 'bfloat16', 'host'),
    'item_weights': ('plain', 'every_other', 'offset4', 'expanded', 'float64', 'float16', 'bfloat16', 'host'),
    'uniforms': ('plain', 'every_other', 'offset4', 'float64', 'float16', 'bfloat16', 'host'),
}
OTHER_DTYPES = ('float64', 'float16', 'bfloat16', 'int64')
# every operand in a non-plain form at once (the forms that keep float32 / int32, so that every entry takes them)
TOGETHER = {'observation': 'time_slice', 'batch_frames': 'every_other', 'transition': 'transposed', 'initial': 'offset4',
            'item_weights': 'every_other', 'uniforms': 'offset4'}


@functools.lru_cache(maxsize=None)
def problem(model):
    """name of an operand -> its plain host tensor (log space; never written) for a model of MODELS."""
    states, left, right, background = MODELS[model]
    g = torch.Generator().manual_seed(states)
    if left is None:
        A = torch.log_softmax(2 * torch.randn(states, states, generator=g), 0)
    else:
        A = torch.from_numpy(sbc.band_matrix(states, left, right, background, seed=7))
    return {'observation': torch.log_softmax(3 * torch.randn(B, T, states, generator=g), 2),
            'batch_frames': torch.tensor(FRAMES, dtype=torch.int32),
            'transition': A,
            'initial': torch.log_softmax(torch.randn(states, generator=g), 0),
            'item_weights': torch.tensor(WEIGHTS),
            'uniforms': torch.rand((B, DRAWS, T), generator=g)}


def _filler(dtype):
    """What the elements around a view hold: NaN for scores (a kernel that reads one shows it), -7 for counts."""
    return math.nan if dtype.is_floating_point else -7


def form(name, x, device):
    """(the values of the plain host tensor `x` in form `name` on `device`, the base it was cut from).  `expanded` and
    `out_of_range` change the values: the reference is always the plain copy of the FORM."""
    device = torch.device(device)
    if name == 'plain':
        t = x.to(device).clone()
        return t, t
    if name == 'transposed':
        base = x.to(device).t().contiguous()
        return base.t(), base
    if name == 'every_other':
        wide = [2 * n if k in (0, x.dim() - 1) else n for k, n in enumerate(x.shape)]
        base = torch.full(wide, _filler(x.dtype), dtype=x.dtype, device=device)
        view = base[tuple(slice(None, None, 2) if k in (0, x.dim() - 1) else slice(None) for k in range(x.dim()))]
        view.copy_(x)
        return view, base
    if name == 'time_slice':
        base = torch.full((x.shape[0], x.shape[1] + 5, x.shape[2]), math.nan, dtype=x.dtype, device=device)
        view = base[:, 2:2 + x.shape[1]]
        view.copy_(x)
        return view, base
    if name == 'offset4':
        base = torch.full((x.numel() + 7,), _filler(x.dtype), dtype=x.dtype, device=device)
        view = base[1:1 + x.numel()].view(x.shape)
        view.copy_(x)
        assert view.is_contiguous() and view.data_ptr() % 16 == 4
        return view, base
    if name == 'expanded':
        base = torch.full((1,), float(x[0]), dtype=x.dtype, device=device)
        return base.expand(x.shape[0]), base
    if name in OTHER_DTYPES:
        t = x.to(device=device, dtype=getattr(torch, name))
        return t, t
    if name == 'host':
        t = x.clone()
        return t, t
    if name == 'out_of_range':
        t = x.to(device).clone()
        t[0], t[1] = 0, T + 3
        return t, t
    raise KeyError(name)


def plain_copy(x, device, clamp=False):
    x = x.detach()
    if x.dtype.is_floating_point:
        return x.to(device=device, dtype=torch.float32).contiguous().clone()
    x = x.to(device=device, dtype=torch.int64)
    return (x.clamp(1, T) if clamp else x).to(torch.int32).contiguous().clone()


def bits(t):
    """A tensor's bits, as int32 / int64 words on the host."""
    t = t.detach().cpu().contiguous()
    if t.dtype.is_floating_point:
        return t.view({2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])
    return t


def same(got, want, what=''):
    """Every output of `got` equals its partner in `want` bit for bit, NaN patterns included.  Outputs that follow an
    operand's dtype (`log_likelihood`) are compared in the narrower of the two dtypes."""
    assert len(got) == len(want), (what, len(got), len(want))
    for k, (g, w) in enumerate(zip(got, want)):
        if not isinstance(g, torch.Tensor):
            assert g == w, (what, k, g, w)
            continue
        assert g.shape == w.shape, (what, k, g.shape, w.shape)
        if g.dtype != w.dtype:
            assert g.dtype.is_floating_point and w.dtype.is_floating_point, (what, k, g.dtype, w.dtype)
            narrow = g.dtype if torch.finfo(g.dtype).bits <= torch.finfo(w.dtype).bits else w.dtype
            g, w = g.detach().cpu().to(narrow), w.detach().cpu().to(narrow)
        assert torch.equal(bits(g), bits(w)), (what, k)


class Entry:
    """One row of the table.  `call(ops, gpu)` takes name -> tensor for the entry's `operands` and returns a tuple of
    outputs; `api`: the names of torbi_amd.__all__ the row covers; `model`: the key of MODELS it runs at; `raises`: the
    operands whose other dtypes raise 'expected scalar type'; `out_of_range`: frames are clamped to [1, T]; `cpu`: has a
    `gpu=None` route (or takes CPU tensors), `gpu`: runs on a HIP device; `route` / `band`: has a `route=` argument / a stated band; `in_place`: may
    write a float32 observation on the compute device, which `from_probabilities` documents; `frames`: its own plain frames."""

    def __init__(self, name, api, operands, model, call, raises=(), out_of_range=True, cpu=False, route=False, band=False,
                 in_place=False, frames=None, gpu=True):
        self.name, self.api, self.operands, self.model, self.call = name, tuple(api), tuple(operands), model, call
        self.raises, self.out_of_range, self.cpu, self.route, self.band = tuple(raises), out_of_range, cpu, route, band
        self.in_place, self.frames, self.gpu = in_place, frames, gpu

    def plain(self):
        """name -> plain host tensor of every operand of the entry."""
        ops = {k: v for k, v in problem(self.model).items() if k in self.operands}
        if self.frames is not None:
            ops['batch_frames'] = torch.tensor(self.frames, dtype=torch.int32)
        return ops

    def forms(self, operand, device):
        """The forms of FORMS that apply to `operand` of this entry on `device`."""
        out = []
        for name in FORMS[operand]:
            if name == 'host' and torch.device(device).type == 'cpu':
                continue                       # (the operand is where the observation is)
            if name == 'out_of_range' and not self.out_of_range:
                continue
            if name == 'transposed' and problem(self.model)[operand].dim() != 2:
                continue
            out.append(name)
        return out

    def refuses(self, operand, form_name):
        return operand in self.raises and form_name in OTHER_DTYPES


O, F, A, PI, W, U = KINDS
BAND = MODELS['band'][1:]
UNIFORM = float(torch.tensor(math.log(1. / S), dtype=torch.float32))


def _model(o, gpu, **more):
    return dict(batch_frames=o[F], transition=o[A], initial=o[PI], log_probs=True, gpu=gpu, **more)


def _log_likelihood(o, gpu):
    leaves = [o[k].detach().requires_grad_() for k in (O, A, PI)]
    L = torbi_amd.log_likelihood(leaves[0], o[F], leaves[1], leaves[2], route='auto')
    (L * torch.tensor(WEIGHTS, dtype=L.dtype, device=L.device)).sum().backward()
    return (L.detach(), *(x.grad for x in leaves))


def _pushes(obs, second):
    """The two pushes of a stream, every chunk cut from the caller's observation where it lives."""
    return (obs[:, :PUSH], None), (obs[:, PUSH:], second)


def _stream_decoder(route):
    def call(o, gpu):
        out = []
        for max_lag in (None, MAX_LAG):
            dec = torbi_amd.StreamDecoder(B, S, o[A], o[PI], log_probs=True, gpu=gpu, max_lag=max_lag, route=route)
            assert dec.route == ('host' if gpu is None else route)
            parts = [dec.push(chunk, frames) for chunk, frames in _pushes(o[O], o[F])] + [dec.flush()]
            out += [torch.cat(per_stream) for per_stream in zip(*parts)] + [dec.forced]
        return tuple(out)
    return call


def _stream_posteriors(route):
    def call(o, gpu):
        sp = torbi_amd.StreamPosteriors(B, S, o[A], o[PI], log_probs=True, gpu=gpu, lag=LAG, route=route)
        assert sp.route == ('host' if gpu is None else route)
        out = []
        for chunk, frames in _pushes(o[O], o[F]):
            out += [*sp.push(chunk, frames), sp.filtered(), sp.log_likelihood]
        rest, final = sp.flush()
        return (*out, *rest, final)
    return call


def _routes(o, gpu):
    return (torbi_amd.posterior_route(o[A], B, T, S, gpu=gpu, log_probs=True),
            torbi_amd.counts_route(o[A], B, T, S, gpu=gpu, log_probs=True),
            torbi_amd.sample_route(o[A], B, T, S, draws=DRAWS, gpu=gpu, log_probs=True),
            torbi_amd.k_best_route(o[A], B, T, S, K, gpu=gpu, log_probs=True),
            torbi_amd.stream_route(o[A], B, S, gpu=gpu, log_probs=True),
            torbi_amd.stream_posterior_route(o[A], B, S, gpu=gpu, log_probs=True))


OFAP = (O, F, A, PI)
ENTRIES = [
    Entry('decode', ['decode'], OFAP, 'dense', lambda o, gpu: (torbi_amd.decode(o[O], o[F], o[A], o[PI]),),
          raises=OFAP, out_of_range=False),
    Entry('decode_cpu', ['decode_cpu'], OFAP, 'dense', lambda o, gpu: (torbi_amd.decode_cpu(o[O], o[F], o[A], o[PI]),),
          raises=OFAP, out_of_range=False, cpu=True, gpu=False),
    Entry('decode_uniform', ['decode_uniform'], (O, F, PI), 'band',
          lambda o, gpu: (torbi_amd.decode_uniform(o[O], o[F], UNIFORM, o[PI]),), raises=(O, F, PI), out_of_range=False),
    Entry('from_probabilities', ['from_probabilities'], OFAP, 'dense',
          lambda o, gpu: (torbi_amd.from_probabilities(o[O], **_model(o, gpu)),), raises=(A, PI), out_of_range=False,
          cpu=True, in_place=True),
    Entry('forward_backward', ['forward_backward'], OFAP, 'dense',
          lambda o, gpu: torbi_amd.forward_backward(o[O], o[F], o[A], o[PI])),
    Entry('forward_backward_banded', ['forward_backward_banded'], OFAP, 'band',
          lambda o, gpu: torbi_amd.forward_backward_banded(o[O], o[F], o[A], o[PI], *BAND), band=True),
    Entry('forward_backward_counts', ['forward_backward_counts'], OFAP + (W,), 'dense',
          lambda o, gpu: torbi_amd.forward_backward_counts(o[O], o[F], o[A], o[PI], o[W])),
    Entry('forward_backward_counts_banded', ['forward_backward_counts_banded'], OFAP + (W,), 'band',
          lambda o, gpu: torbi_amd.forward_backward_counts_banded(o[O], o[F], o[A], o[PI], *BAND, item_weights=o[W]), band=True),
    Entry('state_posteriors', ['state_posteriors'], OFAP, 'band',
          lambda o, gpu: torbi_amd.state_posteriors(o[O], **_model(o, gpu, route='auto')), cpu=True, route=True),
    Entry('expected_counts', ['expected_counts'], OFAP, 'band',
          lambda o, gpu: torbi_amd.expected_counts(o[O], **_model(o, gpu, route='auto')), cpu=True, route=True),
    Entry('log_likelihood', ['log_likelihood'], OFAP, 'band', _log_likelihood, cpu=True, route=True),
    Entry('decode_k_best', ['decode_k_best'], OFAP, 'dense',
          lambda o, gpu: torbi_amd.decode_k_best(o[O], o[F], o[A], o[PI], K, route='dense'), route=True),
    Entry('decode_k_best_banded', ['decode_k_best_banded'], OFAP, 'band',
          lambda o, gpu: torbi_amd.decode_k_best_banded(o[O], o[F], o[A], o[PI], K, *BAND), band=True),
    Entry('best_paths', ['best_paths'], OFAP, 'band',
          lambda o, gpu: torbi_amd.best_paths(o[O], K, **_model(o, gpu, route='auto')), cpu=True, route=True),
    Entry('forward_sample', ['forward_sample'], OFAP + (U,), 'dense',
          lambda o, gpu: torbi_amd.forward_sample(o[O], o[F], o[A], o[PI], o[U])),
    Entry('forward_sample_banded', ['forward_sample_banded'], OFAP + (U,), 'band',
          lambda o, gpu: torbi_amd.forward_sample_banded(o[O], o[F], o[A], o[PI], o[U], *BAND), band=True),
    Entry('sample_paths', ['sample_paths'], OFAP + (U,), 'band',
          lambda o, gpu: torbi_amd.sample_paths(o[O], DRAWS, uniforms=o[U], **_model(o, gpu, route='auto')), cpu=True,
          route=True),
    Entry('StreamDecoder-dense', ['StreamDecoder'], OFAP, 'band', _stream_decoder('dense'), out_of_range=False, cpu=True,
          route=True, frames=SECOND),
    Entry('StreamDecoder-band', ['StreamDecoder'], OFAP, 'band', _stream_decoder('band'), out_of_range=False, route=True,
          frames=SECOND),
    Entry('StreamPosteriors-dense', ['StreamPosteriors'], OFAP, 'band', _stream_posteriors('dense'), out_of_range=False,
          cpu=True, route=True, frames=SECOND),
    Entry('StreamPosteriors-band', ['StreamPosteriors'], OFAP, 'band', _stream_posteriors('band'), out_of_range=False,
          route=True, frames=SECOND),
    Entry('routes', ['posterior_route', 'counts_route', 'sample_route', 'k_best_route', 'stream_route',
                     'stream_posterior_route'], (A,), 'band', _routes, route=True),
]
BY_NAME = {e.name: e for e in ENTRIES}
# public names that take an observation and have no row, each with its reason
NOT_TABLED = {
    'chunk': 'torch ops on one (frames, states) host tensor, in the dtype it is given: no front, no kernel',
    'DecodePipeline': "`decode`'s arguments, handed to decode_batches, which takes contiguous float32 device tensors and "
                      'raises for anything else (tests/test_gpu_parity.py)',
}


def takes_an_observation(thing):
    """A public function with an `observation` parameter, or a class one of whose public methods has one."""
    if inspect.isclass(thing):
        return any(takes_an_observation(member) for name, member in vars(thing).items()
                   if not name.startswith('_') and inspect.isfunction(member))
    return inspect.isfunction(thing) and 'observation' in inspect.signature(thing).parameters


def cases(device, cpu_only=False):
    """(entry name, operand, form) of every case on `device`, 'plain' left to the anchors."""
    out = []
    for entry in ENTRIES:
        if not (entry.cpu if cpu_only else entry.gpu):
            continue
        for operand in entry.operands:
            out += [(entry.name, operand, name) for name in entry.forms(operand, device) if name != 'plain']
    return out


class Snapshot:
    """The bits of a caller's tensors and of the bases they were cut from, to be found again after a call."""

    def __init__(self, tensors):
        self.kept = [(t, bits(t).clone()) for t in tensors]

    def check(self, what='', written=()):
        """Nothing changed -- except, for the tensors of `written` (a documented in-place path), inside the view: those
        are put back first, so that what surrounds them in their base is still checked."""
        for t, before in self.kept:
            if any(t is w for w in written):
                t.copy_(before.view(t.dtype).to(t.device))
        for k, (t, before) in enumerate(self.kept):
            assert torch.equal(bits(t), before), (what, 'tensor', k, 'was written')


def operands(entry, device, forms=None):
    """(ops, plain ops, Snapshot) for `entry` on `device` with operand -> form name in `forms` (the rest plain)."""
    forms = forms or {}
    device = torch.device(device)
    ops, bases = {}, []
    for name, x in entry.plain().items():
        ops[name], base = form(forms.get(name, 'plain'), x, device)
        bases.append(base)
    plain = {name: plain_copy(t, device, clamp=entry.out_of_range and name == F) for name, t in ops.items()}
    return ops, plain, Snapshot(list(ops.values()) + bases)


_references = {}


def reference(entry, plain, gpu):
    """The entry on plain copies, computed once per distinct content of the operands and left unchanged."""
    key = (entry.name, gpu) + tuple(bits(plain[name]).numpy().tobytes() for name in entry.operands)
    if key not in _references:
        _references[key] = tuple(x.detach().clone() if isinstance(x, torch.Tensor) else x for x in entry.call(plain, gpu))
    return _references[key]


def check_forms(entry, device, gpu, forms):
    """The body of a case: `entry` with operand -> form in `forms` raises 'expected scalar type' where its row says so --
    before anything runs: the next plain call is unchanged --, else equals the plain copies' call bit for bit; either way
    the caller's tensors and their bases keep their bits (but for the documented in-place path).  Returns (ops, outputs)."""
    ops, plain, snapshot = operands(entry, device, forms)
    what = (entry.name, forms)
    if any(entry.refuses(operand, name) for operand, name in forms.items()):
        before = reference(entry, operands(entry, device)[1], gpu)
        try:
            entry.call(ops, gpu)
        except RuntimeError as error:
            assert 'expected scalar type' in str(error), (what, error)
        else:
            raise AssertionError((what, 'did not raise'))
        snapshot.check(what)
        same(entry.call(operands(entry, device)[1], gpu), before, what)
        return ops, None
    want = reference(entry, plain, gpu)
    got = entry.call(ops, gpu)
    same(got, want, what)
    observation = ops.get(O)
    in_place = (entry.in_place and observation is not None and observation.dtype == torch.float32
                and observation.device.type == torch.device(device).type)
    snapshot.check(what, written=[observation] if in_place else [])
    return ops, got
