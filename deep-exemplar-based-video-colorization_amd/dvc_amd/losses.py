"""train.py's pixel losses on the package's own fused reduction: `mse_loss`, `l1_loss`, `weighted_mse_loss`, `weighted_l1_loss` with
the signatures of the reference's utils/util.py, and `fused(terms)`, which evaluates any number of such terms — every term is
scale * mean(w * |input - target|^p), p in {1, 2} — with ONE dvc_loss_fwd call forward and ONE dvc_loss_bwd call backward
(csrc/loss.hip; the design, the order of the sums and the error bound are in DESIGN.md §6d).

The four helpers are `fused` with a one-row table, and a term's value is bit-identical whether it is computed alone or inside any
`fused` call: the kernel's partial sums depend on the term's data alone.  Values and gradients are bit-reproducible from run to run.

Per call the host sends the term table and the chunk table (dvc_amd.optim's) with one host-to-device copy on the current stream and
launches; the staging buffers, and `Plan`'s resident tables, follow dvc_amd.tables, where the discipline is described once.  The
tables carry addresses, so a call cannot be replayed from a captured graph: it raises while the current stream is capturing.

What is not done is refused by name: CPU tensors (no CPU fallback), non-fp32, weights that require grad (the mask is data in
train.py), broadcasts other than a Python-number target and a [B,1,H,W] weight, zero-element inputs.  Non-contiguous inputs are made
contiguous in torch before the fused function, so their adjoint is torch's.
"""
import numbers

import numpy as np
import torch
from torch.autograd.function import once_differentiable

from . import _lib, ops, optim, tables

CHUNK = 4096  # elements per chunk == DVC_LOSS_CHUNK of include/dvc_hip.h (tests/test_losses_host.py holds the two together)
TERM_DTYPE = np.dtype(_lib.DvcLossTerm)
CHUNK_DTYPE = np.dtype(_lib.DvcLossChunk)
KINDS = {"mse": 2, "l1": 1}
assert CHUNK == optim.CHUNK and CHUNK_DTYPE.itemsize == optim.CHUNK_DTYPE.itemsize      # one chunk table serves both


def chunk_table(counts):
    """dvc_amd.optim.chunk_table under DvcLossChunk's field names: chunk j of term k is {term: k, start: j * CHUNK}, terms in order;
    every element of every term lies in exactly one chunk and no chunk crosses a term."""
    return optim.chunk_table(counts).view(CHUNK_DTYPE)


def build_tables(entries):
    """The two tables of one call from `entries`, one (x, t, w, dx, dt, n, plane, cpl, p, t_scalar, scale) per term: five addresses
    (0 for an absent t, w, dx, dt), the element count, the broadcast geometry of w (plane 1 and cpl 0 when w is absent or has x's
    shape), the power, the scalar target and the scale.  Returns (TERM_DTYPE array, CHUNK_DTYPE array).  Needs no device."""
    terms = np.array([(x, t, w, dx, dt, n, plane, cpl, p, 0, ts, sc) for x, t, w, dx, dt, n, plane, cpl, p, ts, sc in entries],
                     dtype=TERM_DTYPE)
    return terms.reshape(-1), chunk_table([e[5] for e in entries])


# ---- what a term is: checked without a device
class _Term:
    __slots__ = ("p", "scale", "x", "t", "t_scalar", "w", "plane", "cpl")


def _check_term(where, kind, x, target, weights, scale):
    """-> _Term; every refusal that needs no device, in the order type, dtype, weights' grad, shapes, size, device."""
    if kind not in KINDS:
        raise ValueError(f"{where}: kind must be 'mse' or 'l1' (got {kind!r})")
    if not isinstance(x, torch.Tensor):
        raise TypeError(f"{where}: input must be a tensor (got {type(x).__name__})")
    if not isinstance(scale, numbers.Real) or isinstance(scale, bool):
        raise TypeError(f"{where}: scale must be a Python number (got {type(scale).__name__})")
    tensors = [("input", x)]
    if isinstance(target, torch.Tensor):
        tensors.append(("target", target))
    elif not isinstance(target, numbers.Real) or isinstance(target, bool):
        raise TypeError(f"{where}: target must be a tensor of input's shape or a Python number (got {type(target).__name__})")
    if weights is not None:
        if not isinstance(weights, torch.Tensor):
            raise TypeError(f"{where}: weights must be a tensor or None (got {type(weights).__name__})")
        tensors.append(("weights", weights))
    for name, v in tensors:
        if v.dtype != torch.float32:
            raise TypeError(f"{where}: {name} must be float32 (got {v.dtype})")
    if weights is not None and weights.requires_grad and torch.is_grad_enabled():
        raise NotImplementedError(f"{where}: weights that require grad are not supported (the mask is data in train.py); detach them")
    if isinstance(target, torch.Tensor) and target.shape != x.shape:
        raise NotImplementedError(f"{where}: broadcasting a target of shape {tuple(target.shape)} against an input of shape "
                                  f"{tuple(x.shape)} is not implemented; the target has input's shape or is a Python number")
    T = _Term()
    T.plane, T.cpl = 1, 0
    if weights is not None and weights.shape != x.shape:
        if not (x.dim() == 4 and weights.dim() == 4 and weights.shape[1] == 1
                and (weights.shape[0],) + tuple(weights.shape[2:]) == (x.shape[0],) + tuple(x.shape[2:])):
            raise NotImplementedError(f"{where}: broadcasting weights of shape {tuple(weights.shape)} against an input of shape "
                                      f"{tuple(x.shape)} is not implemented; weights have input's shape or are [B,1,H,W] for a "
                                      "[B,C,H,W] input")
        T.plane = x.shape[2] * x.shape[3]
        T.cpl = x.shape[1] * T.plane
    if x.numel() == 0:
        raise ValueError(f"{where}: the input has no elements (shape {tuple(x.shape)}); torch's mean of it would be NaN")
    dev = None
    for name, v in tensors:
        if not v.is_cuda:
            raise RuntimeError(f"{where}: {name} must be a ROCm device tensor; the HIP reduction has no CPU fallback")
        if dev is None:
            dev = v.device
        elif v.device != dev:
            raise RuntimeError(f"{where}: {name} lives on {v.device} but input on {dev}")
    T.p, T.scale = KINDS[kind], float(scale)
    T.x = x
    T.t = target if isinstance(target, torch.Tensor) else None
    T.t_scalar = 0.0 if T.t is not None else float(target)
    T.w = weights
    return T


# ---- one call: tables through the staging buffers, one copy, the launch(es)
_staging = {}       # device index -> optim._Staging
_refuse_capture = optim._refuse_capture     # (where): "... its tables carry the tensors' addresses ..."


def _send(entries, device):
    """Write the tables of `entries` into the next staging buffer and copy them to the device on the current stream.
    -> (device table, its host copy, bytes of the term table, number of chunks)"""
    st = _staging.get(device.index)
    if st is None:
        st = _staging[device.index] = optim._Staging()
    terms = np.array([e[:9] + (0,) + e[9:] for e in entries], dtype=TERM_DTYPE)
    table, host, n_c = optim._send(st, terms, tuple(e[5] for e in entries), device)      # (one chunk table serves both: above)
    return table, host, terms.nbytes, n_c


def _ptr(t):
    return 0 if t is None else t.data_ptr()


class _Fused(torch.autograd.Function):
    """(spec, *tensors) -> (total, values).  spec: per term (p, scale, t_scalar, has_t, has_w, plane, cpl); tensors: per term x, then
    t and w where present.  One ops.loss_fwd forward, one ops.loss_bwd backward."""

    @staticmethod
    def forward(ctx, spec, *tensors):
        _refuse_capture("dvc_amd.losses.fused")
        entries, it = [], iter(tensors)
        for p, scale, t_scalar, has_t, has_w, plane, cpl in spec:
            x = next(it)
            t = next(it) if has_t else None
            w = next(it) if has_w else None
            entries.append((x.data_ptr(), _ptr(t), _ptr(w), 0, 0, x.numel(), plane, cpl, p, t_scalar, scale))
        n = len(spec)
        device = tensors[0].device
        table, host, t_bytes, n_c = _send(entries, device)
        partials = torch.empty(n_c, dtype=torch.float64, device=device)
        out = torch.empty(n + 1, dtype=torch.float32, device=device)
        ops.loss_fwd(table, host, n, table[t_bytes:], n_c, partials, out)
        ctx.spec = spec
        ctx.save_for_backward(*tensors)
        ctx.set_materialize_grads(False)
        return out[n], out[:n]

    @staticmethod
    @once_differentiable
    def backward(ctx, g_total, g_values):
        _refuse_capture("the backward of dvc_amd.losses.fused")
        tensors, need = ctx.saved_tensors, ctx.needs_input_grad[1:]
        grads = [None] * len(tensors)
        if g_total is None and g_values is None:
            return (None, *grads)
        device = tensors[0].device
        g_total = torch.zeros(1, dtype=torch.float32, device=device) if g_total is None else g_total.contiguous()
        g_values = None if g_values is None else g_values.contiguous()
        entries, i = [], 0
        for p, scale, t_scalar, has_t, has_w, plane, cpl in ctx.spec:
            x, ix = tensors[i], i
            i += 1
            t = w = None
            if has_t:
                t, it_ = tensors[i], i
                i += 1
                if need[it_]:
                    grads[it_] = torch.empty_like(t)
            if has_w:
                w = tensors[i]
                i += 1
            if need[ix]:
                grads[ix] = torch.empty_like(x)
            entries.append((x.data_ptr(), _ptr(t), _ptr(w), _ptr(grads[ix]), _ptr(grads[it_]) if has_t else 0, x.numel(), plane, cpl,
                            p, t_scalar, scale))
        table, host, t_bytes, n_c = _send(entries, device)
        ops.loss_bwd(table, host, len(entries), table[t_bytes:], n_c, g_total, g_values)
        return (None, *grads)


def _checked_terms(where, terms, shape, row):
    """The checks `fused` and `Plan` share, in their order: a non-empty list of 5-tuples (`shape` is how the message spells one);
    per term `row(at, *term)` -> (its spec row, its tensors, None for an absent one), which refuses what it refuses; the tensors
    made contiguous; all of them on the current device.  -> (spec tuple, tensor list)"""
    terms = list(terms)
    if not terms:
        raise ValueError(f"{where}: no terms")
    for k, term in enumerate(terms):
        if not isinstance(term, (tuple, list)) or len(term) != 5:
            raise ValueError(f"{where}: term {k} is not {shape}")
    spec, tensors = [], []
    for k, term in enumerate(terms):
        one, used = row(f"{where}: term {k}", *term)
        spec.append(one)
        tensors += [v.contiguous() for v in used if v is not None]      # (a no-op for a contiguous tensor)
    dev = ops._current_device()
    for v in tensors:
        if v.device.index != dev:
            raise RuntimeError(f"{where}: a tensor lives on {v.device} but the current device is cuda:{dev}; call "
                               "torch.cuda.set_device / use torch.cuda.device(...)")
    return tuple(spec), tensors


def _fused_row(at, *term):
    T = _check_term(at, *term)
    return (T.p, T.scale, T.t_scalar, T.t is not None, T.w is not None, T.plane, T.cpl), (T.x, T.t, T.w)


def fused(terms):
    """terms: a list of (kind, input, target, weights_or_None, scale), kind in {"mse", "l1"} -> (total, values): the 0-dim sum of the
    terms and the [len(terms)] tensor of the terms, scale_k * mean(w * |input - target|^p), both differentiable in every input and
    target that requires grad.  One forward call and one backward call of the library serve every term."""
    spec, tensors = _checked_terms("dvc_amd.losses.fused", terms, "(kind, input, target, weights_or_None, scale)", _fused_row)
    _refuse_capture("dvc_amd.losses.fused")
    return _Fused.apply(spec, *tensors)


def _one(kind, input, target, weights):
    # the total of a one-row table is (float)(0.0 + v): the bits of values[0]
    return fused([(kind, input, target, weights, 1.0)])[0]


def mse_loss(input, target=0):
    """torch.mean((input - target) ** 2) — utils/util.py's mse_loss."""
    return _one("mse", input, target, None)


def l1_loss(input, target=0):
    """torch.mean(torch.abs(input - target)) — utils/util.py's l1_loss."""
    return _one("l1", input, target, None)


def weighted_mse_loss(input, target, weights):
    """((input - target) ** 2 * weights.expand_as(input)).mean() — utils/util.py's weighted_mse_loss."""
    return _one("mse", input, target, weights)


def weighted_l1_loss(input, target, weights):
    """(torch.abs(input - target) * weights.expand_as(input)).mean() — utils/util.py's weighted_l1_loss."""
    return _one("l1", input, target, weights)


# ---- plans: resident tables, replayable, with the signed mean and the relativistic GAN term (csrc/loss_plan.hip)
PLAN_TERM_DTYPE = np.dtype(_lib.DvcPlanTerm)
PLAN_KINDS = {"l1": 1, "mse": 2, "mean": 3, "rel": 4}       # == DVC_LOSS_KIND_* of include/dvc_hip.h
_PLAN_P = {1: 1, 2: 2, 3: 1, 4: 2}
_REL = PLAN_KINDS["rel"]
HINT_CHUNKS = 4096      # chunk records a spare sized from `n_terms_hint` has room for: 16 Mi elements over all terms


def build_plan_tables(entries):
    """The tables of one direction of a plan from `entries`, one (kind, x, t, w, dx, dt, n, plane, cpl, t_scalar, scale, y, dy, n_y,
    c) per term: the kind number, five addresses, the count and geometry of a DvcLossTerm, the two scalars, and for a relativistic
    term the addresses of y and dy, y's count and the constant (0 otherwise).  -> (PLAN_TERM_DTYPE array, CHUNK_DTYPE array, n_c,
    n_yc): the chunk table holds the n_c chunks of every x, then the n_yc chunks of every relativistic term's y, both in term order
    with the term's index in the plan; relativistic terms take the scratch slots 0, 1, ... in order.  Needs no device."""
    terms = np.zeros(len(entries), dtype=PLAN_TERM_DTYPE)
    slot = 0
    for i, (kind, x, t, w, dx, dt, n, plane, cpl, ts, sc, y, dy, n_y, c) in enumerate(entries):
        terms[i] = (x, t, w, dx, dt, n, plane, cpl, _PLAN_P.get(kind, 0), kind, ts, sc, y, dy, n_y, c, slot if kind == _REL else 0)
        slot += kind == _REL
    xc = chunk_table([e[6] for e in entries])
    yc = chunk_table([e[13] if e[0] == _REL else 0 for e in entries])
    return terms, np.concatenate([xc, yc]), len(xc), len(yc)


def plan_fingerprint(entries):
    """What a plan's resident tables were built from: per term its kind, addresses, counts, geometry and scalars — the entries
    themselves, as a tuple.  Equal fingerprints <=> the tables a rebuild would write are the ones already on the device."""
    return tuple(tuple(e) for e in entries)


def _check_rel(where, x, y, c, scale):
    """The refusals of a ("rel", x, y, c, scale) term that need no device, then the device ones; -> (x, y, float(c), float(scale))."""
    if not isinstance(x, torch.Tensor):
        raise TypeError(f"{where}: input must be a tensor (got {type(x).__name__})")
    if not isinstance(scale, numbers.Real) or isinstance(scale, bool):
        raise TypeError(f"{where}: scale must be a Python number (got {type(scale).__name__})")
    if not isinstance(c, numbers.Real) or isinstance(c, bool):
        raise TypeError(f"{where}: c must be a Python number (got {type(c).__name__}); the term is (\"rel\", x, y, c, scale)")
    if not isinstance(y, torch.Tensor):
        raise TypeError(f"{where}: y must be a float32 device tensor (got {type(y).__name__})")
    for name, v in (("input", x), ("y", y)):
        if v.dtype != torch.float32:
            raise TypeError(f"{where}: {name} must be float32 (got {v.dtype})")
    if x.numel() == 0:
        raise ValueError(f"{where}: the input has no elements (shape {tuple(x.shape)}); torch's mean of it would be NaN")
    if y.numel() == 0:
        raise ValueError(f"{where}: y has no elements (shape {tuple(y.shape)}); torch's mean of it would be NaN")
    for name, v in (("input", x), ("y", y)):
        if not v.is_cuda:
            raise RuntimeError(f"{where}: {name} must be a ROCm device tensor; the HIP reduction has no CPU fallback")
    if y.device != x.device:
        raise RuntimeError(f"{where}: y lives on {y.device} but input on {x.device}")
    return x, y, float(c), float(scale)


def _plan_row(at, kind, a, b, c, scale):
    if not isinstance(kind, str) or kind not in PLAN_KINDS:
        raise ValueError(f"{at}: kind must be one of 'l1', 'mse', 'mean', 'rel' (got {kind!r})")
    if kind == "rel":
        x, y, cc, sc = _check_rel(at, a, b, c, scale)
        return (_REL, sc, 0.0, False, False, 1, 0, cc), (x, y)
    T = _check_term(at, "l1" if kind == "mean" else kind, a, b, c, scale)
    return (PLAN_KINDS[kind], T.scale, T.t_scalar, T.t is not None, T.w is not None, T.plane, T.cpl, 0.0), (T.x, T.t, T.w)


class _PlanResident(tables.Resident):
    """One direction's tables on the device ([term records | chunk records | scratch]) and what they were built from."""
    __slots__ = ("n", "n_c", "n_yc", "terms", "chunks", "scratch")

    def __init__(self, key, table, c_at, end, n, n_c, n_yc, pinned, stream):
        super().__init__(key, table, pinned, stream)
        self.n, self.n_c, self.n_yc = n, n_c, n_yc
        self.terms, self.chunks = table[:c_at], table[c_at:end]
        self.scratch = table[end:].view(torch.float64)      # (the forward's; empty for the backward's tables)


class _PlanFn(torch.autograd.Function):
    """(plan, spec, *tensors) -> (total, values).  spec: per term (kind, scale, t_scalar, has_t, has_w, plane, cpl, c); tensors: per
    term x, then t and w where present, or x and y for a relativistic term.  One ops.loss_plan_fwd, one ops.loss_plan_bwd."""

    @staticmethod
    def forward(ctx, plan, spec, *tensors):
        entries, it = [], iter(tensors)
        for kind, scale, t_scalar, has_t, has_w, plane, cpl, c in spec:
            x = next(it)
            if kind == _REL:
                y = next(it)
                entries.append((kind, x.data_ptr(), 0, 0, 0, 0, x.numel(), 1, 0, 0.0, scale, y.data_ptr(), 0, y.numel(), c))
            else:
                t = next(it) if has_t else None
                w = next(it) if has_w else None
                entries.append((kind, x.data_ptr(), _ptr(t), _ptr(w), 0, 0, x.numel(), plane, cpl, t_scalar, scale, 0, 0, 0, 0.0))
        n, device = len(spec), tensors[0].device
        res = plan._tables(0, entries, device)
        out = torch.empty(n + 1, dtype=torch.float32, device=device)
        ops.loss_plan_fwd(res.terms, n, res.chunks, res.n_c, res.n_yc, res.scratch, out)
        plan._generation += 1
        ctx.plan, ctx.spec, ctx.res, ctx.generation = plan, spec, res, plan._generation
        ctx.save_for_backward(*tensors)
        ctx.set_materialize_grads(False)
        return out[n], out[:n]

    @staticmethod
    @once_differentiable
    def backward(ctx, g_total, g_values):
        tensors, need = ctx.saved_tensors, ctx.needs_input_grad[2:]
        grads = [None] * len(tensors)
        if g_total is None and g_values is None:
            return (None, None, *grads)
        plan, fwd = ctx.plan, ctx.res
        if fwd.n_yc and plan._generation != ctx.generation:
            raise RuntimeError("dvc_amd.losses.Plan: the plan was called again before this backward, and the sums a relativistic "
                               "term's backward reads from the plan's scratch are the later call's; use one Plan per call site")
        device = tensors[0].device
        g_total = torch.zeros(1, dtype=torch.float32, device=device) if g_total is None else g_total.contiguous()
        g_values = None if g_values is None else g_values.contiguous()
        entries, i = [], 0
        for kind, scale, t_scalar, has_t, has_w, plane, cpl, c in ctx.spec:
            x, ix = tensors[i], i
            i += 1
            if need[ix]:
                grads[ix] = torch.empty_like(x)
            if kind == _REL:
                y, iy = tensors[i], i
                i += 1
                if need[iy]:
                    grads[iy] = torch.empty_like(y)
                entries.append((kind, x.data_ptr(), 0, 0, _ptr(grads[ix]), 0, x.numel(), 1, 0, 0.0, scale, y.data_ptr(),
                                _ptr(grads[iy]), y.numel(), c))
                continue
            t = w = None
            dt = 0
            if has_t:
                t = tensors[i]
                if need[i]:
                    grads[i] = torch.empty_like(t)
                    dt = grads[i].data_ptr()
                i += 1
            if has_w:
                w = tensors[i]
                i += 1
            entries.append((kind, x.data_ptr(), _ptr(t), _ptr(w), _ptr(grads[ix]), dt, x.numel(), plane, cpl, t_scalar, scale,
                            0, 0, 0, 0.0))
        res = plan._tables(1, entries, device)
        ops.loss_plan_bwd(res.terms, res.n, res.chunks, res.n_c, res.n_yc, fwd.scratch, g_total, g_values)
        return (None, None, *grads)


class Plan:
    """A list of loss terms on tables that stay on the device: `total, values = plan(terms)` with `fused`'s return contract, where a
    term is (kind, input, target, weights_or_None, scale) with kind in {"l1", "mse", "mean"} or ("rel", x, y, c, scale):

      "l1", "mse"   scale * mean(w * |input - target|^p), with `fused`'s bits;
      "mean"        scale * mean(w * (input - target)), signed; target and weights as for "l1";
      "rel"         scale * mean(((x - mean(y)) - c)^2), the relativistic GAN term; x and y float32 device tensors of any shapes
                    and sizes, both differentiable, c a Python number.

    A call checks the terms as `fused` does (the same refusals by the same exception types; an unknown kind, a non-number c and a
    y that is not a float32 device tensor or has no elements are refused too) and fingerprints kinds, addresses, counts, geometry
    and scalars (`plan_fingerprint`).  If nothing moved since the tables were uploaded the forward is its launches and one
    allocation, the outputs: no numpy, no copy.  The backward works the same way against tables of its own, which also carry the
    dx / dt / dy addresses — it hits when the allocator hands the gradients the addresses of the step before.  If something moved,
    that direction's tables are rebuilt, checked by dvc_loss_plan_check, and sent with one copy from a pinned buffer under
    tables.Staging's discipline.  `uploads` counts those copies.

    A call works under `torch.cuda.graph`; the rule is CapturableAdam's and the tables are kept as dvc_amd.tables says.  Pinned
    memory is never allocated during a capture: two spares are kept, sized from `n_terms_hint` (room for that many terms and
    HINT_CHUNKS chunks) or from the first eager call; without one a captured call raises a RuntimeError that says to call the plan
    eagerly once.  A replay recomputes from whatever the SAME tensors then hold.

    The sum a relativistic term's backward needs is left in the plan's scratch by the forward, so the backward of a call must run
    before the plan is called again (it raises otherwise): one Plan per call site — one for the discriminator step, one for the
    generator step.  Non-contiguous inputs are made contiguous in torch first, which moves them on every call."""

    def __init__(self, n_terms_hint=None):
        if n_terms_hint is not None and (not isinstance(n_terms_hint, numbers.Integral) or isinstance(n_terms_hint, bool)
                                         or n_terms_hint < 1):
            raise ValueError(f"dvc_amd.losses.Plan: n_terms_hint must be a positive integer or None (got {n_terms_hint!r})")
        self._staging = optim._Staging()
        self._resident = [None, None]       # forward, backward
        self._captured = []                 # tables a graph refers to: alive as long as the plan
        self._spares = []                   # pinned buffers for uploads that are themselves captured
        self._spare_bytes = 0
        self._generation = 0
        self.uploads = 0
        if n_terms_hint is not None:
            self._spare_bytes = int(n_terms_hint) * PLAN_TERM_DTYPE.itemsize + HINT_CHUNKS * CHUNK_DTYPE.itemsize
            self._ensure_spares()

    def _ensure_spares(self):
        """Two pinned buffers (a capture may upload both directions), allocated OUTSIDE any capture."""
        if not self._spare_bytes or not torch.cuda.is_available() or torch.cuda.is_current_stream_capturing():
            return
        self._spares = [s for s in self._spares if s.numel() >= self._spare_bytes]
        while len(self._spares) < 2:
            self._spares.append(torch.empty(self._spare_bytes, dtype=torch.uint8, pin_memory=True))

    def _tables(self, which, entries, device):
        """The resident tables of direction `which` for `entries`: the ones on the device if the fingerprint is theirs, else rebuilt."""
        key = plan_fingerprint(entries)
        capturing = torch.cuda.is_current_stream_capturing()
        res = self._resident[which]
        if res is None or res.key != key or res.table.device != device:
            res = self._upload(which, key, entries, device, capturing)
        res.use(self._captured, capturing, ops._stream_handle())
        if not capturing and len(self._spares) < 2:
            self._ensure_spares()
        return res

    def _upload(self, which, key, entries, device, capturing):
        """Rebuild one direction's tables, check them, and send them to a fresh table tensor with one host-to-device copy."""
        terms, chunks, n_c, n_yc = build_plan_tables(entries)
        ops.loss_plan_check(terms, n_c, n_yc)
        nbytes = terms.nbytes + chunks.nbytes
        if capturing:       # a buffer of its own, never rewritten: the replay's copy node reads it again
            pinned = next((s for s in self._spares if s.numel() >= nbytes), None)
            if pinned is None:
                raise RuntimeError("dvc_amd.losses.Plan: the tables have to be uploaded and the stream is capturing, but no pinned "
                                   "buffer of their size was set aside (pinned memory is not allocated during a capture); call the "
                                   "plan eagerly once with these terms before the capture, or pass n_terms_hint")
            self._spares.remove(pinned)
        else:
            slot = self._staging.acquire(nbytes)
            pinned = self._staging.buf[slot]
            self._spare_bytes = max(self._spare_bytes, nbytes)
        (_, c_at), _ = tables.pack(pinned.numpy(), [terms, chunks])
        scratch = 8 * ops.loss_plan_scratch_doubles(len(terms), n_c, n_yc) if which == 0 else 0
        table = tables.upload(pinned, nbytes, device, scratch)
        if not capturing:
            self._staging.sent(slot)
        self.uploads += 1
        res = self._resident[which] = _PlanResident(key, table, c_at, nbytes, len(terms), n_c, n_yc, pinned if capturing else None,
                                                    ops._stream_handle())
        return res

    def __call__(self, terms):
        spec, tensors = _checked_terms("dvc_amd.losses.Plan", terms,
                                       "(kind, input, target, weights_or_None, scale) or (\"rel\", x, y, c, scale)", _plan_row)
        return _PlanFn.apply(self, spec, *tensors)


def relativistic_loss(x, y, c):
    """torch.mean((x - torch.mean(y) - c) ** 2) — one half of train.py's relativistic GAN objective — as a one-term Plan of its own
    (so: eager only, and tables uploaded on every call; a training step keeps a Plan)."""
    return Plan()([("rel", x, y, c, 1.0)])[0]
