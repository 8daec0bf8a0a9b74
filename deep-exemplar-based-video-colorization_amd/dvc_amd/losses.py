"""train.py's pixel losses on the package's own fused reduction: `mse_loss`, `l1_loss`, `weighted_mse_loss`, `weighted_l1_loss` with
the signatures of the reference's utils/util.py, and `fused(terms)`, which evaluates any number of such terms — every term is
scale * mean(w * |input - target|^p), p in {1, 2} — with ONE dvc_loss_fwd call forward and ONE dvc_loss_bwd call backward
(csrc/loss.hip; the design, the order of the sums and the error bound are in DESIGN.md §6d).

The four helpers are `fused` with a one-row table, and a term's value is bit-identical whether it is computed alone or inside any
`fused` call: the kernel's partial sums depend on the term's data alone.  Values and gradients are bit-reproducible from run to run.

Per call the host writes the term table and the chunk table into a pinned staging buffer, sends them with one host-to-device copy on
the current stream and launches; two staging buffers alternate, each behind an event recorded after its copy (dvc_amd.optim's
scheme, and its chunk table).  The tables carry addresses, so a call cannot be replayed from a captured graph: it raises while the
current stream is capturing.

What is not done is refused by name: CPU tensors (no CPU fallback), non-fp32, weights that require grad (the mask is data in
train.py), broadcasts other than a Python-number target and a [B,1,H,W] weight, zero-element inputs.  Non-contiguous inputs are made
contiguous in torch before the fused function, so their adjoint is torch's.
"""
import numbers

import numpy as np
import torch
from torch.autograd.function import once_differentiable

from . import _lib, ops, optim

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


def _send(entries, device):
    """Write the tables of `entries` into the next staging buffer and copy them to the device on the current stream.
    -> (device table, its host copy, bytes of the term table, number of chunks)"""
    st = _staging.get(device.index)
    if st is None:
        st = _staging[device.index] = optim._Staging()
    counts = tuple(e[5] for e in entries)
    n_c = sum((n + CHUNK - 1) // CHUNK for n in counts)
    t_bytes, c_bytes = len(entries) * TERM_DTYPE.itemsize, n_c * CHUNK_DTYPE.itemsize       # (80 n: the chunk table stays 16-byte aligned)
    nbytes = t_bytes + c_bytes
    slot = st.slot = 1 - st.slot
    if st.event[slot] is not None:
        st.event[slot].synchronize()        # the copy that last read this buffer (two calls ago) has run
    if st.buf[slot] is None or st.buf[slot].numel() < nbytes:
        st.buf[slot] = torch.empty(nbytes + nbytes // 4, dtype=torch.uint8, pin_memory=True)
        st.counts[slot] = None
    host = st.buf[slot].numpy()
    host[:t_bytes].view(TERM_DTYPE)[:] = np.array([e[:9] + (0,) + e[9:] for e in entries], dtype=TERM_DTYPE)
    if st.counts[slot] != counts:
        host[t_bytes:nbytes].view(CHUNK_DTYPE)[:] = chunk_table(counts)
        st.counts[slot] = counts
    table = torch.empty(nbytes, dtype=torch.uint8, device=device)       # (freed on return: the allocator reuses it in stream order)
    table.copy_(st.buf[slot][:nbytes], non_blocking=True)
    if st.event[slot] is None:
        st.event[slot] = torch.cuda.Event()
    st.event[slot].record()
    return table, st.buf[slot], t_bytes, n_c


def _refuse_capture(where):
    if torch.cuda.is_initialized() and torch.cuda.is_current_stream_capturing():        # before anything is allocated or launched
        raise RuntimeError(f"{where} cannot be captured into a graph: its tables carry the tensors' addresses and are launch-time "
                           "data; call it outside the capture")


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


def fused(terms):
    """terms: a list of (kind, input, target, weights_or_None, scale), kind in {"mse", "l1"} -> (total, values): the 0-dim sum of the
    terms and the [len(terms)] tensor of the terms, scale_k * mean(w * |input - target|^p), both differentiable in every input and
    target that requires grad.  One forward call and one backward call of the library serve every term."""
    terms = list(terms)
    if not terms:
        raise ValueError("dvc_amd.losses.fused: no terms")
    for k, term in enumerate(terms):
        if not isinstance(term, (tuple, list)) or len(term) != 5:
            raise ValueError(f"dvc_amd.losses.fused: term {k} is not (kind, input, target, weights_or_None, scale)")
    spec, tensors = [], []
    for k, term in enumerate(terms):
        T =_check_term(f"dvc_amd.losses.fused: term {k}", *term)
        spec.append((T.p, T.scale, T.t_scalar, T.t is not None, T.w is not None, T.plane, T.cpl))
        tensors += [v.contiguous() for v in (T.x, T.t, T.w) if v is not None]       # (a no-op for a contiguous tensor)
    dev = ops._current_device()
    for v in tensors:
        if v.device.index != dev:
            raise RuntimeError(f"dvc_amd.losses.fused: a tensor lives on {v.device} but the current device is cuda:{dev}; call "
                               "torch.cuda.set_device / use torch.cuda.device(...)")
    _refuse_capture("dvc_amd.losses.fused")
    return _Fused.apply(tuple(spec), *tensors)


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
