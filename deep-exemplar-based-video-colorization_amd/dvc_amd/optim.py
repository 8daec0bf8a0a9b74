"""Adam on the package's own kernel: `dvc_amd.optim.Adam` is a drop-in for `torch.optim.Adam` whose `step()` updates every
parameter of every group in ONE launch of dvc_adam_step (csrc/optim.hip; the design is DESIGN.md §6d).

Same constructor, same lazily created state ({"step", "exp_avg", "exp_avg_sq"[, "max_exp_avg_sq"]}, `step` a CPU float32 scalar
per parameter), and a `state_dict()` that `torch.optim.Adam` loads and vice versa; LR schedulers, `add_param_group` and
`zero_grad` are the base class's.  What it does not do it refuses by name: maximize, capturable, differentiable,
decoupled_weight_decay, foreach=True, fused=True, tensor hyper-parameters, CPU / non-fp32 / sparse / non-contiguous tensors.

Per step the host evaluates each tensor's scalars in double (per TENSOR: torch keeps `step` per parameter, and groups differ in
`lr`), packs the tensor and chunk tables into a pinned staging buffer, sends them with one host-to-device copy on the current
stream and launches once; the staging discipline (and the resident tables' below) is dvc_amd.tables', described there once.
The scalars change every step, so a step cannot be replayed from a captured graph: `step()` raises while the stream is capturing.

`CapturableAdam` (below) is the variant that can: torch's `capturable=True` contract.  Its `step` tensors live on the device, a
second small launch (dvc_adam_advance) advances them and rewrites the two step-dependent columns of the tensor table there, and the
tables stay resident between steps, so a step whose addresses did not move is two launches and nothing else — eagerly or replayed.

`GuardedAdam` (at the bottom) is `CapturableAdam` with a look at its gradients first: dvc_grad_norm reduces their global L2 norm
into a small device record, and the guarded advance and step obey it — clip_grad_norm_'s coefficient goes into the step as one
multiply of g, and a NaN or Inf anywhere skips the whole step, count and all.  Four launches, no host code between them.
`grad_norm` and `clip_grad_norm_` are the same reduction as stand-alone functions (torch.nn.utils.clip_grad_norm_'s signature).
"""
import math

import numpy as np
import torch
from torch.optim.optimizer import Optimizer

from . import _lib, ops, tables

CHUNK = 4096  # elements per chunk == DVC_ADAM_CHUNK of include/dvc_hip.h (tests/test_adam_host.py holds the two together)
TENSOR_DTYPE = np.dtype(_lib.DvcAdamTensor)
CHUNK_DTYPE = np.dtype(_lib.DvcAdamChunk)
ADVANCE_DTYPE = np.dtype(_lib.DvcAdamAdvance)      # (CapturableAdam's third table)
GUARD_DTYPE = np.dtype(_lib.DvcGradGuard)          # (GuardedAdam's device record)
_REFUSED_FLAGS = ("maximize", "capturable", "differentiable", "decoupled_weight_decay")
_Staging = tables.Staging       # (the name dvc_amd.losses and the tests know it by)


def adam_scalars(step, lr, beta1, beta2, eps, weight_decay):
    """The per-tensor scalars of step number `step` (>= 1), evaluated in double, in the order of DvcAdamTensor's float fields;
    each is rounded once, to fp32, when it is stored in the table."""
    bc1 = 1.0 - beta1 ** step
    bc2 = 1.0 - beta2 ** step
    return (lr / bc1, 1.0 / math.sqrt(bc2), beta2, 1.0 - beta1, 1.0 - beta2, eps, weight_decay, 0.0)


def n_chunks(counts):
    """The number of records of chunk_table(counts), without building it."""
    return sum((n + CHUNK - 1) // CHUNK for n in counts)


def chunk_table(counts):
    """Cut tensors of `counts` elements into chunks of at most CHUNK: a CHUNK_DTYPE array with chunk k of tensor i as
    {tensor: i, start: k * CHUNK}, tensors in order.  Every element of every tensor lies in exactly one chunk, no chunk crosses a
    tensor, and a tensor of 0 elements gets none."""
    counts = np.asarray(counts, dtype=np.int64).reshape(-1)
    if (counts < 0).any():
        raise ValueError(f"dvc_amd.optim: negative element count in {counts.tolist()}")
    per = (counts + (CHUNK - 1)) // CHUNK
    out = np.zeros(int(per.sum()), dtype=CHUNK_DTYPE)
    out["tensor"] = np.repeat(np.arange(len(counts), dtype=np.int32), per)
    out["start"] = (np.arange(len(out), dtype=np.int64) - np.repeat(np.cumsum(per) - per, per)) * CHUNK
    return out


def build_tables(entries):
    """The two tables of one launch from `entries`, one (p, g, m, v, vmax, n, scalars) per tensor: five addresses (vmax 0 without
    amsgrad), the element count and adam_scalars(...).  Returns (TENSOR_DTYPE array, CHUNK_DTYPE array).  Needs no device: the
    16-byte path is chosen per chunk by the kernel from the addresses themselves."""
    tensors = np.array([(p, g, m, v, vmax, n) + tuple(sc) for p, g, m, v, vmax, n, sc in entries], dtype=TENSOR_DTYPE)
    return tensors.reshape(-1), chunk_table([e[5] for e in entries])


def vector_path(*addresses):
    """Whether a chunk of a tensor with these p, g, m, v (and vmax) addresses moves as 16-byte vectors (the kernel's predicate; a
    chunk starts a multiple of CHUNK elements into its tensor, so the tensor's base addresses decide)."""
    return all(a % 16 == 0 for a in addresses)


def _capturing():
    return torch.cuda.is_initialized() and torch.cuda.is_current_stream_capturing()


def _refuse_capture(where, whose="tensors", advice=""):
    """For calls whose tables are launch-time data: raise while the stream is capturing, before anything is allocated or launched."""
    if _capturing():
        raise RuntimeError(f"{where} cannot be captured into a graph: its tables carry the {whose}' addresses and are launch-time "
                           f"data; call it outside the capture{advice}")


def _send(st, records, counts, device):
    """[records | chunk_table(counts)] through `st`'s next buffer into a table tensor that lives for one call (freed on return,
    the allocator reuses it in stream order).  The chunk table is built only if the buffer does not already hold the one of
    `counts`.  -> (table, the pinned buffer it was sent from, number of chunks)"""
    n_c = n_chunks(counts)
    c_bytes = n_c * CHUNK_DTYPE.itemsize
    slot = st.acquire(records.nbytes + c_bytes)
    if st.counts[slot] == counts:
        tables.pack(st.buf[slot].numpy(), [records], tail_bytes=c_bytes)
    else:
        tables.pack(st.buf[slot].numpy(), [records, chunk_table(counts)])
        st.counts[slot] = counts
    table = tables.upload(st.buf[slot], records.nbytes + c_bytes, device)
    st.sent(slot)
    return table, st.buf[slot], n_c


class Adam(Optimizer):
    """torch.optim.Adam on one HIP launch per step.  See the module docstring."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, amsgrad=False, *, foreach=None,
                 maximize=False, capturable=False, differentiable=False, fused=None, decoupled_weight_decay=False,
                 max_grad_norm=None, skip_nonfinite=None):
        if not self._guarded and (max_grad_norm is not None or skip_nonfinite is not None):
            raise NotImplementedError(f"{self._name}: `max_grad_norm` / `skip_nonfinite` are not supported by this step; use "
                                      "dvc_amd.optim.GuardedAdam")
        if isinstance(lr, torch.Tensor):
            if not self._capturable:
                raise NotImplementedError("dvc_amd.optim.Adam: a tensor `lr` is not supported (the step's scalars are evaluated on "
                                          "the host); pass a float, or use dvc_amd.optim.CapturableAdam")
            if lr.numel() != 1 or lr.dtype != torch.float32:
                raise ValueError(f"{self._name}: a tensor `lr` must be a one-element float32 tensor")
        if any(isinstance(b, torch.Tensor) for b in betas):
            raise NotImplementedError(f"{self._name}: tensor `betas` are not supported; pass floats")
        for name, value in (("maximize", maximize), ("capturable", capturable and not self._capturable),
                            ("differentiable", differentiable), ("decoupled_weight_decay", decoupled_weight_decay),
                            ("foreach", foreach), ("fused", fused)):
            if value:
                raise NotImplementedError(f"{self._name}: `{name}=True` is not supported by the HIP step"
                                          + ("; use dvc_amd.optim.CapturableAdam" if name == "capturable" else ""))
        if not isinstance(lr, torch.Tensor) and not 0.0 <= lr:         # (a tensor lr lives on the device and is never read back)
            raise ValueError(f"Invalid learning rate: {lr}")
        if not 0.0 <= eps:
            raise ValueError(f"Invalid epsilon value: {eps}")
        if not 0.0 <= betas[0] < 1.0:
            raise ValueError(f"Invalid beta parameter at index 0: {betas[0]}")
        if not 0.0 <= betas[1] < 1.0:
            raise ValueError(f"Invalid beta parameter at index 1: {betas[1]}")
        if not 0.0 <= weight_decay:
            raise ValueError(f"Invalid weight_decay value: {weight_decay}")
        # the keys torch.optim.Adam keeps in a group, so that either class loads the other's state_dict
        defaults = dict(lr=lr, betas=tuple(betas), eps=eps, weight_decay=weight_decay, amsgrad=amsgrad, maximize=False,
                        foreach=None, capturable=self._capturable, differentiable=False, fused=None, decoupled_weight_decay=False)
        super().__init__(params, defaults)

    def __setstate__(self, state):
        super().__setstate__(state)
        for group in self.param_groups:
            group.setdefault("amsgrad", False)
            for name in _REFUSED_FLAGS:
                group.setdefault(name, False)
            group.setdefault("foreach", None)
            group.setdefault("fused", None)
            for p in group["params"]:
                st = self.state.get(p, {})
                if len(st) and not torch.is_tensor(st["step"]):
                    st["step"] = torch.tensor(float(st["step"]), dtype=torch.float32)

    # ---- what CapturableAdam answers differently
    _name = "dvc_amd.optim.Adam"
    _capturable = False
    _guarded = False
    _refused_flags = _REFUSED_FLAGS

    def _check_group(self, group):
        if isinstance(group["lr"], torch.Tensor) or any(isinstance(b, torch.Tensor) for b in group["betas"]):
            raise NotImplementedError(f"{self._name}: a tensor `lr` / `betas` is not supported; pass floats")

    def _new_step(self, p):
        return torch.tensor(0.0, dtype=torch.float32)

    # ---- one step
    def _collect(self):
        """Validate everything and create missing state; nothing is advanced.  -> [(group, p, grad, state)]"""
        work = []
        for group in self.param_groups:
            for name in self._refused_flags:
                if group.get(name):
                    raise NotImplementedError(f"{self._name}: `{name}=True` is not supported by the HIP step")
            self._check_group(group)
            for p in group["params"]:
                grad = p.grad
                if grad is None:
                    continue
                if grad.is_sparse:
                    raise RuntimeError("Adam does not support sparse gradients, please consider SparseAdam instead")
                if not p.is_cuda or not grad.is_cuda:
                    raise RuntimeError(f"{self._name}: parameters and gradients must be ROCm device tensors; the HIP step has "
                                       "no CPU fallback")
                if p.dtype != torch.float32 or grad.dtype != torch.float32:
                    raise TypeError(f"{self._name}: parameters and gradients must be float32 (got {p.dtype}, {grad.dtype})")
                if not p.is_contiguous():
                    raise ValueError(f"{self._name}: a parameter of shape {tuple(p.shape)} and strides {p.stride()} is not "
                                     "contiguous")
                if grad.shape != p.shape:
                    raise ValueError(f"{self._name}: gradient shape {tuple(grad.shape)} != parameter {tuple(p.shape)}")
                state = self.state[p]
                if len(state) == 0:
                    state["step"] = self._new_step(p)
                    state["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                    state["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                    if group["amsgrad"]:
                        state["max_exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                elif group["amsgrad"] and "max_exp_avg_sq" not in state:
                    raise RuntimeError(f"{self._name}: amsgrad was switched on for a parameter whose state has no max_exp_avg_sq")
                for key in ("exp_avg", "exp_avg_sq") + (("max_exp_avg_sq",) if group["amsgrad"] else ()):
                    s = state[key]
                    if not s.is_cuda:
                        raise RuntimeError(f"{self._name}: state `{key}` is a CPU tensor; the HIP step has no CPU fallback")
                    if s.dtype != torch.float32:
                        raise TypeError(f"{self._name}: state `{key}` must be float32 (got {s.dtype})")
                    if not s.is_contiguous() or s.numel() != p.numel():
                        raise ValueError(f"{self._name}: state `{key}` must be contiguous with {p.numel()} elements")
                work.append((group, p, grad, state))
        if work:
            dev = ops._current_device()
            for _, p, grad, state in work:
                for t in (p, grad, state["exp_avg"], state["exp_avg_sq"], state.get("max_exp_avg_sq")):
                    if t is not None and t.device.index != dev:
                        raise RuntimeError(f"{self._name}: a tensor lives on {t.device} but the current device is cuda:{dev}; "
                                           "call torch.cuda.set_device / use torch.cuda.device(...)")
        return work

    @torch.no_grad()
    def step(self, closure=None):
        if _capturing():        # before anything is allocated or launched
            raise RuntimeError("dvc_amd.optim.Adam: step() cannot be captured into a graph: its scalars (the bias corrections of "
                               "step t) change every step and are launch-time table entries; step outside the capture, or use "
                               "dvc_amd.optim.CapturableAdam")
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        work = self._collect()
        entries, updated, memo = [], [], {}
        for group, p, grad, state in work:
            step_t = state["step"]
            if step_t.device.type != "cpu" or step_t.dtype != torch.float32:    # (a state_dict of a fused / capturable torch.optim.Adam)
                step_t = state["step"] = step_t.detach().to(device="cpu", dtype=torch.float32)
            step_t += 1
            if p.numel() == 0:
                continue
            beta1, beta2 = group["betas"]
            key = (step_t.item(), group["lr"], beta1, beta2, group["eps"], group["weight_decay"])
            sc = memo.get(key)
            if sc is None:
                sc = memo[key] = adam_scalars(*key)
            if not grad.is_contiguous():
                grad = grad.contiguous()
            vmax = state["max_exp_avg_sq"] if group["amsgrad"] else None
            entries.append((p.data_ptr(), grad.data_ptr(), state["exp_avg"].data_ptr(), state["exp_avg_sq"].data_ptr(),
                            0 if vmax is None else vmax.data_ptr(), p.numel(), sc))
            updated.append((p, grad))       # (holds a contiguous copy of a gradient until the launch is enqueued)
        if entries:
            self._launch(entries, updated[0][0].device)
            # the kernel wrote the parameters behind autograd's back: a graph that saved one must refuse its backward
            torch.autograd.graph.increment_version([p for p, _ in updated])
        return loss

    def _staging(self):
        st = self.__dict__.get("_dvc_staging")
        return st if st is not None else self.__dict__.setdefault("_dvc_staging", _Staging())

    def _launch(self, entries, device):
        tensors = np.array([e[:6] + e[6] for e in entries], dtype=TENSOR_DTYPE)
        table, _, n_c = _send(self._staging(), tensors, tuple(e[5] for e in entries), device)
        ops.adam_step(table, len(entries), table[tensors.nbytes:], n_c)


# ---- the capturable variant: step counts and bias terms kept on the device
def fingerprint(work):
    """What a set of resident tables was built from, for `work` = [(group, p, grad, state)] (gradients contiguous): per group with
    work its lr (a tensor lr by address), betas, eps, weight_decay and amsgrad; per tensor its group, the five addresses (vmax 0
    without amsgrad), n and the address of its `step`.  Equal fingerprints <=> the tables a rebuild would write are the ones
    already on the device; a parameter whose gradient went to None drops out of `work` and so changes it."""
    groups, index, tensors = [], {}, []
    for group, p, grad, state in work:
        gi = index.get(id(group))
        if gi is None:
            gi = index[id(group)] = len(groups)
            lr = group["lr"]
            groups.append((("tensor", lr.data_ptr()) if isinstance(lr, torch.Tensor) else lr, group["betas"][0], group["betas"][1],
                           group["eps"], group["weight_decay"], bool(group["amsgrad"])))
        tensors.append((gi, p.data_ptr(), grad.data_ptr(), state["exp_avg"].data_ptr(), state["exp_avg_sq"].data_ptr(),
                        state["max_exp_avg_sq"].data_ptr() if group["amsgrad"] else 0, p.numel(), state["step"].data_ptr()))
    return groups, tensors


def build_capturable_tables(work):
    """The three tables of a capturable step from `work` = [(group, p, grad, state)]: (TENSOR_DTYPE, CHUNK_DTYPE, ADVANCE_DTYPE)
    arrays, one tensor and one advance record per entry.  step_size and inv_sqrt_bc2 are left 0: dvc_adam_advance writes them on
    the device before every dvc_adam_step; the other five scalar columns are adam_scalars' (they do not depend on the step)."""
    tensors = np.zeros(len(work), dtype=TENSOR_DTYPE)
    advance = np.zeros(len(work), dtype=ADVANCE_DTYPE)
    for i, (group, p, grad, state) in enumerate(work):
        beta1, beta2 = group["betas"]
        lr = group["lr"]
        vmax = state["max_exp_avg_sq"].data_ptr() if group["amsgrad"] else 0
        sc = adam_scalars(1, 0.0, beta1, beta2, group["eps"], group["weight_decay"])
        tensors[i] = (p.data_ptr(), grad.data_ptr(), state["exp_avg"].data_ptr(), state["exp_avg_sq"].data_ptr(), vmax, p.numel(),
                      0.0, 0.0) + sc[2:]
        if isinstance(lr, torch.Tensor):
            advance[i] = (state["step"].data_ptr(), lr.data_ptr(), 0.0, beta1, beta2)
        else:
            advance[i] = (state["step"].data_ptr(), 0, lr, beta1, beta2)
    return tensors, chunk_table([w[1].numel() for w in work]), advance


class _Resident(tables.Resident):
    """One table tensor on the device ([tensor records | chunk records | advance records | scratch]) and what it was built from."""

    def __init__(self, key, table, c_at, a_at, end, n_t, n_c, params, pinned, stream):
        super().__init__(key, table, pinned, stream)
        self.n_t, self.n_c, self.params = n_t, n_c, params
        self.chunks, self.advance = table[c_at:a_at], table[a_at:end]
        self.scratch = table[end:]          # (CapturableAdam._scratch_bytes: empty unless a subclass asks for some)
        self.guard = None                   # (GuardedAdam: the record its launches on these tables write, kept alive with them)


class CapturableAdam(Adam):
    """torch.optim.Adam(capturable=True) on two HIP launches per step: dvc_adam_advance, then the unchanged dvc_adam_step.

    The constructor is `Adam`'s, except that `lr` may also be a one-element fp32 device tensor and `capturable` is True.
    `state["step"]` is a device fp32 scalar per parameter, and `state_dict()` / `load_state_dict()` are interchangeable with
    `torch.optim.Adam(capturable=True)` in both directions; a CPU `step` loaded from a plain Adam is moved to the device once, and
    nothing ever reads a `step` back.

    The tensor, chunk and advance tables live in ONE device tensor the optimiser owns.  A step validates as `Adam` does (a refused
    step advances nothing), fingerprints the addresses, element counts and hyper-parameters (`fingerprint`), and if nothing moved
    since the tables were uploaded it is exactly two launches: no copy, no allocation, no host arithmetic.  If something moved
    (a reallocated `.grad`, a gradient that went to None, a scheduler's new float `lr`, a loaded state) the tables are rebuilt and
    uploaded from a pinned buffer under `tables.Staging`'s discipline.

    `step()` works under `torch.cuda.graph`.  Take one eager step (or load a state_dict) first: state created during a capture
    would be zeroed again by every replay, so a captured step refuses to create it.  Tables uploaded during a capture, and tables
    a graph refers to, are kept as dvc_amd.tables says; the replayed copy re-sends the same bytes and the advance launch that
    follows rewrites the two step-dependent columns from the device `step`: a replay is correct whatever the copy restored.
    A float `lr` changed by a scheduler is seen by the next eager `step()` but not by a replay (it is baked into the captured
    tables); a tensor `lr` updated in place is seen by both.

    A replay runs no host code, so it cannot bump the parameters' version counters as the eager `step()` does: call
    `mark_updated()` after every replay.  Without it the modules' packed-weight caches, which are keyed on the version, go stale,
    and a graph that saved a parameter does not refuse its backward."""

    _name = "dvc_amd.optim.CapturableAdam"
    _capturable = True
    _refused_flags = tuple(f for f in _REFUSED_FLAGS if f != "capturable")

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, amsgrad=False, *, foreach=None,
                 maximize=False, capturable=True, differentiable=False, fused=None, decoupled_weight_decay=False,
                 max_grad_norm=None, skip_nonfinite=None):
        if not capturable:
            raise ValueError(f"{self._name}: `capturable=False` is dvc_amd.optim.Adam")
        super().__init__(params, lr, betas, eps, weight_decay, amsgrad, foreach=foreach, maximize=maximize, capturable=True,
                         differentiable=differentiable, fused=fused, decoupled_weight_decay=decoupled_weight_decay,
                         max_grad_norm=max_grad_norm, skip_nonfinite=skip_nonfinite)
        self._ensure_spare()

    def __setstate__(self, state):
        super().__setstate__(state)
        for group in self.param_groups:
            group["capturable"] = True
            for p in group["params"]:
                st = self.state.get(p)
                if st:
                    st["step"] = self._device_step(st["step"], p)

    def add_param_group(self, param_group):
        super().add_param_group(param_group)
        if "_dvc_spare" in self.__dict__:       # (not while the constructor is still adding its groups)
            self._ensure_spare()

    @staticmethod
    def _device_step(step, p):
        """`step` as a float32 tensor on p's device (a CPU step of a plain Adam's state_dict is moved once, never read)."""
        if step.device != p.device or step.dtype != torch.float32:
            step = step.detach().to(device=p.device, dtype=torch.float32)
        return step

    def _check_group(self, group):
        if any(isinstance(b, torch.Tensor) for b in group["betas"]):
            raise NotImplementedError(f"{self._name}: tensor `betas` are not supported; pass floats")
        lr = group["lr"]
        if isinstance(lr, torch.Tensor):
            if lr.numel() != 1 or lr.dtype != torch.float32:
                raise ValueError(f"{self._name}: a tensor `lr` must be a one-element float32 tensor")
            if not lr.is_cuda:
                raise RuntimeError(f"{self._name}: a tensor `lr` must be a ROCm device tensor; the HIP step has no CPU fallback")

    def _new_step(self, p):
        return torch.zeros((), dtype=torch.float32, device=p.device)

    def _collect(self):
        work = super()._collect()
        for _, p, _, state in work:
            step = state["step"]
            if not torch.is_tensor(step) or step.numel() != 1:
                raise ValueError(f"{self._name}: state `step` must be a one-element tensor")
            if step.device != p.device or step.dtype != torch.float32:
                state["step"] = self._device_step(step, p)
        return work

    # ---- pinned memory for an upload that is itself captured
    def _table_bytes_bound(self):
        params = [p for group in self.param_groups for p in group["params"]]
        n_c = n_chunks(p.numel() for p in params)
        return len(params) * (TENSOR_DTYPE.itemsize + ADVANCE_DTYPE.itemsize) + n_c * CHUNK_DTYPE.itemsize

    def _ensure_spare(self):
        """Keep one pinned buffer, large enough for the tables of every parameter, allocated OUTSIDE any capture: pinned memory
        cannot be relied on to be allocatable while a stream is capturing, and a captured upload needs a buffer of its own."""
        need = self._table_bytes_bound()
        spare = self.__dict__.setdefault("_dvc_spare", None)
        if spare is not None and spare.numel() >= need:
            return
        if need == 0 or not any(p.is_cuda for group in self.param_groups for p in group["params"]):
            return
        if torch.cuda.is_current_stream_capturing():
            return
        self.__dict__["_dvc_spare"] = torch.empty(need, dtype=torch.uint8, pin_memory=True)

    # ---- one step
    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        capturing = _capturing()
        if capturing:
            for group in self.param_groups:
                for p in group["params"]:
                    if p.grad is not None and len(self.state.get(p, ())) == 0:
                        raise RuntimeError(f"{self._name}: a parameter has no state yet and the stream is capturing: every replay "
                                           "would zero it again; take one eager step() or load a state_dict before the capture")
        work = self._collect()
        if not work:
            return loss
        if not all(w[2].is_contiguous() for w in work):
            work = [(g, p, grad if grad.is_contiguous() else grad.contiguous(), st) for g, p, grad, st in work]
        key = fingerprint(work)
        res = self.__dict__.get("_dvc_resident")
        if res is None or res.key != key:
            res = self._upload(work, key, capturing)
        res.use(self.__dict__.setdefault("_dvc_captured", []) if capturing else None, capturing, ops._stream_handle())
        self._launch_resident(res, capturing)
        # the kernel wrote the parameters behind autograd's back: a graph that saved one must refuse its backward
        torch.autograd.graph.increment_version(res.params)
        if not capturing and self.__dict__.get("_dvc_spare") is None:
            self._ensure_spare()
        return loss

    def _launch_resident(self, res, capturing):
        """The launches of one step on resident tables (GuardedAdam puts the norm in front and uses the guarded pair)."""
        ops.adam_advance(res.advance, res.table, res.n_t)
        if res.n_c:
            ops.adam_step(res.table, res.n_t, res.chunks, res.n_c)

    def _scratch_bytes(self, n_c):
        """Bytes of device scratch kept behind the three tables, in the same tensor (GuardedAdam: the norm's partials)."""
        return 0

    def mark_updated(self):
        """Bump the version counter of every parameter the resident tables update — what the eager `step()` does after its
        launches, and what a graph replay cannot do: host-only, no GPU work.  Call it after every replay of a captured step."""
        res = self.__dict__.get("_dvc_resident")
        if res is not None:
            torch.autograd.graph.increment_version(res.params)

    def _upload(self, work, key, capturing):
        """Rebuild the three tables and send them to a fresh table tensor with one host-to-device copy on the current stream."""
        tensors, chunks, advance = build_capturable_tables(work)
        n_t, n_c = len(tensors), len(chunks)
        nbytes = tensors.nbytes + chunks.nbytes + advance.nbytes
        if capturing:       # a buffer of its own, never rewritten: the replay's copy node reads it again
            pinned = self.__dict__.get("_dvc_spare")
            self.__dict__["_dvc_spare"] = None
            if pinned is None or pinned.numel() < nbytes:
                pinned = torch.empty(nbytes, dtype=torch.uint8, pin_memory=True)
        else:
            st = self._staging()
            slot = st.acquire(nbytes)
            pinned = st.buf[slot]
        (_, c_at, a_at), _ = tables.pack(pinned.numpy(), [tensors, chunks, advance])
        table = tables.upload(pinned, nbytes, work[0][1].device, self._scratch_bytes(n_c))
        if not capturing:
            st.sent(slot)
        res = self.__dict__["_dvc_resident"] = _Resident(key, table, c_at, a_at, nbytes, n_t, n_c, [w[1] for w in work],
                                                         pinned if capturing else None, ops._stream_handle())
        return res


# ---- the gradient guard: norm, clipping, non-finite skip
_NONFINITE_MESSAGE = ("The total norm of order {} for gradients from `parameters` is non-finite, so it cannot be clipped. To disable "
                      "this error and scale the gradients by the non-finite norm anyway, set `error_if_nonfinite=False`")


def _checked_max_norm(max_norm, where):
    """`max_norm` as a float; None is +inf (no clipping).  NaN and values <= 0 are refused, as dvc_grad_norm refuses them."""
    if max_norm is None:
        return math.inf
    if isinstance(max_norm, torch.Tensor):
        raise NotImplementedError(f"{where}: a tensor `max_norm` is not supported (it is a launch argument); pass a float")
    max_norm = float(max_norm)
    if not max_norm > 0.0:
        raise ValueError(f"{where}: `max_norm` must be a positive number or None (got {max_norm})")
    return max_norm


def new_guard(device):
    """A zeroed DvcGradGuard record on `device`, as the uint8 tensor the launch wrappers take."""
    return torch.zeros(GUARD_DTYPE.itemsize, dtype=torch.uint8, device=device)


def guard_views(guard):
    """(total_norm, skipped) of a guard record as 0-dim device tensors that VIEW it: float32 and int32."""
    return guard[0:4].view(torch.float32)[0], guard[12:16].view(torch.int32)[0]


def read_guard(guard):
    """The record read back as a dict of Python numbers (total_norm, clip_coef, found_inf, skipped, sumsq).  Synchronises."""
    rec = guard.cpu().numpy().view(GUARD_DTYPE)[0]
    return {name: rec[name].item() for name in GUARD_DTYPE.names}


def build_norm_tables(grads):
    """The two tables dvc_grad_norm / dvc_grad_scale walk for the contiguous fp32 tensors `grads`, through build_tables: only g and n
    of a record are filled in, the four other addresses and the scalars are 0 (those kernels read nothing else)."""
    zeros = (0.0,) * 8
    return build_tables([(0, g.data_ptr(), 0, 0, 0, g.numel(), zeros) for g in grads])


_functional_staging = _Staging()


def _gradients(parameters, where, in_place):
    if isinstance(parameters, torch.Tensor):
        parameters = [parameters]
    grads = [p.grad for p in parameters if p.grad is not None]
    for g in grads:
        if g.is_sparse:
            raise NotImplementedError(f"{where}: sparse gradients are not supported")
        if not g.is_cuda:
            raise RuntimeError(f"{where}: gradients must be ROCm device tensors; the HIP reduction has no CPU fallback")
        if g.dtype != torch.float32:
            raise TypeError(f"{where}: gradients must be float32 (got {g.dtype})")
        if in_place and not g.is_contiguous():
            raise ValueError(f"{where}: a gradient of shape {tuple(g.shape)} and strides {g.stride()} is not contiguous and cannot "
                             "be scaled in place")
    if grads:
        dev = ops._current_device()
        for g in grads:
            if g.device.index != dev:
                raise RuntimeError(f"{where}: a gradient lives on {g.device} but the current device is cuda:{dev}; call "
                                   "torch.cuda.set_device / use torch.cuda.device(...)")
    return [g if g.is_contiguous() else g.contiguous() for g in grads]


def _functional_norm(grads, max_norm, where):
    """Upload the tables of `grads` through _functional_staging and launch dvc_grad_norm.  -> (table, n_t, chunks, n_c, guard)"""
    _refuse_capture(where, "gradients", ", or use dvc_amd.optim.GuardedAdam")
    tensors, chunks = build_norm_tables(grads)
    n_t, n_c = len(tensors), len(chunks)
    t_bytes, nbytes = tensors.nbytes, tensors.nbytes + chunks.nbytes
    st = _functional_staging
    slot = st.acquire(nbytes)
    tables.pack(st.buf[slot].numpy(), [tensors, chunks])
    device = grads[0].device
    table = tables.upload(st.buf[slot], nbytes, device, 8 * n_c)        # (tables | partials; freed on return, in stream order)
    st.sent(slot)
    guard = new_guard(device)
    ops.grad_norm(table, n_t, table[t_bytes:nbytes], n_c, table[nbytes:].view(torch.float64), max_norm, guard)
    return table, n_t, table[t_bytes:nbytes], n_c, guard


def grad_norm(parameters):
    """The global L2 norm of the gradients of `parameters` (a tensor or an iterable; those without a .grad sit out) as a 0-dim fp32
    device tensor: one dvc_grad_norm, nothing synchronised.  Raises while the stream is capturing."""
    where = "dvc_amd.optim.grad_norm"
    grads = _gradients(parameters, where, in_place=False)
    if sum(g.numel() for g in grads) == 0:
        return torch.zeros((), device=grads[0].device) if grads else torch.tensor(0.0)
    guard = _functional_norm(grads, math.inf, where)[-1]
    return guard_views(guard)[0]


@torch.no_grad()
def clip_grad_norm_(parameters, max_norm, norm_type=2.0, error_if_nonfinite=False, foreach=None):
    """torch.nn.utils.clip_grad_norm_ on one dvc_grad_norm and one dvc_grad_scale: the gradients are multiplied in place by
    min(1, max_norm / (norm + 1e-6)) and the norm comes back as a 0-dim fp32 device tensor.  Nothing is synchronised unless
    `error_if_nonfinite` (one read of the flag).  Only the 2-norm; `foreach` is accepted and ignored (there is one path).
    Non-finite gradients without `error_if_nonfinite` are scaled as torch scales them (include/dvc_hip.h, dvc_grad_scale)."""
    where = "dvc_amd.optim.clip_grad_norm_"
    if float(norm_type) != 2.0:
        raise NotImplementedError(f"{where}: only norm_type=2 is supported by the HIP reduction (got {norm_type})")
    if max_norm is None:
        raise ValueError(f"{where}: `max_norm` must be a positive number (got None)")
    max_norm = _checked_max_norm(max_norm, where)
    grads = _gradients(parameters, where, in_place=True)
    if sum(g.numel() for g in grads) == 0:
        return torch.zeros((), device=grads[0].device) if grads else torch.tensor(0.0)
    table, n_t, chunks, n_c, guard = _functional_norm(grads, max_norm, where)
    if error_if_nonfinite and read_guard(guard)["found_inf"]:
        raise RuntimeError(_NONFINITE_MESSAGE.format(float(norm_type)))
    ops.grad_scale(table, n_t, chunks, n_c, guard)
    return guard_views(guard)[0]


class GuardedAdam(CapturableAdam):
    """CapturableAdam whose step first measures its gradients, on four launches in a straight line over the resident tables:
    dvc_grad_norm (two), dvc_adam_advance_guarded, dvc_adam_step_guarded.

    `max_grad_norm` (keyword only; None: no clipping) is torch.nn.utils.clip_grad_norm_'s `max_norm`, over every tensor that has a
    gradient in that step, all groups together: the step runs on min(1, max_grad_norm / (norm + 1e-6)) * g without writing `.grad`.
    `skip_nonfinite` (default True): if any gradient holds a NaN or an Inf the step does nothing at all — parameters, moments and
    every `step` count keep their bytes — and `skipped_steps` goes up by one.  With skip_nonfinite=False the same launches run but
    the flag is never raised, and non-finite gradients do what they do to CapturableAdam.  With neither option active the result is
    CapturableAdam's bit for bit (the multiply is by 1.0f).

    Both options are attributes of the optimiser, not group keys: `state_dict()` is CapturableAdam's and loads into
    torch.optim.Adam(capturable=True); pickling and deepcopy keep them.  An eager step reads them afresh; a replay has them baked in.

    `last_grad_norm` (0-dim float32) and `skipped_steps` (0-dim int32) are device tensors that view the guard record, which is
    allocated once, at construction, and lives as long as the optimiser; reading them synchronises, nothing in step() does.  The
    norm's partial sums live behind the resident tables, in the same tensor, and are rebuilt with them.  A norm of finite
    gradients that exceeds the fp32 range reads inf but does not skip the step: the flag and the coefficient come from the double.
    The count is not part of state_dict(); a copy or an unpickled optimiser starts from 0.

    Capture is CapturableAdam's, rule for rule; the captured sequence is [copy,] norm, finish, advance, step, with no branches."""

    _name = "dvc_amd.optim.GuardedAdam"
    _guarded = True

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, amsgrad=False, *, foreach=None,
                 maximize=False, capturable=True, differentiable=False, fused=None, decoupled_weight_decay=False,
                 max_grad_norm=None, skip_nonfinite=True):
        _checked_max_norm(max_grad_norm, self._name)
        self.max_grad_norm = max_grad_norm
        self.skip_nonfinite = bool(skip_nonfinite)
        super().__init__(params, lr, betas, eps, weight_decay, amsgrad, foreach=foreach, maximize=maximize, capturable=capturable,
                         differentiable=differentiable, fused=fused, decoupled_weight_decay=decoupled_weight_decay)
        self._ensure_guard()

    def __getstate__(self):
        state = super().__getstate__()
        state["max_grad_norm"], state["skip_nonfinite"] = self.max_grad_norm, self.skip_nonfinite
        return state

    def __setstate__(self, state):
        super().__setstate__(state)
        self.__dict__.setdefault("max_grad_norm", None)
        self.__dict__.setdefault("skip_nonfinite", True)

    def add_param_group(self, param_group):
        super().add_param_group(param_group)
        if "_dvc_spare" in self.__dict__:       # (not while the constructor is still adding its groups)
            self._ensure_guard()

    def _ensure_guard(self):
        """The guard record, allocated and zeroed OUTSIDE any capture (a zeroing inside one would be replayed, count and all)."""
        guard = self.__dict__.get("_dvc_guard")
        if guard is not None:
            return guard
        device = next((p.device for group in self.param_groups for p in group["params"] if p.is_cuda), None)
        if device is None:
            return None
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError(f"{self._name}: the guard record does not exist yet and the stream is capturing: every replay would "
                               "zero it again; construct the optimiser (or take one eager step) before the capture")
        guard = self.__dict__["_dvc_guard"] = new_guard(device)
        self.__dict__["_dvc_guard_stream"] = ops._stream_handle()
        return guard

    def _guard_view(self, which):
        guard = self._ensure_guard()
        if guard is None:
            raise RuntimeError(f"{self._name}: no parameter is a ROCm device tensor yet, so there is no guard record to read")
        return guard_views(guard)[which]

    @property
    def last_grad_norm(self):
        return self._guard_view(0)

    @property
    def skipped_steps(self):
        return self._guard_view(1)

    def _scratch_bytes(self, n_c):
        return 8 * n_c

    def _launch_resident(self, res, capturing):
        if not res.n_c:         # only empty tensors: nothing to measure, nothing to skip
            return super()._launch_resident(res, capturing)
        guard = res.guard = self._ensure_guard()
        if not capturing and ops._stream_handle() != self.__dict__["_dvc_guard_stream"]:
            guard.record_stream(torch.cuda.current_stream())
            self.__dict__["_dvc_guard_stream"] = ops._stream_handle()
        max_norm = _checked_max_norm(self.max_grad_norm, self._name)
        ops.grad_norm(res.table, res.n_t, res.chunks, res.n_c, res.scratch.view(torch.float64), max_norm, guard,
                      keep_nonfinite=not self.skip_nonfinite)
        ops.adam_advance_guarded(res.advance, res.table, res.n_t, guard)
        ops.adam_step_guarded(res.table, res.n_t, res.chunks, res.n_c, guard)
