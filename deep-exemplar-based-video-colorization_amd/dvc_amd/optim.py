"""Adam on the package's own kernel: `dvc_amd.optim.Adam` is a drop-in for `torch.optim.Adam` whose `step()` updates every
parameter of every group in ONE launch of dvc_adam_step (csrc/optim.hip; the design is DESIGN.md §6d).

Same constructor, same lazily created state ({"step", "exp_avg", "exp_avg_sq"[, "max_exp_avg_sq"]}, `step` a CPU float32 scalar
per parameter), and a `state_dict()` that `torch.optim.Adam` loads and vice versa; LR schedulers, `add_param_group` and
`zero_grad` are the base class's.  What it does not do it refuses by name: maximize, capturable, differentiable,
decoupled_weight_decay, foreach=True, fused=True, tensor hyper-parameters, CPU / non-fp32 / sparse / non-contiguous tensors.

Per step the host evaluates each tensor's scalars in double (per TENSOR: torch keeps `step` per parameter, and groups differ in
`lr`), writes the tensor and chunk tables into a pinned staging buffer, sends them with one host-to-device copy on the current
stream and launches once.  Two staging buffers alternate, each behind an event recorded after its copy, so a step never
overwrites a buffer whose copy has not run yet.  The scalars change every step, so a step cannot be replayed from a captured
graph: `step()` raises while the current stream is capturing.
"""
import math

import numpy as np
import torch
from torch.optim.optimizer import Optimizer

from . import _lib, ops

CHUNK = 4096  # elements per chunk == DVC_ADAM_CHUNK of include/dvc_hip.h (tests/test_adam_host.py holds the two together)
TENSOR_DTYPE = np.dtype(_lib.DvcAdamTensor)
CHUNK_DTYPE = np.dtype(_lib.DvcAdamChunk)
_REFUSED_FLAGS = ("maximize", "capturable", "differentiable", "decoupled_weight_decay")


def adam_scalars(step, lr, beta1, beta2, eps, weight_decay):
    """The per-tensor scalars of step number `step` (>= 1), evaluated in double, in the order of DvcAdamTensor's float fields;
    each is rounded once, to fp32, when it is stored in the table."""
    bc1 = 1.0 - beta1 ** step
    bc2 = 1.0 - beta2 ** step
    return (lr / bc1, 1.0 / math.sqrt(bc2), beta2, 1.0 - beta1, 1.0 - beta2, eps, weight_decay, 0.0)


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


class _Staging:
    """Two pinned buffers used in turn; `event[i]` is recorded after the copy out of buffer i."""

    def __init__(self):
        self.buf = [None, None]
        self.event = [None, None]
        self.counts = [None, None]      # the counts whose chunk table buffer i holds (at the offset they imply)
        self.slot = 0


class Adam(Optimizer):
    """torch.optim.Adam on one HIP launch per step.  See the module docstring."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, amsgrad=False, *, foreach=None,
                 maximize=False, capturable=False, differentiable=False, fused=None, decoupled_weight_decay=False):
        if isinstance(lr, torch.Tensor):
            raise NotImplementedError("dvc_amd.optim.Adam: a tensor `lr` is not supported (the step's scalars are evaluated on "
                                      "the host); pass a float")
        if any(isinstance(b, torch.Tensor) for b in betas):
            raise NotImplementedError("dvc_amd.optim.Adam: tensor `betas` are not supported; pass floats")
        for name, value in (("maximize", maximize), ("capturable", capturable), ("differentiable", differentiable),
                            ("decoupled_weight_decay", decoupled_weight_decay), ("foreach", foreach), ("fused", fused)):
            if value:
                raise NotImplementedError(f"dvc_amd.optim.Adam: `{name}=True` is not supported by the HIP step")
        if not 0.0 <= lr:
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
                        foreach=None, capturable=False, differentiable=False, fused=None, decoupled_weight_decay=False)
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

    # ---- one step
    def _collect(self):
        """Validate everything and create missing state; nothing is advanced.  -> [(group, p, grad, state)]"""
        work = []
        for group in self.param_groups:
            for name in _REFUSED_FLAGS:
                if group.get(name):
                    raise NotImplementedError(f"dvc_amd.optim.Adam: `{name}=True` is not supported by the HIP step")
            if isinstance(group["lr"], torch.Tensor) or any(isinstance(b, torch.Tensor) for b in group["betas"]):
                raise NotImplementedError("dvc_amd.optim.Adam: a tensor `lr` / `betas` is not supported; pass floats")
            for p in group["params"]:
                grad = p.grad
                if grad is None:
                    continue
                if grad.is_sparse:
                    raise RuntimeError("Adam does not support sparse gradients, please consider SparseAdam instead")
                if not p.is_cuda or not grad.is_cuda:
                    raise RuntimeError("dvc_amd.optim.Adam: parameters and gradients must be ROCm device tensors; the HIP step has "
                                       "no CPU fallback")
                if p.dtype != torch.float32 or grad.dtype != torch.float32:
                    raise TypeError(f"dvc_amd.optim.Adam: parameters and gradients must be float32 (got {p.dtype}, {grad.dtype})")
                if not p.is_contiguous():
                    raise ValueError(f"dvc_amd.optim.Adam: a parameter of shape {tuple(p.shape)} and strides {p.stride()} is not "
                                     "contiguous")
                if grad.shape != p.shape:
                    raise ValueError(f"dvc_amd.optim.Adam: gradient shape {tuple(grad.shape)} != parameter {tuple(p.shape)}")
                state = self.state[p]
                if len(state) == 0:
                    state["step"] = torch.tensor(0.0, dtype=torch.float32)
                    state["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                    state["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                    if group["amsgrad"]:
                        state["max_exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                elif group["amsgrad"] and "max_exp_avg_sq" not in state:
                    raise RuntimeError("dvc_amd.optim.Adam: amsgrad was switched on for a parameter whose state has no max_exp_avg_sq")
                for key in ("exp_avg", "exp_avg_sq") + (("max_exp_avg_sq",) if group["amsgrad"] else ()):
                    s = state[key]
                    if not s.is_cuda:
                        raise RuntimeError(f"dvc_amd.optim.Adam: state `{key}` is a CPU tensor; the HIP step has no CPU fallback")
                    if s.dtype != torch.float32:
                        raise TypeError(f"dvc_amd.optim.Adam: state `{key}` must be float32 (got {s.dtype})")
                    if not s.is_contiguous() or s.numel() != p.numel():
                        raise ValueError(f"dvc_amd.optim.Adam: state `{key}` must be contiguous with {p.numel()} elements")
                work.append((group, p, grad, state))
        if work:
            dev = ops._current_device()
            for _, p, grad, state in work:
                for t in (p, grad, state["exp_avg"], state["exp_avg_sq"], state.get("max_exp_avg_sq")):
                    if t is not None and t.device.index != dev:
                        raise RuntimeError(f"dvc_amd.optim.Adam: a tensor lives on {t.device} but the current device is cuda:{dev}; "
                                           "call torch.cuda.set_device / use torch.cuda.device(...)")
        return work

    @torch.no_grad()
    def step(self, closure=None):
        if torch.cuda.is_initialized() and torch.cuda.is_current_stream_capturing():       # before anything is allocated or launched
            raise RuntimeError("dvc_amd.optim.Adam: step() cannot be captured into a graph: its scalars (the bias corrections of "
                               "step t) change every step and are launch-time table entries; step outside the capture")
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

    def _launch(self, entries, device):
        st = self.__dict__.get("_dvc_staging")
        if st is None:
            st = self.__dict__["_dvc_staging"] = _Staging()
        counts = tuple(e[5] for e in entries)
        n_t = len(entries)
        n_c = sum((n + CHUNK - 1) // CHUNK for n in counts)
        t_bytes, c_bytes = n_t * TENSOR_DTYPE.itemsize, n_c * CHUNK_DTYPE.itemsize       # (80 n_t: the chunk table stays 16-byte aligned)
        nbytes = t_bytes + c_bytes
        slot = st.slot = 1 - st.slot
        if st.event[slot] is not None:
            st.event[slot].synchronize()        # the copy that last read this buffer (two steps ago) has run
        if st.buf[slot] is None or st.buf[slot].numel() < nbytes:
            st.buf[slot] = torch.empty(nbytes + nbytes // 4, dtype=torch.uint8, pin_memory=True)
            st.counts[slot] = None
        host = st.buf[slot].numpy()
        host[:t_bytes].view(TENSOR_DTYPE)[:] = np.array([e[:6] + e[6] for e in entries], dtype=TENSOR_DTYPE)
        if st.counts[slot] != counts:
            host[t_bytes:nbytes].view(CHUNK_DTYPE)[:] = chunk_table(counts)
            st.counts[slot] = counts
        table = torch.empty(nbytes, dtype=torch.uint8, device=device)       # (freed on return: the allocator reuses it in stream order)
        table.copy_(st.buf[slot][:nbytes], non_blocking=True)
        if st.event[slot] is None:
            st.event[slot] = torch.cuda.Event()
        st.event[slot].record()
        ops.adam_step(table, n_t, table[t_bytes:], n_c)
