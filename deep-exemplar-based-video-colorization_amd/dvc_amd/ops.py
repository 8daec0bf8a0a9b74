"""Tensor-level wrappers over the C-ABI (include/dvc_hip.h).

PyTorch is used here only for device memory (torch.empty on the caching allocator) and for the
current HIP stream; every number is produced by the kernels in csrc/.  All functions require
contiguous fp32 ROCm tensors and raise otherwise — there is no CPU fallback.

Order of the file: plumbing, run-time switches (ONE table), the autotuner, then the wrappers grouped as in the header —
convolutions, norms and pools, colour, correlation, backward.
"""
import ctypes
import os as _os
import sys
from typing import NamedTuple

import torch

from . import _lib
from ._lib import DvcConvDesc, DvcConvGroupItem, DvcInstNormItem

ACT_NONE, ACT_RELU, ACT_PRELU, ACT_LEAKY, ACT_TANH128 = 0, 1, 2, 3, 4
PAD_ZERO, PAD_REFLECT = 0, 1
EPS64 = sys.float_info.epsilon  # the reference adds float64 epsilon to fp32 norms (util.py:156)


# ---- plumbing
def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _pv(t):
    """Raw address for a ctypes structure field (None -> NULL)."""
    return None if t is None else t.data_ptr()


# The launch thread issues ~150 kernels per frame and is within 10-15 % of being the bottleneck of the clip driver
# (tools/host_issue_probe.py: 2.1 ms of host time per 2.4 ms frame), so the per-call plumbing uses torch's raw accessors:
# torch.cuda.current_stream() builds a Stream object through four Python frames (3 us, called once or twice per launch).
_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)
_raw_device = getattr(torch._C, "_cuda_getDevice", None)


def _current_device():
    return _raw_device() if _raw_device is not None else torch.cuda.current_device()


def _stream_handle():
    """The current HIP stream of the current device as an integer handle."""
    if _raw_stream is not None:
        return _raw_stream(_current_device())
    return torch.cuda.current_stream().cuda_stream


def _stream():
    return ctypes.c_void_p(_stream_handle())


def _need(t, name):
    if t is None:
        return
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise RuntimeError(f"dvc_amd: `{name}` must be a ROCm device tensor; the HIP path has no CPU fallback")
    if t.dtype != torch.float32:
        raise RuntimeError(f"dvc_amd: `{name}` must be float32 (got {t.dtype})")
    if not t.is_contiguous():
        raise RuntimeError(f"dvc_amd: `{name}` must be contiguous")
    if t.device.index != _current_device():
        # libdvc_hip launches on the CURRENT device's current stream and never calls hipSetDevice:
        # one process per GPU (torch.cuda.set_device(LOCAL_RANK)) is the supported mode
        raise RuntimeError(f"dvc_amd: `{name}` lives on {t.device} but the current device is cuda:"
                           f"{_current_device()}; call torch.cuda.set_device / use torch.cuda.device(...)")


def _need_all(**named):
    """_need for every `name=tensor` pair, in the order given (None: an optional argument that was not passed)."""
    for name, t in named.items():
        _need(t, name)


_ws_cache = {}
_ws_scope = None


class workspace_scope:
    """While active, scratch buffers come from `store` (a dict the caller owns) instead of the per-stream cache: a captured
    launch sequence (dvc_amd/graph.py) bakes its workspace addresses in and may be replayed on any stream, next to eager
    launches or other graphs that use that stream's workspaces — so every capture gets private ones."""

    def __init__(self, store):
        self.store = store

    def __enter__(self):
        global _ws_scope
        self.prev, _ws_scope = _ws_scope, self.store
        return self.store

    def __exit__(self, *exc):
        global _ws_scope
        _ws_scope = self.prev


def _workspace(device, nbytes, tag="corr"):
    if _ws_scope is not None:
        cache, key = _ws_scope, (tag, device.index)
    else:
        cache, key = _ws_cache, (tag, device.index, _stream_handle())
    ws = cache.get(key)
    if ws is None or ws.numel() < nbytes:
        ws = torch.empty(nbytes, device=device, dtype=torch.uint8)
        cache[key] = ws
    return ws


conv_record = None   # set to a list to log every conv2d launch (tools/tune_conv.py)
layer_record = None  # set to a list to log every NAMED 3x3 layer that goes through conv3x3 (tools/engine_sensitivity.py)


# ---- run-time switches.  Every switch is declared ONCE, in _SWITCHES: the environment variable that seeds it, the default,
# the parse rule, and whether it decides WHICH launches a sequence consists of (launch_epoch -> graph._epoch: a captured
# hipGraph that was recorded under another value is stale).  The value itself lives in the module global `var`, which the
# per-launch code below reads directly — a switch read costs one global load, as it always did.
def _on_unless_0(v):
    """On for anything but the literal "0"."""
    return v != "0"


def _on_if_1(v):
    """On for the literal "1" only."""
    return v == "1"


def _memo_mode(v):
    """DVC_EXEMPLAR_MEMO: "0" off, "verify", anything else on."""
    return {"0": "off", "verify": "verify"}.get(v, "on")


def _layer_names(v):
    """DVC_DIRECT_LAYERS: comma-separated layer names (the empty string: none); unset: the built-in map."""
    return None if v is None else frozenset(v.split(","))


class _Switch(NamedTuple):
    getter: str     # public function that returns the value
    setter: str     # public `set_x(flag=True)`: a plain flag, getter and setter are generated below; None: both are written out
                    # by hand further down (values that are not flags, setters that do more than store)
    var: str        # module global that holds the value
    env: str        # environment variable read once, at import (None: no variable)
    default: str    # what an unset variable counts as
    parse: object   # environment string -> value
    launch: bool    # decides which launches a sequence consists of


_SWITCHES = (
    # the analogue of the reference's `cudnn.benchmark = True` (autotuner block below)
    _Switch("autotune_enabled", None, "_autotune", "DVC_AUTOTUNE", "0", _on_if_1, True),
    # weights-in-registers direct engine (csrc/conv_ws.hip): the large-map / few-channel 3x3 layers that stay on the direct
    # engine (ColorVidNet conv1_1[2], conv1_2, conv2_1 under the error-aware map).  0: the general direct engine (A/B)
    _Switch("ws_conv_enabled", "set_ws_conv", "_ws_conv", "DVC_WS_CONV", "1", _on_unless_0, True),
    # VGG19's max pools out of the launch of the convolution in front of them (conv2d_winograd_pool)
    _Switch("pool_fusion", "set_pool_fusion", "_pool_fusion", "DVC_POOL_FUSION", "1", _on_unless_0, True),
    # decoder-block pairs `conv(up(a)) + conv_short(b)` as one launch (0: two launches)
    _Switch("dual_conv_enabled", "set_dual_conv", "_dual_conv", "DVC_DUAL_CONV", "1", _on_if_1, True),
    # conv -> InstanceNorm pairs: let the InstanceNorm launch sum the convolution's split-K partials
    _Switch("fuse_reduce", "set_fuse_reduce", "_fuse_reduce", "DVC_FUSE_REDUCE", "1", _on_if_1, True),
    # engine of the 3x3 stride-1 layers: see set_conv_algo
    _Switch("conv_algo", None, "_conv_algo", "DVC_CONV_ALGO", "auto", str, True),
    # the exemplar side of WarpNet memoised behind the reference's unmodified call pattern: see set_exemplar_memo
    _Switch("exemplar_memo_mode", None, "_exemplar_memo", "DVC_EXEMPLAR_MEMO", "1", _memo_mode, False),
    # the training side's plain batched GEMMs through the vendor library: see bmm.  The INFERENCE path never goes there
    _Switch("gemm_lib", "set_gemm_lib", "_gemm_lib", "DVC_GEMM_LIB", "1", _on_unless_0, False),
    # gray2rgb_batch folded into VGG19 conv1_1's load behind warp_color (0: the two launches, bit-identical)
    _Switch("gray_fusion", "set_gray_fusion", "_gray_fusion", "DVC_GRAY_FUSION", "1", _on_unless_0, True),
    # independent layers as one launch (WarpNet's four heads).  0: one launch per layer (A/B; results are bit-identical either
    # way — every item keeps the plan and the kernel body it has alone)
    _Switch("group_heads", "set_group_heads", "_group_heads", "DVC_GROUP_HEADS", "1", _on_unless_0, True),
    # the merge of the correlation's partial softmax states folded into its consumer (pack_color_input)
    _Switch("fold_merge", "set_fold_merge", "_fold_merge", "DVC_FOLD_MERGE", "1", _on_if_1, True),
    # Winograd launches planned for the whole batch: no variable, set by the `batch_plan` context manager
    _Switch("batch_plan_enabled", None, "_batch_plan", None, "0", _on_if_1, True),
    # the error-aware engine map: see direct_layers / set_direct_layers
    _Switch("direct_layers", None, "DEFAULT_DIRECT_LAYERS", "DVC_DIRECT_LAYERS", None, _layer_names, True),
)


def _flag_functions(var, getter, setter):
    """The public pair of a plain flag: getter() -> the module global `var`, setter(flag=True) stores bool(flag) in it."""
    g = globals()

    def get():
        return g[var]

    def set_(flag=True):
        g[var] = bool(flag)
    get.__name__ = get.__qualname__ = getter
    set_.__name__ = set_.__qualname__ = setter
    return get, set_


for _sw in _SWITCHES:
    globals()[_sw.var] = _sw.parse(_os.environ.get(_sw.env, _sw.default) if _sw.env else _sw.default)
    if _sw.setter:
        globals()[_sw.getter], globals()[_sw.setter] = _flag_functions(_sw.var, _sw.getter, _sw.setter)
del _sw


def launch_epoch():
    """The value of every switch that decides which launches a sequence consists of, read through its public getter."""
    g = globals()
    return tuple(g[sw.getter]() for sw in _SWITCHES if sw.launch)


def autotune_enabled():
    return _autotune


def set_autotune(flag=True):
    global _autotune
    _autotune = bool(flag)
    if _autotune:
        _load_tuned()


# ---- algorithm choice for the 3x3 stride-1 layers.  "direct": the implicit-GEMM engine everywhere; "winograd": the
# F(2x2,3x3) kernel on every layer it takes; "auto" (default): the static rule below, fitted to
# profiles/r02_conv_wino_probe.txt (Winograd where it is measured faster).  The choice is a pure function of the layer
# geometry, so the clip driver's pipelined and sequential orders still run the same kernels (bit-identical outputs).
def conv_algo():
    return _conv_algo


def set_conv_algo(algo):
    global _conv_algo
    if algo not in ("auto", "speed", "direct", "winograd"):
        raise ValueError("conv algo must be 'auto', 'speed', 'direct' or 'winograd'")
    _conv_algo = algo


# the exemplar side of WarpNet memoised behind the reference's unmodified call pattern (nets.WarpNet._memo_exemplar_side).
# DVC_EXEMPLAR_MEMO: "1" (default) on, "0" off, "verify" = on, and every hit ALSO recomputes the exemplar side and compares it
# bit for bit with the memo (a mismatch warns, replaces the memo and returns the fresh value) — the debugging mode for callers
# that write to the exemplar tensors or the WarpNet parameters through `.data`, which no version counter sees.
def exemplar_memo_enabled():
    return _exemplar_memo != "off"


def exemplar_memo_mode():
    """"on" | "off" | "verify"."""
    return _exemplar_memo


def set_exemplar_memo(flag=True):
    """True / False, or "verify" (see above)."""
    global _exemplar_memo
    _exemplar_memo = "verify" if flag == "verify" else ("on" if flag else "off")


# ---- error-aware engine map (r05).  Winograd F(2x2,3x3) rounds 2-3x coarser than the direct sum per layer, and through the
# 31 layers of a frame the timed engine ended up FURTHER from the fp64 truth than the reference's own CPU fp32 (r04 review:
# 216x384, plain seed-0 weights, q999 1.8x / max 2.8x the CPU run's).  `tools/engine_sensitivity.py` measures, per named layer,
# what switching that ONE layer from the direct engine to Winograd does to the frame's ab output (the perturbation field, no
# truth needed) and ranks the layers by perturbation energy per microsecond saved; the layers below are the ones "auto" keeps
# on the direct engine so that the whole path is at or below the CPU fp32 run's error against fp64
# (profiles/r05_engine_sensitivity.txt; asserted by tests/test_gpu_nets.py::test_e2e_error_vs_fp64_oracle_next_to_cpu_fp32).
# Names: "vgg.<conv>", "warp.<head>.<index>" / "warp.layer.<b>.conv<k>", "cvn.<key>" (the reference's state_dict prefixes).
# "speed" is the geometry-only rule (what "auto" meant up to r04), "winograd" / "direct" force one engine.
# DEFAULT_DIRECT_LAYERS: what DVC_DIRECT_LAYERS names (None: unset).
_direct_layers = None      # None: the built-in map (arch.DIRECT_LAYERS); a frozenset: an explicit one


def direct_layers():
    """Names of the layers `auto` keeps on the direct engine."""
    if _direct_layers is not None:
        return _direct_layers
    if DEFAULT_DIRECT_LAYERS is not None:
        return DEFAULT_DIRECT_LAYERS
    from . import arch
    return arch.DIRECT_LAYERS


def set_direct_layers(names=None):
    """Replace the error-aware map (None: back to the built-in one).  Captured launch sequences notice (launch_epoch)."""
    global _direct_layers
    _direct_layers = None if names is None else frozenset(names)


DEFER_REDUCE = 1     # DVC_CONV_DEFER_REDUCE
BATCH_PLAN = 2       # DVC_CONV_BATCH_PLAN
GRAY_INPUT = 4       # DVC_CONV_GRAY_INPUT


class batch_plan:
    """While active, Winograd launches that carry a batch are planned for the WHOLE batch (DVC_CONV_BATCH_PLAN): the images'
    workgroups fill the chip together, so under-filled layers drop (part of) their split over input channels — no partial
    sums, no reduce.  Results are deterministic per batch size but no longer bit-identical to single-image calls (the fp32
    summation order over input channels follows the split).  Off by default: everywhere else a batch of N equals N calls bit
    for bit.  Used by the multi-reference pass (ClipColorizer.set_exemplars -> clip), whose R recurrences must run together, and by
    ClipColorizer(batch_plan=True) for batches of independent clips."""

    def __init__(self, on=True):
        self.on = bool(on)

    def __enter__(self):
        global _batch_plan
        self.prev, _batch_plan = _batch_plan, self.on
        return self

    def __exit__(self, *exc):
        global _batch_plan
        _batch_plan = self.prev


def batch_plan_enabled():
    return _batch_plan


def _plan_flags(N):
    return BATCH_PLAN if (_batch_plan and N > 1) else 0


# ---- autotuning (the analogue of the reference's `cudnn.benchmark = True`, test.py:140): the first
# time a conv geometry is seen, every (tile configuration, split-K) candidate is timed once on the
# real tensors and the fastest is cached for the rest of the process.  Off by default (static cost
# model in the library); `set_autotune(True)` or DVC_AUTOTUNE=1 turns it on.  Tuning synchronises the
# device, so do it during warm-up, never inside a timed or graph-captured region.
_tuned = {}

# optional persistence (DVC_AUTOTUNE_CACHE=<file.json>): tune once, reuse in later processes — e.g. so
# that a profiled run contains production launches only
_cache_path = _os.environ.get("DVC_AUTOTUNE_CACHE")
_cache_loaded = False


def _load_tuned():
    global _cache_loaded
    if _cache_loaded or not _cache_path:
        return
    _cache_loaded = True
    try:
        import json
        with open(_cache_path) as f:
            for k, v in json.load(f).items():
                _tuned[tuple(json.loads(k))] = tuple(v)
    except (OSError, ValueError):
        pass


def _save_tuned():
    if not _cache_path:
        return
    import json
    tmp = _cache_path + ".tmp%d" % _os.getpid()
    with open(tmp, "w") as f:
        json.dump({json.dumps(list(k)): list(v) for k, v in _tuned.items()}, f)
    _os.replace(tmp, _cache_path)


def autotune_table():
    return dict(_tuned)


if _autotune:
    _load_tuned()  # env-enabled autotune: pick up a persisted table


# split-K candidates of the autotuner (DVC_TUNE_SPLITS=1 disables split-K: experiments only)
_TUNE_SPLITS = tuple(int(v) for v in _os.environ.get("DVC_TUNE_SPLITS", "1,2,3,4,6,8").split(","))
_TUNE_STREAMK = tuple((int(a), int(b)) for a, b in (v.split(":") for v in _os.environ.get("DVC_TUNE_STREAMK", "36:2,36:1").split(",") if v))


def _tune_conv(lib, d, tensors):
    """Time every (cfg, split_k) candidate for descriptor `d`; returns the fastest pair."""
    x, w_packed, bias, in_scale, in_shift, in_slope_t, act_slope_t, residual, out = tensors
    if residual is not None and residual.data_ptr() == out.data_ptr():
        # accumulate-in-place call (corr_autograd: d_phi += theta_blk dS): every timing launch would add the product
        # once more into the caller's tensor — time into a scratch output, the caller's launch follows the tuning
        out = torch.empty_like(out)
    ws = _workspace(x.device, CONV_WORKSPACE_BYTES, "conv")
    stream = _stream()

    def launch():
        return lib.dvc_conv2d(ctypes.byref(d), _p(x), _p(w_packed), _p(bias), _p(in_scale), _p(in_shift),
                              _p(in_slope_t), _p(act_slope_t), _p(residual), _p(out),
                              ctypes.c_void_p(ws.data_ptr()), ws.numel(), stream)

    best, best_t = (-1, 0), float("inf")
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def time_it():
        launch()
        e0.record()
        for _ in range(3):
            launch()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    # the library's own choice first: it is the only way to the kernels that are not a (cfg, split_k) of the general engine
    # (the image-input layers, csrc/conv_image.hip)
    d.cfg, d.split_k = -1, 0
    if launch() == 0:
        best, best_t = (-1, 0), time_it()
    # (layers without a fused input transform stage through LDS-DMA; forcing register staging, cfg 16 + k,
    # never won in the per-layer sweep, so it is not a candidate)
    for cfg in (0, 1, 2, 3, 4):
        for sk in _TUNE_SPLITS:
            d.cfg, d.split_k = cfg, sk
            if launch() != 0:          # configuration does not fit this geometry
                break
            t = time_it()
            if t < best_t:
                best, best_t = (cfg, sk), t
    # stream-K decomposition (cfg 32 + tile configuration; plain stride-1 layers only, the call fails cleanly otherwise):
    # 64x64 tiles, 1 or 2 workgroups per CU
    for cfg, per_cu in _TUNE_STREAMK:
        d.cfg, d.split_k = cfg, per_cu
        if launch() != 0:
            continue
        t = time_it()
        if t < best_t:
            best, best_t = (cfg, per_cu), t
    d.cfg, d.split_k = best
    return best


# ---- convolutions
CONV_WORKSPACE_BYTES = 64 << 20   # split-K scratch: up to 8 partial copies of an under-filled layer's output


def pack_conv_weight(w):
    """[Cout][Cin][kh][kw] -> [Cin][kh*kw][Cout] (layout consumed by dvc_conv2d).  Pure data movement."""
    co, ci, kh, kw = w.shape
    return w.detach().permute(1, 2, 3, 0).reshape(ci, kh * kw, co).contiguous()


def conv_out_hw(H, W, ksize=3, stride=1, dil=1, pad=1, in_up=1, in_sub=1):
    vh = H * 2 if in_up == 2 else ((H + 1) // 2 if in_sub == 2 else H)
    vw = W * 2 if in_up == 2 else ((W + 1) // 2 if in_sub == 2 else W)
    ext = dil * (ksize - 1) + 1
    return (vh + 2 * pad - ext) // stride + 1, (vw + 2 * pad - ext) // stride + 1


def _conv_desc(N, Cin, H, W, Cout, *, ksize=3, stride=1, dil=1, pad=None, pad_mode=PAD_ZERO, in_up=1, in_sub=1, act=ACT_NONE,
               act_slope=0.0, in_prelu=False, cfg=-1, split_k=0, x_batch_stride=0, y_batch_stride=0, res_batch_stride=0, flags=0,
               w_batch_stride=0):
    """The one place a DvcConvDesc is filled, by field name.  pad=None: "same" padding, dil * (ksize - 1) / 2 (the 3x3 layers'
    pad == dil).  The batch strides are in elements; 0: densely packed."""
    return DvcConvDesc(N=N, Cin=Cin, H=H, W=W, Cout=Cout, ksize=ksize, stride=stride, dil=dil,
                       pad=dil * (ksize - 1) // 2 if pad is None else pad, pad_mode=pad_mode, in_up=in_up, in_sub=in_sub,
                       act=act, act_slope=float(act_slope), in_prelu=1 if in_prelu else 0, cfg=cfg, split_k=split_k,
                       x_batch_stride=x_batch_stride, y_batch_stride=y_batch_stride, res_batch_stride=res_batch_stride,
                       flags=flags, w_batch_stride=w_batch_stride)


def _record_conv(d, *, affine, in_prelu, residual, algo=None):
    """The conv_record entry of a launch with descriptor `d` (bench.py's roofline and tests/bwd_audit.py read these).  The
    general engine logs no `algo`: readers take a missing one as "direct"."""
    rec = dict(N=d.N, Cin=d.Cin, H=d.H, W=d.W, Cout=d.Cout, ksize=d.ksize, stride=d.stride, dil=d.dil, pad=d.pad,
               pad_mode=d.pad_mode, in_up=d.in_up, in_sub=d.in_sub, affine=affine, in_prelu=in_prelu, residual=residual, act=d.act)
    if algo is not None:
        rec["algo"] = algo
    return rec


def record_layer(layer, Cin, Cout, H, W, *, dil=1, in_up=1, in_sub=1, eligible=True, **extra):
    """Append the layer_record entry of a named 3x3 layer (callers check `layer_record is not None` first)."""
    layer_record.append(dict(layer=layer, Cin=Cin, Cout=Cout, H=H, W=W, dil=dil, in_up=in_up, in_sub=in_sub, eligible=eligible,
                             **extra))


def conv2d(x, w_packed, bias, *, ksize=3, stride=1, dil=1, pad=1, pad_mode=PAD_ZERO, in_up=1, in_sub=1,
           act=ACT_NONE, act_slope=0.0, act_slope_t=None, in_scale=None, in_shift=None, in_slope_t=None,
           residual=None, out=None, out_batch_stride=0, cfg=-1, split_k=0, tune=True, gray_input=False):
    """dvc_conv2d.  x: [N,Cin,H,W]; w_packed: [Cin, k*k, Cout].  `out` may be a channel slice view's
    base pointer tensor (pass `out_batch_stride` in elements).  `tune=False`: the library's static plan even with the
    autotuner on (the layers of the error-aware engine map: ONE summation order, the one the parity tests see).
    `gray_input=True` (VGG19 conv1_1 only, DVC_CONV_GRAY_INPUT): x is [N,1,H,W], the centred luminance; the three input
    channels all read (L + 50) / 100 — gray2rgb_batch folded into the load, bit-identical to gray2rgb(x) followed by this call.
    w_packed [N, Cin, k*k, Cout]: per-image filters (DvcConvDesc.w_batch_stride) — with ksize 1 a batched GEMM
    out[n] = w_packed[n]^T x[n], one launch for the whole batch (the training-side N x N products)."""
    lib = _lib.load()
    x_bs = 0
    if gray_input:
        # (the luminance plane is usually the channel-0 slice of a contiguous [N,3,H,W] Lab tensor: rows contiguous, images
        # 3*H*W apart — the descriptor's batch stride carries that, nothing is copied)
        assert x.dim() == 4 and x.shape[1] == 1 and w_packed.dim() == 3 and w_packed.shape[0] == 3 and cfg == -1 and split_k == 0, \
            (x.shape, w_packed.shape)
        if x.stride(3) != 1 or x.stride(2) != x.shape[3]:
            x = x.contiguous()
        x_bs = x.stride(0) if x.shape[0] > 1 else 0
        if not (isinstance(x, torch.Tensor) and x.is_cuda and x.dtype == torch.float32):
            raise RuntimeError("dvc_amd: `x` must be a float32 ROCm device tensor; no CPU fallback")
    _need_all(x=None if gray_input else x, w_packed=w_packed, bias=bias, in_scale=in_scale, in_shift=in_shift,
              in_slope=in_slope_t, act_slope=act_slope_t, residual=residual)
    N, Cin, H, W = x.shape
    if gray_input:
        Cin, tune = 3, False
    w_bs = 0
    if w_packed.dim() == 4:
        assert w_packed.shape[0] == N, (w_packed.shape, x.shape)
        # (one image: the per-image filter set IS the shared one — no batch stride, so no 16-byte alignment requirement on a
        # filter slice; the one-image-per-call fallbacks of corr_autograd / contextual for odd P*C lean on this)
        w_bs = w_packed[0].numel() if N > 1 else 0
    wshape = tuple(w_packed.shape[-3:])
    assert wshape[0] == Cin and wshape[1] == ksize * ksize, (w_packed.shape, Cin, ksize)
    Cout = wshape[2]
    OH, OW = conv_out_hw(H, W, ksize, stride, dil, pad, in_up, in_sub)
    if out is None:
        out = torch.empty((N, Cout, OH, OW), device=x.device, dtype=torch.float32)
    d = _conv_desc(N, Cin, H, W, Cout, ksize=ksize, stride=stride, dil=dil, pad=pad, pad_mode=pad_mode, in_up=in_up,
                   in_sub=in_sub, act=act, act_slope=act_slope, in_prelu=in_slope_t is not None, cfg=cfg, split_k=split_k,
                   x_batch_stride=x_bs, y_batch_stride=out_batch_stride, flags=GRAY_INPUT if gray_input else 0,
                   w_batch_stride=w_bs)
    if residual is not None:
        assert tuple(residual.shape) == (N, Cout, OH, OW), (residual.shape, (N, Cout, OH, OW))
    if _autotune and tune and cfg == -1 and split_k == 0:
        # (no N in the key and a single-image descriptor for the timing: the library plans per image, so that a batch is
        # bit-identical to single-image calls — the tuned choice must not depend on the batch size either)
        key = (Cin, H, W, Cout, ksize, stride, dil, pad, pad_mode, in_up, in_sub, in_scale is not None,
               in_slope_t is not None, residual is not None, act, x.device.index, w_packed.dim() == 4)
        best = _tuned.get(key)
        if best is None:
            d1 = DvcConvDesc.from_buffer_copy(d)
            d1.N = 1
            best = _tune_conv(lib, d1, (x, w_packed, bias, in_scale, in_shift, in_slope_t, act_slope_t, residual, out))
            _tuned[key] = best
            _save_tuned()
        d.cfg, d.split_k = best
    if conv_record is not None:
        conv_record.append(_record_conv(d, affine=in_scale is not None, in_prelu=in_slope_t is not None,
                                        residual=residual is not None))
    ws = _workspace(x.device, CONV_WORKSPACE_BYTES, "conv")
    _bump_generation(ws)
    rc = lib.dvc_conv2d(ctypes.byref(d), _p(x), _p(w_packed), _p(bias), _p(in_scale), _p(in_shift),
                        _p(in_slope_t), _p(act_slope_t), _p(residual), _p(out),
                        ctypes.c_void_p(ws.data_ptr()), ws.numel(), _stream())
    _lib.check(rc, "dvc_conv2d")
    return out


def ws_eligible(Cin, Cout, dil=1, pad_mode=PAD_ZERO, in_up=1, in_sub=1, act=ACT_NONE):
    """Geometry the weights-in-registers kernel takes (dvc_conv2d_ws_eligible): 3x3 stride 1 pad 1, zero padding, plain input,
    32, 64 or 128 input channels, Cout % 64 == 0."""
    return (Cin in (32, 64, 128) and Cout % 64 == 0 and dil == 1 and pad_mode == PAD_ZERO and in_up == 1 and in_sub == 1
            and act in (ACT_NONE, ACT_RELU, ACT_PRELU, ACT_LEAKY))


def pack_ws_weight(w):
    """[Cout][Cin][3][3] -> the MFMA A-fragment order dvc_conv2d_ws loads (dvc_conv2d_ws_pack_weight), Cout*Cin*9 floats."""
    lib = _lib.load()
    w = w.detach().contiguous().float()
    _need(w, "weight")
    Cout, Cin = w.shape[0], w.shape[1]
    u = torch.empty(Cout * Cin * 9, device=w.device, dtype=torch.float32)
    _lib.check(lib.dvc_conv2d_ws_pack_weight(_p(w), Cout, Cin, _p(u), _stream()), "dvc_conv2d_ws_pack_weight")
    return u


def conv2d_ws(x, u_packed, bias, Cout, *, act=ACT_NONE, act_slope=0.0, act_slope_t=None, out=None, out_batch_stride=0):
    """dvc_conv2d_ws: 3x3 / stride 1 / pad 1 (zero) with the filters resident in registers; see ws_eligible."""
    lib = _lib.load()
    _need_all(x=x, u_packed=u_packed, bias=bias, act_slope=act_slope_t)
    N, Cin, H, W = x.shape
    assert u_packed.numel() == Cout * Cin * 9, (u_packed.shape, Cout, Cin)
    if out is None:
        out = torch.empty((N, Cout, H, W), device=x.device, dtype=torch.float32)
    d = _conv_desc(N, Cin, H, W, Cout, act=act, act_slope=act_slope, y_batch_stride=out_batch_stride)
    if conv_record is not None:
        conv_record.append(_record_conv(d, affine=False, in_prelu=False, residual=False, algo="direct-ws"))
    _lib.check(lib.dvc_conv2d_ws(ctypes.byref(d), _p(x), _p(u_packed), _p(bias), _p(act_slope_t), _p(out), _stream()), "dvc_conv2d_ws")
    return out


def pack_winograd_weight(w):
    """[Cout][Cin][3][3] -> the Winograd F(2x2,3x3) transform-domain filters U = G g G^T in the layout
    dvc_conv2d_winograd stages, [Cout/32][Cin][4][32][4] (dvc_winograd_pack_weight: evaluated in double, rounded once)."""
    lib = _lib.load()
    w = w.detach()
    _need(w, "weight")
    co, ci, kh, kw = w.shape
    assert (kh, kw) == (3, 3) and co % 32 == 0, w.shape
    u = torch.empty((co // 32, ci, 4, 32, 4), device=w.device, dtype=torch.float32)
    assert u.numel() == lib.dvc_winograd_weight_floats(co, ci)
    _lib.check(lib.dvc_winograd_pack_weight(_p(w), co, ci, _p(u), _stream()), "dvc_winograd_pack_weight")
    return u


def winograd_eligible(Cin, Cout, ksize=3, stride=1, dil=1, pad=1, in_affine=False, in_prelu=False):
    """Layers dvc_conv2d_winograd takes (include/dvc_hip.h)."""
    return (ksize == 3 and stride == 1 and dil in (1, 2) and pad == dil and not in_affine and not in_prelu
            and Cin % 8 == 0 and Cout % 64 == 0)


def winograd_selected(N, Cin, H, W, Cout, *, ksize=3, stride=1, dil=1, pad=1, in_up=1, in_sub=1, in_affine=False,
                      in_prelu=False, layer=None):
    """True if the current algorithm choice sends this layer to dvc_conv2d_winograd."""
    if _conv_algo == "direct" or not winograd_eligible(Cin, Cout, ksize, stride, dil, pad, in_affine, in_prelu):
        return False
    if _conv_algo == "winograd":
        return True
    if _conv_algo == "auto" and layer is not None and layer in direct_layers():
        return False
    OH, OW = conv_out_hw(H, W, ksize, stride, dil, pad, in_up, in_sub)
    return _wino_rule(N, Cin, Cout, OH, OW, dil)


def _wino_rule(N, Cin, Cout, OH, OW, dil):
    # measured on the MI355X (profiles/r02_conv_algo_sweep.txt): with the two-workgroups-per-CU shape Winograd is faster than
    # or level with the direct engine on every eligible layer of the network down to the 13x24 feature maps
    # (per image, never a function of the batch size: a batch must run the kernels its images would run alone)
    # (r03 sweep: WarpNet's 128 -> 64 at 54x96 is the one eligible layer where the direct engine is level, 21.9 vs 22.5 us as a
    # launch of its own; since r06 it runs inside the grouped launch of the heads' second convolutions, conv3x3_group, which
    # takes Winograd layers only)
    return OH * OW >= 13 * 24


_conv_ws_generation = {}     # convolution workspace (one per device and stream) -> number of convolutions that have used it


def _bump_generation(ws):
    g = _conv_ws_generation.get(ws.data_ptr(), 0) + 1
    _conv_ws_generation[ws.data_ptr()] = g
    return g


class ConvPartials:
    """What conv2d_winograd(..., defer_reduce=True) returns for a layer that is split over input channels: the partial sums
    [S][N][C][H*W] sitting in the stream's convolution workspace, with the bias / activation still to be applied.  Valid
    until the next convolution on the same stream reuses the workspace; the one consumer is instnorm_apply."""

    def __init__(self, ws, S, shape, bias, act, act_slope, act_slope_t, generation, device, offset=0):
        self.ws, self.S, self.shape, self.bias = ws, S, tuple(shape), bias
        self.act, self.act_slope, self.act_slope_t, self.generation, self.device = act, act_slope, act_slope_t, generation, device
        self.offset = int(offset)       # bytes into the workspace (conv3x3_group: several layers' partial sums side by side)

    def data_ptr(self):
        return self.ws.data_ptr() + self.offset

    def check_live(self):
        if self.generation != _conv_ws_generation.get(self.ws.data_ptr()):
            raise RuntimeError("dvc_amd: the convolution workspace holding these partial sums has been reused by a later "
                               "convolution; instnorm_apply must directly follow conv3x3(defer_reduce=True)")


def _may_defer(act, OH, OW):
    """Launches whose reduce the InstanceNorm launch can take over (dvc_instnorm_apply_partials): planes of at most 16384
    positions and an activation it applies itself."""
    return OH * OW <= 16384 and act in (ACT_NONE, ACT_RELU, ACT_PRELU, ACT_LEAKY)


def _winograd_split(lib, d, workspace_bytes):
    """dvc_conv2d_winograd_split: (split over input channels, images one launch covers) for `d` with that much workspace."""
    sp, ipl = ctypes.c_int32(0), ctypes.c_int32(0)
    _lib.check(lib.dvc_conv2d_winograd_split(ctypes.byref(d), workspace_bytes, ctypes.byref(sp), ctypes.byref(ipl)),
               "dvc_conv2d_winograd_split")
    return sp.value, ipl.value


def conv2d_winograd(x, u_packed, bias, *, dil=1, pad_mode=PAD_ZERO, in_up=1, in_sub=1, act=ACT_NONE, act_slope=0.0,
                    act_slope_t=None, residual=None, out=None, out_batch_stride=0, cfg=-1, split_k=0, defer_reduce=False,
                    ws_tag="conv"):
    """dvc_conv2d_winograd: 3x3, stride 1, pad == dil.  u_packed from pack_winograd_weight.
    defer_reduce=True: if the library splits this layer over input channels, skip the reduce launch and return the
    ConvPartials for instnorm_apply to sum (otherwise the ordinary output tensor).
    `ws_tag`: which of the stream's convolution workspaces to use (conv3x3_group's per-layer fall-back keeps the deferred
    partial sums of several layers alive at once)."""
    lib = _lib.load()
    _need_all(x=x, u_packed=u_packed, bias=bias, act_slope=act_slope_t, residual=residual)
    N, Cin, H, W = x.shape
    assert u_packed.dim() == 5 and u_packed.shape[1] == Cin and tuple(u_packed.shape[2:]) == (4, 32, 4), u_packed.shape
    Cout = u_packed.shape[0] * 32
    OH, OW = conv_out_hw(H, W, 3, 1, dil, dil, in_up, in_sub)
    if out is not None:
        defer_reduce = False
    if residual is not None:
        assert tuple(residual.shape) == (N, Cout, OH, OW), (residual.shape, (N, Cout, OH, OW))
    d = _conv_desc(N, Cin, H, W, Cout, dil=dil, pad_mode=pad_mode, in_up=in_up, in_sub=in_sub, act=act, act_slope=act_slope,
                   cfg=cfg, split_k=split_k, y_batch_stride=out_batch_stride, flags=_plan_flags(N))
    if conv_record is not None:
        conv_record.append(_record_conv(d, affine=False, in_prelu=False, residual=residual is not None, algo="winograd"))
    ws = _workspace(x.device, CONV_WORKSPACE_BYTES, ws_tag)
    generation = _bump_generation(ws)
    S = 1
    if defer_reduce and residual is None and _may_defer(act, OH, OW):
        S, ipl = _winograd_split(lib, d, ws.numel())
        # (a batch the library would cover in several launches - workspace capacity, 65535-workgroup cap - takes the
        # ordinary reduce: the deferred partial sums must be those of the whole batch)
        if S > 1 and ipl >= N and S * N * Cout * OH * OW * 4 <= ws.numel():
            d.flags |= DEFER_REDUCE
        else:
            S = 1
    if S == 1 and out is None:
        out = torch.empty((N, Cout, OH, OW), device=x.device, dtype=torch.float32)
    rc = lib.dvc_conv2d_winograd(ctypes.byref(d), _p(x), _p(u_packed), _p(bias), _p(act_slope_t), _p(residual),
                                 _p(out) if out is not None else ctypes.c_void_p(ws.data_ptr()),
                                 ctypes.c_void_p(ws.data_ptr()), ws.numel(), _stream())
    _lib.check(rc, "dvc_conv2d_winograd")
    if S > 1:
        return ConvPartials(ws, S, (N, Cout, OH, OW), bias, act, float(act_slope), act_slope_t, generation, x.device)
    return out


def conv2d_winograd_pool(x, u_packed, bias, *, act=ACT_NONE, act_slope=0.0, act_slope_t=None, pad_mode=PAD_ZERO, want_full=True):
    """dvc_conv2d_winograd_pool: (act(conv3x3(x)), maxpool2x2 of it) from one convolution launch (+ its reduce when the layer is
    split); the full-resolution tensor is None with want_full=False.  Bit-identical to conv2d_winograd -> maxpool2x2."""
    lib = _lib.load()
    _need_all(x=x, u_packed=u_packed, bias=bias, act_slope=act_slope_t)
    N, Cin, H, W = x.shape
    assert u_packed.dim() == 5 and u_packed.shape[1] == Cin and tuple(u_packed.shape[2:]) == (4, 32, 4), u_packed.shape
    Cout = u_packed.shape[0] * 32
    d = _conv_desc(N, Cin, H, W, Cout, pad_mode=pad_mode, act=act, act_slope=act_slope, flags=_plan_flags(N))
    if conv_record is not None:
        conv_record.append(_record_conv(d, affine=False, in_prelu=False, residual=False, algo="winograd"))
    ws = _workspace(x.device, CONV_WORKSPACE_BYTES, "conv")
    _bump_generation(ws)
    full = torch.empty((N, Cout, H, W), device=x.device, dtype=torch.float32) if want_full else None
    pooled = torch.empty((N, Cout, H // 2, W // 2), device=x.device, dtype=torch.float32)
    _lib.check(lib.dvc_conv2d_winograd_pool(ctypes.byref(d), _p(x), _p(u_packed), _p(bias), _p(act_slope_t), _p(full), _p(pooled), 0,
                                            ctypes.c_void_p(ws.data_ptr()), ws.numel(), _stream()),
               "dvc_conv2d_winograd_pool")
    return full, pooled


def conv2d_winograd_dual(xA, xB, u_cat, bias, *, dil=1, pad_mode=PAD_ZERO, in_upA=1, in_upB=1, act=ACT_NONE, act_slope=0.0,
                         act_slope_t=None):
    """dvc_conv2d_winograd_dual: act(conv3x3(up_A(xA), W_A) + conv3x3(up_B(xB), W_B) + bias) in one launch.  u_cat = the two
    packed filter sets concatenated along Cin (torch.cat((pack(W_A), pack(W_B)), dim=1)), bias = b_A + b_B."""
    lib = _lib.load()
    _need_all(xA=xA, xB=xB, u_cat=u_cat, bias=bias, act_slope=act_slope_t)
    N, CA, HA, WA = xA.shape
    NB, CB, HB, WB = xB.shape
    assert N == NB and u_cat.dim() == 5 and u_cat.shape[1] == CA + CB and tuple(u_cat.shape[2:]) == (4, 32, 4), (xA.shape, xB.shape, u_cat.shape)
    Cout = u_cat.shape[0] * 32
    OH, OW = conv_out_hw(HA, WA, 3, 1, dil, dil, in_upA, 1)
    if (OH, OW) != conv_out_hw(HB, WB, 3, 1, dil, dil, in_upB, 1):
        raise RuntimeError(f"dvc_amd: conv2d_winograd_dual: the two inputs' virtual sizes differ ({HA * in_upA} x {WA * in_upA} vs "
                           f"{HB * in_upB} x {WB * in_upB})")
    common = dict(dil=dil, pad_mode=pad_mode, act=act, act_slope=act_slope)
    dA = _conv_desc(N, CA, HA, WA, Cout, in_up=in_upA, flags=_plan_flags(N), **common)
    dB = _conv_desc(N, CB, HB, WB, Cout, in_up=in_upB, **common)
    if conv_record is not None:
        # (ONE record for the pair: the virtual size both inputs share and the summed input channels)
        conv_record.append(_record_conv(_conv_desc(N, CA + CB, OH, OW, Cout, **common), affine=False, in_prelu=False,
                                        residual=False, algo="winograd-dual"))
    ws = _workspace(xA.device, CONV_WORKSPACE_BYTES, "conv")
    _bump_generation(ws)
    out = torch.empty((N, Cout, OH, OW), device=xA.device, dtype=torch.float32)
    _lib.check(lib.dvc_conv2d_winograd_dual(ctypes.byref(dA), ctypes.byref(dB), _p(xA), _p(xB), _p(u_cat), _p(bias), _p(act_slope_t),
                                            _p(out), ctypes.c_void_p(ws.data_ptr()), ws.numel(), _stream()),
               "dvc_conv2d_winograd_dual")
    return out


def conv3x3(x, weight, packs, bias, *, dil=1, pad_mode=PAD_ZERO, in_up=1, in_sub=1, act=ACT_NONE, act_slope=0.0,
            act_slope_t=None, residual=None, out=None, out_batch_stride=0, defer_reduce=False, layer=None, ws_tag="conv"):
    """A 3x3 stride-1 pad == dil layer through whichever engine the algorithm choice selects.  `packs(kind)` returns
    the packed weight for kind "direct" ([Cin][9][Cout]) or "winograd" (U = G g G^T), normally from a _PackCache.
    `layer`: the layer's name in the error-aware engine map (direct_layers)."""
    N, Cin, H, W = x.shape
    Cout = weight.shape[0]
    if layer_record is not None:
        record_layer(layer, Cin, Cout, H, W, dil=dil, in_up=in_up, in_sub=in_sub,
                     eligible=winograd_eligible(Cin, Cout, 3, 1, dil, dil)
                     and _wino_rule(N, Cin, Cout, *conv_out_hw(H, W, 3, 1, dil, dil, in_up, in_sub), dil))
    if winograd_selected(N, Cin, H, W, Cout, dil=dil, pad=dil, in_up=in_up, in_sub=in_sub, layer=layer):
        return conv2d_winograd(x, packs("winograd"), bias, dil=dil, pad_mode=pad_mode, in_up=in_up, in_sub=in_sub,
                               act=act, act_slope=act_slope, act_slope_t=act_slope_t, residual=residual, out=out,
                               out_batch_stride=out_batch_stride, defer_reduce=defer_reduce and _fuse_reduce, ws_tag=ws_tag)
    if _ws_conv and residual is None and ws_eligible(Cin, Cout, dil, pad_mode, in_up, in_sub, act):
        return conv2d_ws(x, packs("ws"), bias, Cout, act=act, act_slope=act_slope, act_slope_t=act_slope_t, out=out,
                         out_batch_stride=out_batch_stride)
    # (a layer the error-aware map names keeps the library's static plan whatever the autotuner would pick: with the chaotic
    # random weights another split over input channels in ColorVidNet's first layers re-draws the tail of the frame's error
    # field — profiles/r06_parity_pool_probe.txt — and the parity the tests assert must be the parity of the timed run)
    return conv2d(x, packs("direct"), bias, dil=dil, pad=dil, pad_mode=pad_mode, in_up=in_up, in_sub=in_sub, act=act,
                  act_slope=act_slope, act_slope_t=act_slope_t, residual=residual, out=out,
                  out_batch_stride=out_batch_stride, tune=not (_conv_algo == "auto" and layer is not None and layer in direct_layers()))


def _item_is_winograd(it):
    """winograd_selected for an item of conv3x3_group."""
    N, Cin, H, W = it["x"].shape
    dil = it.get("dil", 1)
    return winograd_selected(N, Cin, H, W, it["weight"].shape[0], dil=dil, pad=dil, in_up=it.get("in_up", 1),
                             in_sub=it.get("in_sub", 1), layer=it.get("layer"))


def conv3x3_group(items):
    """`items`: list of dicts with the arguments of conv3x3 (x, weight, packs, bias + keywords) for INDEPENDENT layers.  Returns
    the list of their results (tensors, or ConvPartials where `defer_reduce` applies), each bit-identical to its own conv3x3
    call.  One launch for all of them when grouping is on and every item goes to the Winograd engine
    (dvc_conv2d_winograd_group); otherwise the per-layer calls, in order."""
    def single(it, i=0):
        # (per-layer launches: the items' deferred partial sums must all be alive when the caller's next stage consumes them,
        # so every item but the first gets a convolution workspace of its own — same size, hence the same plan)
        # (the first keeps the stream's own workspace unless a later item runs on the direct engine, which always uses — and so
        # invalidates — that one: WarpNet's heads at 64x96, where layer3_1 is a Winograd layer and layer4_1 / layer5_1 are not)
        kw = {k: v for k, v in it.items() if k not in ("x", "weight", "packs", "bias")}
        own = i > 0 or not all(_item_is_winograd(o) for o in items[1:])
        return conv3x3(it["x"], it["weight"], it["packs"], it["bias"], ws_tag=f"conv.g{i}" if own else "conv", **kw)

    n = len(items)
    if not (_group_heads and 2 <= n <= 4 and all(it.get("out") is None and it.get("residual") is None and _item_is_winograd(it)
                                                 for it in items)):
        return [single(it, i) for i, it in enumerate(items)]
    lib = _lib.load()
    dev = items[0]["x"].device
    ws = _workspace(dev, CONV_WORKSPACE_BYTES, "conv")
    arr = (DvcConvGroupItem * n)()
    meta = []
    off = 0
    for i, it in enumerate(items):
        x, bias = it["x"], it["bias"]
        u = it["packs"]("winograd")
        act_slope_t = it.get("act_slope_t")
        _need_all(x=x, u_packed=u, bias=bias, act_slope=act_slope_t)
        N, Cin, H, W = x.shape
        Cout = u.shape[0] * 32
        dil, in_up, in_sub = it.get("dil", 1), it.get("in_up", 1), it.get("in_sub", 1)
        act, act_slope = it.get("act", ACT_NONE), float(it.get("act_slope", 0.0))
        OH, OW = conv_out_hw(H, W, 3, 1, dil, dil, in_up, in_sub)
        d = _conv_desc(N, Cin, H, W, Cout, dil=dil, pad_mode=it.get("pad_mode", PAD_ZERO), in_up=in_up, in_sub=in_sub, act=act,
                       act_slope=act_slope, flags=_plan_flags(N))
        if layer_record is not None:
            record_layer(it.get("layer"), Cin, Cout, H, W, dil=dil, in_up=in_up, in_sub=in_sub)
        if conv_record is not None:
            conv_record.append(_record_conv(d, affine=False, in_prelu=False, residual=False, algo="winograd"))
        # the split this layer gets ALONE (whole workspace): the grouped launch must reproduce it from this item's share
        S, ipl = _winograd_split(lib, d, ws.numel())
        need = (S * N * Cout * OH * OW * 4 + 255) // 256 * 256 if S > 1 else 0
        room = ws.numel() - off
        S2, ipl2 = _winograd_split(lib, d, max(room, 0))
        if need > room or S2 != S or ipl < N or ipl2 < N:
            return [single(it_, j) for j, it_ in enumerate(items)]   # (the workspace cannot hold the items' partial sums side by side)
        defer = it.get("defer_reduce", False) and _fuse_reduce and S > 1 and _may_defer(act, OH, OW)
        if defer:
            d.flags |= DEFER_REDUCE
        out = None if defer else torch.empty((N, Cout, OH, OW), device=dev, dtype=torch.float32)
        a = arr[i]
        a.d = d
        a.x, a.u_packed, a.bias, a.act_slope_ptr, a.residual = x.data_ptr(), u.data_ptr(), _pv(bias), _pv(act_slope_t), None
        a.y = ws.data_ptr() + off if out is None else out.data_ptr()
        a.workspace, a.workspace_bytes = ws.data_ptr() + off, room
        meta.append((out, S, (N, Cout, OH, OW), bias, act, act_slope, act_slope_t, off, u))
        off += need
    generation = _bump_generation(ws)
    _lib.check(lib.dvc_conv2d_winograd_group(arr, n, _stream()), "dvc_conv2d_winograd_group")
    return [out if out is not None else ConvPartials(ws, S, shape, bias, act, act_slope, act_slope_t, generation, dev, offset=o)
            for (out, S, shape, bias, act, act_slope, act_slope_t, o, _u) in meta]


def conv1x1_small(x, w, bias, act=ACT_NONE):
    lib = _lib.load()
    _need_all(x=x, w=w, bias=bias)
    N, Cin, H, W = x.shape
    Cout = w.shape[0]
    y = torch.empty((N, Cout, H, W), device=x.device, dtype=torch.float32)
    _lib.check(lib.dvc_conv1x1_small(_p(x), _p(w), _p(bias), N, Cin, H * W, Cout, act, _p(y), _stream()),
               "dvc_conv1x1_small")
    return y


# ---- norms and pools
def instnorm_stats(x, eps=1e-5, chan_scale=None):
    """Returns (scale, shift), each [N*C], such that InstanceNorm(x) == x*scale + shift per plane."""
    lib = _lib.load()
    _need_all(x=x, chan_scale=chan_scale)
    N, C, H, W = x.shape
    scale = torch.empty(N * C, device=x.device, dtype=torch.float32)
    shift = torch.empty(N * C, device=x.device, dtype=torch.float32)
    _lib.check(lib.dvc_instnorm_stats(_p(x), N, C, H * W, 0, float(eps), _p(chan_scale), _p(scale), _p(shift),
                                      _stream()), "dvc_instnorm_stats")
    return scale, shift


def affine_act(x, scale, shift, *, residual=None, slope_t=None, up=1, rpad=0, out=None, out_batch_stride=0):
    lib = _lib.load()
    _need_all(x=x, scale=scale, shift=shift, residual=residual, slope=slope_t)
    N, C, H, W = x.shape
    if out is None:
        out = torch.empty((N, C, H * up + 2 * rpad, W * up), device=x.device, dtype=torch.float32)
    _lib.check(lib.dvc_affine_act(_p(x), _p(scale), _p(shift), _p(residual), _p(slope_t), N, C, H, W, up, rpad,
                                  0, 0, out_batch_stride, _p(out), _stream()), "dvc_affine_act")
    return out


def _instnorm_prep(x, chan_scale, residual, slope_t, up, sub, rpad, out):
    """What instnorm_apply and instnorm_apply_group do before they launch: x is a tensor or the ConvPartials of a deferred
    reduce (checked to be alive); returns (partials or None, N, C, H, W, device, the output tensor — allocated if `out` is None)."""
    part = x if isinstance(x, ConvPartials) else None
    if part is not None:
        part.check_live()
    _need_all(x=None if part is not None else x, chan_scale=chan_scale, residual=residual, slope=slope_t)
    N, C, H, W = part.shape if part is not None else x.shape
    dev = part.device if part is not None else x.device
    VH, VW = ((H + 1) // 2, (W + 1) // 2) if sub == 2 else (H * up, W * up)
    if out is None:
        out = torch.empty((N, C, VH + 2 * rpad, VW), device=dev, dtype=torch.float32)
    return part, N, C, H, W, dev, out


def instnorm_apply(x, *, eps=1e-5, chan_scale=None, residual=None, slope_t=None, up=1, sub=1, rpad=0, out=None,
                   out_batch_stride=0, second=None, scale_out=None):
    """InstanceNorm2d (no affine, biased variance) + optional depthwise scale / skip-add / PReLU / nearest
    upsample / stride-2 subsample / replicate row pad, in one launch; `out=x` normalises in place.
    `second=(chan_scale2, sub2)` also returns InstanceNorm(x) * chan_scale2 at stride sub2 (same statistics,
    same launch): the call then returns (y, y2).  `scale_out` [N*C] receives the per-plane scale, rstd * chan_scale
    (the training path of ColorVidNet keeps rstd for its backward)."""
    lib = _lib.load()
    assert not isinstance(out, ConvPartials)
    part, N, C, H, W, dev, out = _instnorm_prep(x, chan_scale, residual, slope_t, up, sub, rpad, out)
    cs2, sub2, y2 = None, 1, None
    if second is not None:
        cs2, sub2 = second
        _need(cs2, "chan_scale2")
        y2 = torch.empty((N, C, (H + 1) // 2, (W + 1) // 2) if sub2 == 2 else (N, C, H, W), device=dev,
                         dtype=torch.float32)
    if part is not None:
        assert scale_out is None, "scale_out: materialise the convolution's output first (defer_reduce=False)"
        _lib.check(lib.dvc_instnorm_apply_partials(ctypes.c_void_p(part.data_ptr()), part.S, _p(part.bias), part.act,
                                                   part.act_slope, _p(part.act_slope_t), _p(residual), _p(slope_t),
                                                   _p(chan_scale), float(eps), N, C, H, W, up, sub, rpad, 0, out_batch_stride,
                                                   _p(out), None, None, _p(cs2), sub2, _p(y2), _stream()),
                   "dvc_instnorm_apply_partials")
        return out if second is None else (out, y2)
    shift_out = None
    if scale_out is not None:
        _need(scale_out, "scale_out")
        assert scale_out.numel() == N * C, (scale_out.shape, N, C)
        shift_out = torch.empty_like(scale_out)
    _lib.check(lib.dvc_instnorm_apply(_p(x), _p(residual), _p(slope_t), _p(chan_scale), float(eps), N, C, H, W, up,
                                      sub, rpad, 0, 0, out_batch_stride, _p(out), _p(scale_out), _p(shift_out), _p(cs2), sub2,
                                      _p(y2), _stream()),
               "dvc_instnorm_apply")
    return out if second is None else (out, y2)


def instnorm_apply_group(items):
    """`items`: list of dicts {x: tensor | ConvPartials, + the keywords of instnorm_apply except `second`} for INDEPENDENT
    norms.  Returns the list of outputs, bit-identical to the per-item instnorm_apply calls; one launch when grouping is on."""
    n = len(items)
    if not (_group_heads and 2 <= n <= 4):
        return [instnorm_apply(it["x"], **{k: v for k, v in it.items() if k != "x"}) for it in items]
    lib = _lib.load()
    arr = (DvcInstNormItem * n)()
    outs = []
    for i, it in enumerate(items):
        x = it["x"]
        residual, slope_t, chan_scale = it.get("residual"), it.get("slope_t"), it.get("chan_scale")
        up, sub, rpad = it.get("up", 1), it.get("sub", 1), it.get("rpad", 0)
        part, N, C, H, W, _dev, out = _instnorm_prep(x, chan_scale, residual, slope_t, up, sub, rpad, it.get("out"))
        a = arr[i]
        a.x = part.data_ptr() if part is not None else x.data_ptr()
        a.S = part.S if part is not None else 0
        a.bias = _pv(part.bias) if part is not None else None
        a.act = part.act if part is not None else ACT_NONE
        a.act_slope = part.act_slope if part is not None else 0.0
        a.act_slope_ptr = _pv(part.act_slope_t) if part is not None else None
        a.residual, a.slope_ptr, a.chan_scale = _pv(residual), _pv(slope_t), _pv(chan_scale)
        a.eps = float(it.get("eps", 1e-5))
        a.N, a.C, a.H, a.W, a.up, a.sub, a.rpad = N, C, H, W, up, sub, rpad
        a.x_batch_stride, a.res_batch_stride, a.y_batch_stride = 0, 0, it.get("out_batch_stride", 0)
        a.y = out.data_ptr()
        outs.append(out)
    _lib.check(lib.dvc_instnorm_apply_group(arr, n, _stream()), "dvc_instnorm_apply_group")
    return outs


def _pool(fn_name, x, k):
    lib = _lib.load()
    _need(x, "x")
    N, C, H, W = x.shape
    y = torch.empty((N, C, H // k, W // k), device=x.device, dtype=torch.float32)
    _lib.check(getattr(lib, fn_name)(_p(x), N * C, H, W, _p(y), _stream()), fn_name)
    return y


def maxpool2x2(x):
    return _pool("dvc_maxpool2x2", x, 2)


def avgpool2x2(x):
    return _pool("dvc_avgpool2x2", x, 2)


def avgpool4x4(x):
    return _pool("dvc_avgpool4x4", x, 4)


def upsample_nearest(x, f):
    lib = _lib.load()
    _need(x, "x")
    N, C, H, W = x.shape
    y = torch.empty((N, C, H * f, W * f), device=x.device, dtype=torch.float32)
    _lib.check(lib.dvc_upsample_nearest(_p(x), N * C, H, W, f, _p(y), _stream()), "dvc_upsample_nearest")
    return y


def channel_l2norm(x, eps=EPS64):
    lib = _lib.load()
    _need(x, "x")
    N, C, H, W = x.shape
    y = torch.empty_like(x)
    _lib.check(lib.dvc_channel_l2norm(_p(x), N, C, H * W, float(eps), _p(y), _stream()), "dvc_channel_l2norm")
    return y


def channel_l2norm_multi(xs, eps=EPS64):
    """feature_normalize of several feature maps of one batch in ONE launch (dvc_channel_l2norm_multi); falls back to one
    launch per map when a map's H*W is not a multiple of 4."""
    lib = _lib.load()
    xs = list(xs)
    for i, x in enumerate(xs):
        _need(x, f"x[{i}]")
    N = xs[0].shape[0]
    # (the one-launch kernel moves float4 pieces: every plane size a multiple of 4 and every base pointer 16-byte aligned —
    # an offset or sliced feature tensor takes the per-map scalar kernel, as it did before the multi entry existed)
    if len(xs) > 8 or any(x.shape[0] != N or (x.shape[2] * x.shape[3]) % 4 or x.data_ptr() % 16 for x in xs):
        return [channel_l2norm(x, eps) for x in xs]
    ys = [torch.empty_like(x) for x in xs]
    n = len(xs)
    px = (ctypes.c_void_p * n)(*[x.data_ptr() for x in xs])
    py = (ctypes.c_void_p * n)(*[y.data_ptr() for y in ys])
    cs = (ctypes.c_int32 * n)(*[x.shape[1] for x in xs])
    hw = (ctypes.c_int32 * n)(*[x.shape[2] * x.shape[3] for x in xs])
    _lib.check(lib.dvc_channel_l2norm_multi(ctypes.cast(px, ctypes.c_void_p), ctypes.cast(py, ctypes.c_void_p),
                                            ctypes.cast(cs, ctypes.c_void_p), ctypes.cast(hw, ctypes.c_void_p), n, N,
                                            float(eps), _stream()), "dvc_channel_l2norm_multi")
    return ys


# ---- colour
def gray2rgb(l):
    """l: [N,1,H,W] (may be the channel-0 slice of a contiguous [N,3,H,W] Lab tensor)."""
    lib = _lib.load()
    if not (isinstance(l, torch.Tensor) and l.is_cuda and l.dtype == torch.float32):
        raise RuntimeError("dvc_amd: `l` must be a float32 ROCm device tensor; no CPU fallback")
    N, C, H, W = l.shape
    assert C == 1
    if l.stride(3) != 1 or l.stride(2) != W:
        l = l.contiguous()
    bs = l.stride(0) if N > 1 else H * W
    y = torch.empty((N, 3, H, W), device=l.device, dtype=torch.float32)
    _lib.check(lib.dvc_gray2rgb(_p(l), N, H * W, bs, _p(y), _stream()), "dvc_gray2rgb")
    return y


def lab2rgb(lab, l_offset=0.0):
    lib = _lib.load()
    _need(lab, "lab")
    N, C, H, W = lab.shape
    assert C == 3
    y = torch.empty_like(lab)
    _lib.check(lib.dvc_lab2rgb(_p(lab), N, H * W, float(l_offset), _p(y), _stream()), "dvc_lab2rgb")
    return y


def _plane(t, ch, name):
    """(pointer, batch stride in elements) of channels ch.. of an [N,C,H,W] fp32 device tensor whose planes are dense
    (a contiguous tensor, or a channel slice of one)."""
    if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float32 and t.dim() == 4):
        raise RuntimeError(f"dvc_amd: `{name}` must be a 4-d float32 ROCm device tensor; no CPU fallback")
    if t.device.index != _current_device():
        raise RuntimeError(f"dvc_amd: `{name}` lives on {t.device} but the current device is cuda:{_current_device()}")
    N, C, H, W = t.shape
    if t.stride(3) != 1 or t.stride(2) != W or (C > 1 and t.stride(1) != H * W):
        raise RuntimeError(f"dvc_amd: `{name}` must have dense planes (a contiguous tensor or a channel slice of one)")
    # (an expanded tensor — one frame seen as R images, ClipColorizer._rep — has batch stride 0, which the C-ABI spells -1:
    # 0 is its "densely packed" default)
    return ctypes.c_void_p(t.data_ptr() + 4 * ch * H * W), ((t.stride(0) or -1) if N > 1 else C * H * W)


def _pack_planes(IA_lab, IA_last_lab, last_l, last_ab, out):
    """The planes pack_color_input reads and the [N,7,H,W] tensor it writes (`out`, or a new one): returns
    ((ia, ia_bs), (ll, ll_bs), (la, la_bs), y) — current luminance, previous luminance, previous ab as _plane pairs."""
    N, _, H, W = IA_lab.shape
    ia = _plane(IA_lab, 0, "IA_lab")
    if IA_last_lab is not None:
        ll = _plane(IA_last_lab, 0, "IA_last_lab")
        la = _plane(IA_last_lab, 1, "IA_last_lab")
    else:
        ll = _plane(last_l, 0, "last_l")
        la = _plane(last_ab, 0, "last_ab")
        assert last_ab.shape[1] == 2
    if out is not None:
        _need(out, "out")
        if tuple(out.shape) != (N, 7, H, W) or out.device != IA_lab.device:
            raise RuntimeError(f"dvc_amd: pack_color_input: `out` must be a contiguous float32 [{N}, 7, {H}, {W}] tensor on "
                               f"{IA_lab.device} (got {tuple(out.shape)} on {out.device})")
    y = torch.empty((N, 7, H, W), device=IA_lab.device, dtype=torch.float32) if out is None else out
    return ia, ll, la, y


def pack_color_input(IA_lab, warped_lab, sim, IA_last_lab=None, *, last_l=None, last_ab=None, out=None, want_warped=False):
    """cat((IA_l, warped ab, similarity, IA_last_lab), 1)  (FrameColor.py:63-64).  IA_lab: the current frame (channel 0 is
    read; a Lab tensor or its [:, 0:1] slice).  The previous frame is either `IA_last_lab` [N,3,H,W] or its two parts
    `last_l` (a tensor whose channel 0 is the previous luminance, e.g. the previous Lab frame) and `last_ab` [N,2,H,W] — the
    clip loop passes the parts and never builds test.py:96's cat.  `out`: an existing [N,7,H,W] tensor (graph replay).
    `warped_lab` may be the CorrPartials of a deferred corr_fwd (`sim` is then None): this launch merges them (same arithmetic
    as the merge inside corr_fwd, bit-identical values); want_warped=True additionally materialises the warped Lab
    [N,3,H,W] (what FrameColor.py:41-67 returns) and the call returns (y, warped_lab)."""
    lib = _lib.load()
    if isinstance(warped_lab, CorrPartials):
        return _merge_pack(lib, IA_lab, warped_lab, IA_last_lab, last_l, last_ab, out, want_warped)
    _need_all(warped_lab=warped_lab, sim=sim)
    N, _, H, W = IA_lab.shape
    (ia, ia_bs), (ll, ll_bs), (la, la_bs), y = _pack_planes(IA_lab, IA_last_lab, last_l, last_ab, out)
    _lib.check(lib.dvc_pack_color_input(ia, ia_bs, _p(warped_lab), _p(sim), ll, ll_bs, la, la_bs, N, H * W, _p(y),
                                        _stream()), "dvc_pack_color_input")
    return (y, warped_lab) if want_warped else y


def _merge_pack(lib, IA_lab, part, IA_last_lab, last_l, last_ab, out, want_warped):
    """pack_color_input for the CorrPartials of a deferred corr_fwd: one dvc_corr_merge_pack launch per image."""
    N, _, H, W = IA_lab.shape
    if N != len(part.bufs) or (H, W) != (4 * part.h, 4 * part.w):
        raise RuntimeError(f"dvc_amd: pack_color_input: frame {tuple(IA_lab.shape)} does not fit the correlation's {len(part.bufs)} x "
                           f"{part.h} x {part.w} partial states")
    HW = H * W
    # (the fused launch moves float4 pieces: a view whose planes do not start on 16 bytes — an odd storage offset — is copied
    # once; fresh allocations and whole tensors never are)
    al = lambda t: t if t is None or (t.data_ptr() % 16 == 0 and (t.stride(0) * 4) % 16 == 0) else t.clone(memory_format=torch.contiguous_format)  # noqa: E731
    # (bound to locals: _pack_planes hands back raw addresses, so the copies must live until the launches below are queued)
    IA_lab, IA_last_lab, last_l, last_ab = al(IA_lab), al(IA_last_lab), al(last_l), al(last_ab)
    (ia, ia_bs), (ll, ll_bs), (la, la_bs), y = _pack_planes(IA_lab, IA_last_lab, last_l, last_ab, out)
    warped = torch.empty((N, 3, H, W), device=IA_lab.device, dtype=torch.float32) if want_warped else None
    step = lambda bs: 0 if bs < 0 else 4 * bs           # noqa: E731  (bytes between images; -1 = the same plane for all)
    st = _stream()
    for n in range(N):
        _lib.check(lib.dvc_corr_merge_pack(ctypes.c_void_p(part.bufs[n].data_ptr()), part.bufs[n].numel(), part.temperature,
                                           part.h, part.w, ctypes.c_void_p(ia.value + n * step(ia_bs)),
                                           ctypes.c_void_p(ll.value + n * step(ll_bs)), ctypes.c_void_p(la.value + n * step(la_bs)),
                                           ctypes.c_void_p(y.data_ptr() + n * 7 * HW * 4),
                                           None if warped is None else ctypes.c_void_p(warped.data_ptr() + n * 3 * HW * 4),
                                           None, st), "dvc_corr_merge_pack")
    return (y, warped) if want_warped else y


# ---- correlation
def corr_prepare_with_mean(t_raw, eps=EPS64):
    """corr_prepare, also returning the per-(image, channel) means [B*C] the launch computes (the backward's centre)."""
    lib = _lib.load()
    _need(t_raw, "t_raw")
    B, C = t_raw.shape[0], t_raw.shape[1]
    P = t_raw[0, 0].numel()
    out = torch.empty((B, C, P), device=t_raw.device, dtype=torch.float32)
    mean = torch.empty(B * C, device=t_raw.device, dtype=torch.float32)
    _lib.check(lib.dvc_corr_prepare(_p(t_raw), B, C, P, float(eps), _p(mean), _p(out), _stream()), "dvc_corr_prepare")
    return out, mean


def corr_prepare(t_raw, eps=EPS64):
    """t_raw: [B,C,h,w] or [B,C,P] output of the theta/phi 1x1 conv -> centred + normalised [B,C,P]."""
    return corr_prepare_with_mean(t_raw, eps)[0]


class CorrPartials:
    """What corr_fwd(..., defer_merge=True) returns: the per-workgroup partial softmax states of B images (one private
    buffer per image), still to be merged.  The one consumer is pack_color_input, whose launch then merges them and writes the
    warped colours / similarity map straight into ColorVidNet's 7-channel input (dvc_corr_merge_pack) — no warped-Lab /
    similarity tensors, no merge launch, no separate pack launch."""

    def __init__(self, bufs, h, w, temperature):
        self.bufs, self.h, self.w, self.temperature = list(bufs), h, w, float(temperature)
        self.shape = (len(self.bufs), 3, 4 * h, 4 * w)      # of the warped Lab it stands for

    def record_stream(self, stream):
        for b in self.bufs:
            b.record_stream(stream)

    def copy_(self, other):
        for a, b in zip(self.bufs, other.bufs):
            a.copy_(b)
        return self


def _corr_outputs(B, h, w, dev, want_up, want_small, want_argmax):
    """The result dict of corr_fwd / corr_fwd_bf16 with the requested outputs allocated for B images (the others None)."""
    def new(*shape, dtype=torch.float32):
        return torch.empty((B,) + shape, device=dev, dtype=dtype)
    return dict(y_up=new(3, 4 * h, 4 * w) if want_up else None, sim_up=new(1, 4 * h, 4 * w) if want_up else None,
                y_small=new(3, h, w) if want_small else None, sim_small=new(1, h, w) if want_small else None,
                argmax=new(h * w, dtype=torch.int32) if want_argmax else None)


def _corr_out_args(out, sl):
    """The five output arguments of dvc_corr_fwd / dvc_corr_fwd_bf16, in the C-ABI's order, for the images `sl` of `out`."""
    return [None if out[k] is None else ctypes.c_void_p(out[k][sl].data_ptr())
            for k in ("y_small", "sim_small", "y_up", "sim_up", "argmax")]


def corr_fwd(theta, phi, blab, temperature, h, w, wta_scale=1.0, want_small=False, want_argmax=False,
             want_up=True, defer_merge=False):
    """Fused affinity + softmax + colour gather.  theta/phi: [B,256,P]; blab: [B,3,P] (P = h*w).
    Returns dict with y_up [B,3,4h,4w], sim_up [B,1,4h,4w] and optionally y_small / sim_small / argmax.
    Batch forms: paired (theta, phi, blab all [B]); one exemplar for B frames (phi / blab [1]: the clip driver's batched
    front ends); ONE FRAME AGAINST R EXEMPLARS (theta [1], phi / blab [R]: the references of a clip colourised in one pass,
    test.py:169-181) — outputs then have R images.  The library runs one image per set of launches in every form, so an
    image's result never depends on the form it came in.
    defer_merge=True (wta_scale == 1, no small / arg-max outputs): the merge of the partial softmax states is left to the
    consumer — returns the CorrPartials for pack_color_input instead of the dict."""
    lib = _lib.load()
    _need_all(theta=theta, phi=phi, blab=blab)
    Bt, C, P = theta.shape
    R = phi.shape[0]
    if defer_merge and (wta_scale != 1.0 or want_small or want_argmax):
        defer_merge = False
    shared = Bt > 1 and R == 1 and blab.shape[0] == 1        # one exemplar for a batch of frames (clip driver)
    refs = Bt == 1 and R > 1 and blab.shape[0] == R          # one frame against R exemplars
    B = max(Bt, R)
    assert P == h * w and tuple(phi.shape[1:]) == (C, P) and blab[0].numel() == 3 * P
    assert shared or refs or (R == Bt and blab.shape[0] == Bt), (theta.shape, phi.shape, blab.shape)
    if not (temperature > 0):
        raise ValueError("temperature must be > 0")
    dev = theta.device
    if defer_merge:
        # one private partial-state buffer per image (2 MB at 54x96): the consumer may run on another stream, later
        nb1 = lib.dvc_corr_workspace_bytes(1, P)
        bufs = [torch.empty(nb1, device=dev, dtype=torch.uint8) for _ in range(B)]
        st = _stream()
        for b in range(B):
            th, ph, bl = theta[b if Bt > 1 else 0], phi[b if R > 1 else 0], blab[b if blab.shape[0] > 1 else 0]
            _lib.check(lib.dvc_corr_fwd(_p(th), _p(ph), _p(bl), float(temperature), 1.0, 1, C, h, w, None, None, None, None, None,
                                        ctypes.c_void_p(bufs[b].data_ptr()), bufs[b].numel(), st), "dvc_corr_fwd")
        return CorrPartials(bufs, h, w, temperature)
    if not (want_up or want_small or want_argmax):
        # (at the C-ABI "every output NULL" means a deferred merge: never reach it by accident)
        raise ValueError("dvc_amd: corr_fwd: no output requested (want_up / want_small / want_argmax all False); pass "
                         "defer_merge=True to leave the merge to pack_color_input")
    out = _corr_outputs(B, h, w, dev, want_up, want_small, want_argmax)
    nbytes = lib.dvc_corr_workspace_bytes(1 if (shared or refs) else B, P)
    ws = _workspace(dev, nbytes)

    def call(th, ph, bl, nb, sl):
        rc = lib.dvc_corr_fwd(_p(th), _p(ph), _p(bl), float(temperature), float(wta_scale), nb, C, h, w, *_corr_out_args(out, sl),
                              ctypes.c_void_p(ws.data_ptr()), ws.numel(), _stream())
        _lib.check(rc, "dvc_corr_fwd")

    if shared:      # the library runs one image per set of launches anyway (results independent of the batch size)
        for b in range(B):
            call(theta[b:b + 1], phi, blab, 1, slice(b, b + 1))
    elif refs:
        for r in range(R):
            call(theta, phi[r:r + 1], blab[r:r + 1], 1, slice(r, r + 1))
    else:
        call(theta, phi, blab, B, slice(0, B))
    return out


def corr_prepare_bf16(t_raw, eps=EPS64):
    """t_raw [B,C,h,w] or [B,C,P] -> (fp32 [B,P,C], bf16 [B,P,C] stored as int16) centred + normalised."""
    lib = _lib.load()
    _need(t_raw, "t_raw")
    B, C = t_raw.shape[0], t_raw.shape[1]
    P = t_raw[0, 0].numel()
    f32 = torch.empty((B, P, C), device=t_raw.device, dtype=torch.float32)
    b16 = torch.empty((B, P, C), device=t_raw.device, dtype=torch.int16)
    mean = torch.empty(B * C, device=t_raw.device, dtype=torch.float32)
    _lib.check(lib.dvc_corr_prepare_bf16(_p(t_raw), B, C, P, float(eps), _p(mean), _p(f32),
                                         ctypes.c_void_p(b16.data_ptr()), _stream()), "dvc_corr_prepare_bf16")
    return f32, b16


def corr_fwd_bf16(theta, phi, blab, temperature, h, w, want_small=False, want_argmax=False, want_up=True):
    """bf16 candidate filter + exact fp32 re-scoring.  theta/phi: (fp32 [B,P,C], bf16 [B,P,C]) pairs from
    corr_prepare_bf16; blab [B,3,P].  Same outputs as corr_fwd.  Requires temperature <= 1e-4.
    theta of ONE frame against the R exemplars of phi / blab (multi-reference pass): one set of launches per exemplar."""
    lib = _lib.load()
    (tf, tb), (pf, pb) = theta, phi
    _need_all(theta=tf, phi=pf, blab=blab)
    Bt, P, C = tf.shape
    R = pf.shape[0]
    refs = Bt == 1 and R > 1
    B = R if refs else Bt
    assert P == h * w and (refs or R == Bt) and blab.shape[0] == B
    dev = tf.device
    out = _corr_outputs(B, h, w, dev, want_up, want_small, want_argmax)
    ws = _workspace(dev, lib.dvc_corr_bf16_workspace_bytes(1 if refs else B, P), "corr_bf16")

    def call(tf_, tb_, pf_, pb_, bl, nb, sl):
        rc = lib.dvc_corr_fwd_bf16(ctypes.c_void_p(tb_.data_ptr()), ctypes.c_void_p(pb_.data_ptr()), _p(tf_), _p(pf_),
                                   _p(bl), float(temperature), nb, C, h, w, *_corr_out_args(out, sl),
                                   ctypes.c_void_p(ws.data_ptr()), ws.numel(), _stream())
        _lib.check(rc, "dvc_corr_fwd_bf16")

    if refs:
        for r in range(R):
            call(tf, tb, pf[r:r + 1], pb[r:r + 1], blab[r:r + 1], 1, slice(r, r + 1))
    else:
        call(tf, tb, pf, pb, blab, B, slice(0, B))
    return out


# ---- backward (the training side)
# The three recompute products of the fused correlation's backward and the N x N products of the contextual losses are plain
# fp32 GEMMs with nothing fused into them; the vendor's library (rocBLAS / hipBLASLt behind torch.bmm: fp32 MFMA, exact
# products, fp32 accumulation — torch's float32 matmul precision is "highest" on ROCm and is asserted below) runs them at
# 103-121 TFLOP/s on the MI355X where this library's 1x1-convolution engine reaches 77-81 (tools/gemm_lib_probe.py; the engine
# keeps the better rounding: blocked sums, 2e-7 against 9e-7 of the result's scale — both far inside the tolerances of
# tests/test_gpu_corr_backward.py).  DVC_GEMM_LIB=0 / set_gemm_lib(False) keeps every product on the engine.
# dvc_amd/block_products.py is the one caller: it issues a row block's products through `bmm` or through `conv2d`, by gemm_lib(),
# or — block_products.set_backend("native") — through `bgemm`, this library's own strided GEMM, which needs neither.
def bmm(a, b, out=None, accumulate=False):
    """out = a @ b (or out += a @ b) for batched fp32 matrices [B, M, K] x [B, K, N] through the vendor GEMM; `a` / `b` may be
    transposed or column-sliced VIEWS (the library takes leading dimensions).  Plain fp32: TF32-like modes are refused."""
    if torch.backends.cuda.matmul.allow_tf32 or torch.get_float32_matmul_precision() != "highest":
        raise RuntimeError("dvc_amd: the training-side GEMMs need torch's float32 matmul precision 'highest' (no TF32); "
                           "restore it, or set DVC_GEMM_LIB=0 to keep these products on this library's own fp32 engine")
    for t, name in ((a, "a"), (b, "b")):
        if t.dtype != torch.float32 or not t.is_cuda or t.dim() != 3:
            raise RuntimeError(f"dvc_amd: `{name}` must be a float32 ROCm tensor [B, M, K]")
    if accumulate:
        if out is None:
            raise RuntimeError("dvc_amd: accumulate needs `out`")
        return torch.baddbmm(out, a, b, out=out)
    return torch.bmm(a, b, out=out) if out is not None else torch.bmm(a, b)


def _inner_strides(t, name):
    """(batch, first, second) strides of a [B, X, Y] view for dvc_bgemm; a dimension of size 1 never decides the layout."""
    sb, s1, s2 = t.stride()
    if t.shape[1] == 1 and s2 != 1:
        s1 = 1
    if t.shape[2] == 1 and s1 != 1:
        s2 = 1
    if (s1 != 1 and s2 != 1) or min(sb, s1, s2) < 0:
        raise RuntimeError(f"dvc_amd: `{name}` needs one inner stride of 1 (a transposed or column-sliced view of a contiguous "
                           f"tensor); got strides {tuple(t.stride())}")
    return (0 if t.shape[0] == 1 else sb), s1, s2


_BGEMM_ENGINES = {"fp32": ("dvc_bgemm_workspace_bytes", "dvc_bgemm_splitk", "bgemm"),
                  "split3": ("dvc_bgemm_split3_workspace_bytes", "dvc_bgemm_split3", "bgemm_split3")}


def bgemm(a, b, out=None, accumulate=False, engine="fp32"):
    """out = a @ b (or out += a @ b) for batched fp32 matrices [B, M, K] x [B, K, N] on this library's own GEMM (dvc_bgemm_splitk,
    csrc/bgemm.hip: exact-fp32 MFMA, bit-reproducible, an image's bits independent of the batch).  Same contract as `bmm`: `a` /
    `b` may be transposed or column-sliced VIEWS, `out` a view with unit inner stride; the strides go to the kernel, nothing is
    copied.  Nothing of torch's is used, so its TF32 setting is not looked at.  Sizes with few output tiles are split over K:
    their partial sums live in the per-stream scratch cache (`_workspace`, tag "bgemm": slices x B x M x N floats, grow-only — a
    d L = M dS^T of 16 images at R = 2048 keeps 268 MB for the life of the process).
    engine="split3": the same contract on the bf16 matrix pipes (dvc_bgemm_split3, csrc/bgemm_split3.hip: three bf16 terms per
    operand, eight products, fp32 accumulation; held to the fp32 kernel's error bound), with a workspace of its own (tag
    "bgemm_split3").  Its bits differ from "fp32"'s and are as reproducible."""
    if engine not in _BGEMM_ENGINES:
        raise ValueError(f"dvc_amd: unknown bgemm engine {engine!r}; one of {tuple(_BGEMM_ENGINES)}")
    ws_bytes_fn, run_fn, ws_tag = _BGEMM_ENGINES[engine]
    for t, name in ((a, "a"), (b, "b"), (out, "out")):
        if t is None:
            continue
        if not isinstance(t, torch.Tensor) or not t.is_cuda:
            raise RuntimeError(f"dvc_amd: `{name}` must be a ROCm device tensor; the HIP path has no CPU fallback")
        if t.dtype != torch.float32 or t.dim() != 3:
            raise RuntimeError(f"dvc_amd: `{name}` must be a float32 ROCm tensor [B, M, K]")
        if t.device.index != _current_device():
            raise RuntimeError(f"dvc_amd: `{name}` lives on {t.device} but the current device is cuda:{_current_device()}")
    (B, M, K), N = a.shape, b.shape[2]
    if b.shape[0] != B or b.shape[1] != K or min(B, M, N, K) < 1:
        raise RuntimeError(f"dvc_amd: bgemm shapes do not match: a {tuple(a.shape)}, b {tuple(b.shape)}")
    if out is None:
        if accumulate:
            raise RuntimeError("dvc_amd: accumulate needs `out`")
        out = torch.empty((B, M, N), device=a.device, dtype=torch.float32)
    ldc = out.stride(1) if M > 1 else max(out.stride(1), N)
    if tuple(out.shape) != (B, M, N) or (out.stride(2) != 1 and N > 1) or ldc < N or (B > 1 and out.stride(0) < 0):
        raise RuntimeError(f"dvc_amd: `out` must be [B, M, N] = {(B, M, N)} with unit inner stride and rows at least N apart; "
                           f"got shape {tuple(out.shape)}, strides {tuple(out.stride())}")
    a_s, b_s = _inner_strides(a, "a"), _inner_strides(b, "b")
    lib = _lib.load()
    nbytes = getattr(lib, ws_bytes_fn)(B, M, N, K)
    ws = _workspace(a.device, nbytes, ws_tag) if nbytes else None
    _lib.check(getattr(lib, run_fn)(_p(a), _p(b), _p(out), B, M, N, K, *a_s, *b_s, 0 if B == 1 else out.stride(0), ldc,
                                    int(bool(accumulate)), _p(ws), nbytes, _stream()), run_fn)
    return out


def lab2rgb_bwd(lab, grad_rgb, l_offset=0.0):
    """dvc_lab2rgb_bwd: d loss / d lab of lab2rgb(lab, l_offset) for d loss / d rgb = grad_rgb."""
    lib = _lib.load()
    _need_all(lab=lab, grad_rgb=grad_rgb)
    N, C, H, W = lab.shape
    assert C == 3 and grad_rgb.shape == lab.shape, (lab.shape, grad_rgb.shape)
    g = torch.empty_like(lab)
    _lib.check(lib.dvc_lab2rgb_bwd(_p(lab), N, H * W, float(l_offset), _p(grad_rgb), _p(g), _stream()), "dvc_lab2rgb_bwd")
    return g


# ---- VGG19 input gradient (csrc/vgg_bwd.hip; dvc_amd/nets.py walks the layers)
def vgg_act_bwd(dX, g, R, out=None):
    """dvc_vgg_act_bwd: (dX + g) * [R > 0]; dX or g may be None (not both).  `out` may be dX (in place)."""
    lib = _lib.load()
    _need_all(dX=dX, g=g, R=R, out=out)
    for t in (dX, g, out):
        assert t is None or t.shape == R.shape, (None if t is None else t.shape, R.shape)
    if out is None:
        out = torch.empty_like(R)
    _lib.check(lib.dvc_vgg_act_bwd(_p(dX), _p(g), _p(R), R.numel(), _p(out), _stream()), "dvc_vgg_act_bwd")
    return out


def vgg_pool_act_bwd(dP, gP, gR, R, avg=False):
    """dvc_vgg_pool_act_bwd: (route(dP + gP) + gR) * [R > 0] through a 2x2 max (avg=False) or average pool of R [N,C,H,W];
    dP, gP: [N,C,H//2,W//2].  Any of dP, gP, gR may be None (not all three)."""
    lib = _lib.load()
    _need_all(dP=dP, gP=gP, gR=gR, R=R)
    N, C, H, W = R.shape
    for t in (dP, gP):
        assert t is None or tuple(t.shape) == (N, C, H // 2, W // 2), (t.shape, R.shape)
    assert gR is None or gR.shape == R.shape, (gR.shape, R.shape)
    out = torch.empty_like(R)
    _lib.check(lib.dvc_vgg_pool_act_bwd(_p(dP), _p(gP), _p(gR), _p(R), N * C, H, W, 1 if avg else 0, _p(out), _stream()),
               "dvc_vgg_pool_act_bwd")
    return out


def vgg_conv1_bwd(dZ, w_t):
    """dvc_vgg_conv1_bwd: the 3-channel input gradient of a 3x3 pad-1 convolution; w_t [3][C][3][3] (nets.vgg_bwd_weight_conv1)."""
    lib = _lib.load()
    _need_all(dZ=dZ, w_t=w_t)
    N, C, H, W = dZ.shape
    assert tuple(w_t.shape) == (3, C, 3, 3), (w_t.shape, dZ.shape)
    dx = torch.empty((N, 3, H, W), device=dZ.device, dtype=torch.float32)
    _lib.check(lib.dvc_vgg_conv1_bwd(_p(dZ), _p(w_t), N, C, H, W, _p(dx), _stream()), "dvc_vgg_conv1_bwd")
    return dx


# ---- ColorVidNet backward (csrc/cvn_bwd.hip; dvc_amd/nets.py walks the layers)
def _slotted_wgrad(name, launch, S, Cout, Cin, k, device):
    """The workspace protocol of the two weight-gradient entry points: S partial slots of ld = Cout*Cin*k*k + Cout floats and an
    `out` of ld floats; launch(part, out) -> rc.  Returns out split into (dW [Cout,Cin,k,k], db [Cout])."""
    nw = Cout * Cin * k * k
    part = torch.empty(S * (nw + Cout), device=device, dtype=torch.float32)
    out = torch.empty(nw + Cout, device=device, dtype=torch.float32)
    _lib.check(launch(part, out), name)
    return out[:nw].view(Cout, Cin, k, k), out[nw:]


def cvn_wgrad_splits(N, Cin, Cout, H, W):
    """The default number of position slots dvc_cvn_wgrad splits a layer's sum over."""
    return int(_lib.load().dvc_cvn_wgrad_splits(N, Cin, Cout, H, W))


def cvn_wgrad(dZ, X, *, dil=1, in_up=1, splits=None):
    """dvc_cvn_wgrad: (dW [Cout][Cin][3][3], db [Cout]) of a 3x3 pad == dil convolution from its output gradient dZ [N,Cout,H,W]
    and its input X [N,Cin,H,W] (in_up = 2: the half-resolution map the layer reads through a nearest x2 upsample)."""
    lib = _lib.load()
    _need_all(dZ=dZ, X=X)
    N, Cout, H, W = dZ.shape
    Cin = X.shape[1]
    assert X.shape[0] == N and tuple(X.shape[2:]) == (H // in_up, W // in_up), (X.shape, dZ.shape, in_up)
    S = cvn_wgrad_splits(N, Cin, Cout, H, W) if splits is None else int(splits)
    return _slotted_wgrad("dvc_cvn_wgrad", lambda part, out: lib.dvc_cvn_wgrad(
        _p(dZ), _p(X), N, Cin, Cout, H, W, dil, in_up, S, _p(part), part.numel(), _p(out), _stream()), S, Cout, Cin, 3, dZ.device)


def cvn_head_bwd(ab, grad_ab, w_ab, R, slope=0.2):
    """dvc_cvn_head_bwd: conv10_ab + tanh*128 backward.  ab: the saved output [N,2,H,W]; w_ab [2][C]; R: the saved post-leaky
    input [N,C,H,W].  Returns (dZ of the layer in front [N,C,H,W], dW_ab [2,C,1,1], db_ab [2])."""
    lib = _lib.load()
    _need_all(ab=ab, grad_ab=grad_ab, w_ab=w_ab, R=R)
    N, C, H, W = R.shape
    assert tuple(ab.shape) == (N, 2, H, W) and grad_ab.shape == ab.shape and tuple(w_ab.shape) == (2, C), (ab.shape, w_ab.shape)
    dZ = torch.empty_like(R)
    part = torch.empty(int(lib.dvc_cvn_head_bwd_workspace_floats(N, C, H * W)), device=R.device, dtype=torch.float32)
    out = torch.empty(2 * C + 2, device=R.device, dtype=torch.float32)
    _lib.check(lib.dvc_cvn_head_bwd(_p(ab), _p(grad_ab), _p(w_ab), _p(R), N, C, H * W, float(slope), _p(dZ), _p(part),
                                    part.numel(), _p(out), _stream()), "dvc_cvn_head_bwd")
    return dZ, out[:2 * C].view(2, C, 1, 1), out[2 * C:]


def cvn_inorm_bwd(n, rstd, R, g_full=None, g_ss=None, ss_w=None, g_up=None):
    """dvc_cvn_inorm_bwd: the gradient at the pre-norm layer's pre-activation, (dn -> dx) * [R > 0], with dn assembled from a
    full-resolution consumer g_full, a stride-2 consumer g_ss of n * ss_w, and a nearest-x2 consumer g_up.  Returns
    (dZ, d ss_w [C] or None)."""
    lib = _lib.load()
    _need_all(n=n, rstd=rstd, R=R, g_full=g_full, g_ss=g_ss, ss_w=ss_w, g_up=g_up)
    N, C, H, W = n.shape
    assert R.shape == n.shape and rstd.numel() == N * C
    assert g_full is None or g_full.shape == n.shape
    assert g_ss is None or tuple(g_ss.shape) == (N, C, (H + 1) // 2, (W + 1) // 2), g_ss.shape
    assert g_up is None or tuple(g_up.shape) == (N, C, 2 * H, 2 * W), g_up.shape
    dZ = torch.empty_like(n)
    ss_part = ss_grad = None
    if g_ss is not None:
        assert ss_w is not None and ss_w.numel() == C
        ss_part = torch.empty(N * C, device=n.device, dtype=torch.float32)
        ss_grad = torch.empty(C, device=n.device, dtype=torch.float32)
    _lib.check(lib.dvc_cvn_inorm_bwd(_p(n), _p(rstd), _p(R), _p(g_full), _p(g_ss), _p(ss_w), _p(g_up), N, C, H, W, _p(dZ),
                                     _p(ss_part), _p(ss_grad), _stream()), "dvc_cvn_inorm_bwd")
    return dZ, ss_grad


# ---- WarpNet backward behind the trunk tensor (csrc/warp_bwd.hip; dvc_amd/nets.py walks the layers)
def warp_up4_bwd(g):
    """dvc_warp_up4_bwd: the 4x4 block sums of g [N,C,4h,4w] -> [N,C,h,w] (backward of the x4 nearest upsample)."""
    lib = _lib.load()
    _need(g, "g")
    N, C, H, W = g.shape
    if H % 4 or W % 4:
        raise RuntimeError(f"dvc_amd: warp_up4_bwd: {H} x {W} is not a x4 upsampled map")
    out = torch.empty((N, C, H // 4, W // 4), device=g.device, dtype=torch.float32)
    _lib.check(lib.dvc_warp_up4_bwd(_p(g), N * C, H // 4, W // 4, _p(out), _stream()), "dvc_warp_up4_bwd")
    return out


def warp_prelu_fwd(n, slope_t, skip=None, out=None):
    """dvc_warp_prelu_fwd: prelu(n + skip) with the one-element slope tensor `slope_t`; `out` may be n (in place)."""
    lib = _lib.load()
    _need_all(n=n, slope=slope_t, skip=skip, out=out)
    assert slope_t.numel() == 1 and (skip is None or skip.shape == n.shape) and (out is None or out.shape == n.shape)
    if out is None:
        out = torch.empty_like(n)
    _lib.check(lib.dvc_warp_prelu_fwd(_p(n), _p(skip), _p(slope_t), n.numel(), _p(out), _stream()), "dvc_warp_prelu_fwd")
    return out


def warp_cn_bwd(t_raw, mean, g, eps=EPS64):
    """dvc_warp_cn_bwd: d t_raw of corr_prepare(t_raw) for d out = g [B,C,P]; mean from corr_prepare_with_mean."""
    lib = _lib.load()
    _need_all(t_raw=t_raw, mean=mean, g=g)
    B, C = t_raw.shape[0], t_raw.shape[1]
    P = t_raw[0, 0].numel()
    assert tuple(g.shape) == (B, C, P) and mean.numel() == B * C, (t_raw.shape, g.shape, mean.shape)
    dt = torch.empty((B, C, P), device=g.device, dtype=torch.float32)
    _lib.check(lib.dvc_warp_cn_bwd(_p(t_raw), _p(mean), _p(g), B, C, P, float(eps), _p(dt), _stream()), "dvc_warp_cn_bwd")
    return dt


def warp_k1_wgrad_splits(N, Cin, Cout, P):
    """The default number of position slots dvc_warp_k1_wgrad splits its sum over."""
    return int(_lib.load().dvc_warp_k1_wgrad_splits(N, Cin, Cout, P))


def warp_k1_wgrad(dT, F, *, splits=None):
    """dvc_warp_k1_wgrad: (dW [Cout,Cin,1,1], db [Cout]) of a 1x1 convolution from its output gradient dT [N,Cout,P] (or
    [N,Cout,h,w]) and its input F [N,Cin,P] (or [N,Cin,h,w])."""
    lib = _lib.load()
    _need_all(dT=dT, F=F)
    N, Cout, Cin = dT.shape[0], dT.shape[1], F.shape[1]
    P = dT[0, 0].numel()
    assert F.shape[0] == N and F[0, 0].numel() == P, (dT.shape, F.shape)
    S = warp_k1_wgrad_splits(N, Cin, Cout, P) if splits is None else int(splits)
    return _slotted_wgrad("dvc_warp_k1_wgrad", lambda part, out: lib.dvc_warp_k1_wgrad(
        _p(dT), _p(F), N, Cin, Cout, P, S, _p(part), part.numel(), _p(out), _stream()), S, Cout, Cin, 1, dT.device)


def warp_norm_prelu_bwd(g, n, rstd, slope_t, skip=None, slope_part=None):
    """dvc_warp_norm_prelu_bwd: from the gradient g [N,C,H,W] at prelu(n + skip), n an InstanceNorm output with 1/sigma rstd [N*C].
    Returns (dz zero-ringed [N,C,H+2,W+2], du [N,C,H,W] — the skip's gradient, None without a skip —, slope_part [N*C] float64:
    the slope gradient's per-plane partial sums; pass a preallocated slice as `slope_part`)."""
    lib = _lib.load()
    _need_all(g=g, n=n, rstd=rstd, slope=slope_t, skip=skip)
    N, C, H, W = n.shape
    assert g.shape == n.shape and rstd.numel() == N * C and slope_t.numel() == 1 and (skip is None or skip.shape == n.shape)
    if slope_part is None:
        slope_part = torch.empty(N * C, device=n.device, dtype=torch.float64)
    if not (slope_part.is_cuda and slope_part.dtype == torch.float64 and slope_part.is_contiguous() and slope_part.numel() == N * C):
        raise RuntimeError("dvc_amd: `slope_part` must be a contiguous float64 ROCm tensor of N*C elements")
    dz = torch.empty((N, C, H + 2, W + 2), device=n.device, dtype=torch.float32)
    du = torch.empty_like(n) if skip is not None else None
    _lib.check(lib.dvc_warp_norm_prelu_bwd(_p(g), _p(n), _p(skip), _p(rstd), _p(slope_t), N * C, H, W, _p(dz), _p(du),
                                           ctypes.c_void_p(slope_part.data_ptr()), _stream()), "dvc_warp_norm_prelu_bwd")
    return dz, du, slope_part


def warp_slope_sum(part):
    """dvc_warp_slope_sum: the float64 partial sums `part` added in a fixed order -> a one-element float32 tensor."""
    lib = _lib.load()
    if not (isinstance(part, torch.Tensor) and part.is_cuda and part.dtype == torch.float64 and part.is_contiguous()):
        raise RuntimeError("dvc_amd: `part` must be a contiguous float64 ROCm tensor")
    out = torch.empty(1, device=part.device, dtype=torch.float32)
    _lib.check(lib.dvc_warp_slope_sum(ctypes.c_void_p(part.data_ptr()), part.numel(), _p(out), _stream()), "dvc_warp_slope_sum")
    return out


def warp_reflect_pad(x):
    """dvc_warp_reflect_pad: ReflectionPad2d(1) of x [N,C,H,W] -> [N,C,H+2,W+2]."""
    lib = _lib.load()
    _need(x, "x")
    N, C, H, W = x.shape
    xp = torch.empty((N, C, H + 2, W + 2), device=x.device, dtype=torch.float32)
    _lib.check(lib.dvc_warp_reflect_pad(_p(x), N * C, H, W, _p(xp), _stream()), "dvc_warp_reflect_pad")
    return xp


def warp_fold(g_padded, skip=None):
    """dvc_warp_fold: the adjoint of ReflectionPad2d(1) of g_padded [N,C,H+2,W+2] (+ skip [N,C,H,W]) -> [N,C,H,W]."""
    lib = _lib.load()
    _need_all(g_padded=g_padded, skip=skip)
    N, C, PH, PW = g_padded.shape
    H, W = PH - 2, PW - 2
    assert skip is None or tuple(skip.shape) == (N, C, H, W), (g_padded.shape, skip.shape)
    dx = torch.empty((N, C, H, W), device=g_padded.device, dtype=torch.float32)
    _lib.check(lib.dvc_warp_fold(_p(g_padded), _p(skip), N * C, H, W, _p(dx), _stream()), "dvc_warp_fold")
    return dx


# ---- WarpNet backward through the four heads (csrc/warp_head_bwd.hip; dvc_amd/nets.py walks arch.WARP_HEAD_PLAN)
def warp_head_wgrad_splits(N, Cin, Cout, H, W, stride):
    """The default number of position slots dvc_warp_head_wgrad splits a layer's sum over."""
    return int(_lib.load().dvc_warp_head_wgrad_splits(N, Cin, Cout, H, W, stride))


def warp_head_wgrad(dz_ringed, x_padded, *, stride=1, splits=None):
    """dvc_warp_head_wgrad: (dW [Cout,Cin,3,3], db [Cout]) of a 3x3 reflect-pad-1 convolution of stride 1 or 2 from the
    zero-ringed dz [N,Cout,Ho+2,Wo+2] (warp_norm_prelu_bwd) and the reflect-padded input [N,Cin,H+2,W+2] (warp_reflect_pad)."""
    lib = _lib.load()
    _need_all(dz_ringed=dz_ringed, x_padded=x_padded)
    N, Cout = dz_ringed.shape[0], dz_ringed.shape[1]
    Cin, H, W = x_padded.shape[1], x_padded.shape[2] - 2, x_padded.shape[3] - 2
    if stride not in (1, 2) or H < 2 or W < 2 or x_padded.shape[0] != N or \
            tuple(dz_ringed.shape[2:]) != ((H - 1) // stride + 3, (W - 1) // stride + 3):
        raise RuntimeError(f"dvc_amd: warp_head_wgrad: dz_ringed {tuple(dz_ringed.shape)} is not the ringed stride-{stride} "
                           f"output of x_padded {tuple(x_padded.shape)}")
    S = warp_head_wgrad_splits(N, Cin, Cout, H, W, stride) if splits is None else int(splits)
    return _slotted_wgrad("dvc_warp_head_wgrad", lambda part, out: lib.dvc_warp_head_wgrad(
        _p(dz_ringed), _p(x_padded), N, Cin, Cout, H, W, stride, S, _p(part), part.numel(), _p(out), _stream()),
        S, Cout, Cin, 3, dz_ringed.device)


def warp_dilate_ring(dz_ringed, H, W):
    """dvc_warp_dilate_ring: the zero-ringed dz [N,C,Ho+2,Wo+2] of a stride-2 layer on an H x W input -> [N,C,H+2,W+2], dz on the
    odd rows / columns, zero elsewhere (what ops.conv3x3 with W^T flipped turns into the gradient at the padded input)."""
    lib = _lib.load()
    _need(dz_ringed, "dz_ringed")
    N, C, Ho, Wo = dz_ringed.shape[0], dz_ringed.shape[1], dz_ringed.shape[2] - 2, dz_ringed.shape[3] - 2
    out = torch.empty((N, C, H + 2, W + 2), device=dz_ringed.device, dtype=torch.float32)
    _lib.check(lib.dvc_warp_dilate_ring(_p(dz_ringed), N * C, Ho, Wo, H, W, _p(out), _stream()), "dvc_warp_dilate_ring")
    return out


def warp_up2_bwd(g):
    """dvc_warp_up2_bwd: the 2x2 block sums of g [N,C,2h,2w] -> [N,C,h,w] (backward of a x2 nearest upsample)."""
    lib = _lib.load()
    _need(g, "g")
    N, C, H, W = g.shape
    if H % 2 or W % 2:
        raise RuntimeError(f"dvc_amd: warp_up2_bwd: {H} x {W} is not a x2 upsampled map")
    out = torch.empty((N, C, H // 2, W // 2), device=g.device, dtype=torch.float32)
    _lib.check(lib.dvc_warp_up2_bwd(_p(g), N * C, H // 2, W // 2, _p(out), _stream()), "dvc_warp_up2_bwd")
    return out


def warp_rpad_rows_bwd(g, rpad):
    """dvc_warp_rpad_rows_bwd: backward of `rpad` replicated rows above and below: g [N,C,h+2*rpad,w] -> [N,C,h,w]."""
    lib = _lib.load()
    _need(g, "g")
    N, C, PH, W = g.shape
    out = torch.empty((N, C, PH - 2 * rpad, W), device=g.device, dtype=torch.float32)
    _lib.check(lib.dvc_warp_rpad_rows_bwd(_p(g), N * C, PH - 2 * rpad, W, rpad, _p(out), _stream()), "dvc_warp_rpad_rows_bwd")
    return out


# ---- Discriminator_x64, forward and input gradient (csrc/gan.hip; dvc_amd/gan.py walks the layers)
def _gan_desc(N, Cin, H, W, Cout, *, slope, act, x_bs=0, y_bs=0):
    return _conv_desc(N, Cin, H, W, Cout, ksize=4, stride=2, pad=1, act=act, act_slope=slope, x_batch_stride=x_bs,
                      y_batch_stride=y_bs)


def gan_spectral_sigma(w_bar, u, v, eps=1e-12):
    """dvc_gan_spectral_sigma: one power step on w_bar [Cout, ...] read as [Cout, K]; u [Cout] and v [K] are updated IN PLACE.
    Returns inv_sigma, a one-element device tensor holding 1 / (u^T W v) — nothing comes back to the host."""
    lib = _lib.load()
    _need_all(w_bar=w_bar, u=u, v=v)
    Cout = w_bar.shape[0]
    K = w_bar.numel() // Cout
    assert u.numel() == Cout and v.numel() == K, (w_bar.shape, u.shape, v.shape)
    inv = torch.empty(1, device=w_bar.device, dtype=torch.float32)
    ws = _workspace(w_bar.device, (K + Cout) * 4, "gan_sn")
    _lib.check(lib.dvc_gan_spectral_sigma(_p(w_bar), Cout, K, float(eps), _p(u), _p(v), _p(inv), _p(ws), ws.numel(), _stream()),
               "dvc_gan_spectral_sigma")
    return inv


def gan_sn_weight(w_bar, inv_sigma, scaled=None, scaled_t=None, col=0):
    """dvc_gan_sn_weight: w_bar [Cout, K] / sigma into `scaled` [Cout, K] and / or, transposed, into columns col .. col + Cout of
    `scaled_t` [K, ld]."""
    lib = _lib.load()
    _need_all(w_bar=w_bar, inv_sigma=inv_sigma, scaled=scaled, scaled_t=scaled_t)
    Cout = w_bar.shape[0]
    K = w_bar.numel() // Cout
    assert scaled is None or scaled.numel() == Cout * K, (scaled.shape, w_bar.shape)
    ldt, pt = 0, None
    if scaled_t is not None:
        ldt = scaled_t.shape[1]
        assert scaled_t.dim() == 2 and scaled_t.shape[0] == K and 0 <= col and col + Cout <= ldt, (scaled_t.shape, col, Cout)
        pt = ctypes.c_void_p(scaled_t.data_ptr() + 4 * col)
    _lib.check(lib.dvc_gan_sn_weight(_p(w_bar), _p(inv_sigma), Cout, K, _p(scaled), pt, ldt, _stream()), "dvc_gan_sn_weight")


def gan_conv4s2(x, w_bar, bias, inv_sigma, *, act=ACT_LEAKY, slope=0.2, out=None, out_batch_stride=0):
    """dvc_gan_conv4s2: act(conv 4x4 stride 2 zero-pad 1 (x, w_bar) / sigma + bias) -> [N, Cout, H // 2, W // 2]."""
    lib = _lib.load()
    _need_all(x=x, w_bar=w_bar, bias=bias, inv_sigma=inv_sigma)
    N, Cin, H, W = x.shape
    Cout = w_bar.shape[0]
    assert tuple(w_bar.shape) == (Cout, Cin, 4, 4) and bias.numel() == Cout, (w_bar.shape, x.shape, bias.shape)
    if out is None:
        out = torch.empty((N, Cout, H // 2, W // 2), device=x.device, dtype=torch.float32)
    d = _gan_desc(N, Cin, H, W, Cout, slope=slope, act=act, y_bs=out_batch_stride)
    if conv_record is not None:
        conv_record.append(_record_conv(d, affine=False, in_prelu=False, residual=False, algo="gan4s2"))
    _lib.check(lib.dvc_gan_conv4s2(ctypes.byref(d), _p(x), _p(w_bar), _p(bias), _p(inv_sigma), _p(out), _stream()), "dvc_gan_conv4s2")
    return out


def gan_conv4s2_dgrad(dz, w_bar, inv_sigma, in_hw, *, mask_act=None, slope=0.2):
    """dvc_gan_conv4s2_dgrad: the layer's input gradient [N, Cin, H, W] (in_hw = (H, W)) for dz [N, Cout, H // 2, W // 2], the
    gradient at its pre-activation output; with mask_act (the layer's input, a LeakyReLU output) times that LeakyReLU's
    derivative."""
    lib = _lib.load()
    _need_all(dz=dz, w_bar=w_bar, inv_sigma=inv_sigma, mask_act=mask_act)
    (N, Cout, OH, OW), Cin, (H, W) = dz.shape, w_bar.shape[1], in_hw
    assert tuple(w_bar.shape) == (Cout, Cin, 4, 4) and (OH, OW) == (H // 2, W // 2), (w_bar.shape, dz.shape, in_hw)
    assert mask_act is None or tuple(mask_act.shape) == (N, Cin, H, W), (mask_act.shape, (N, Cin, H, W))
    dx = torch.empty((N, Cin, H, W), device=dz.device, dtype=torch.float32)
    d = _gan_desc(N, Cin, H, W, Cout, slope=slope, act=ACT_LEAKY)
    _lib.check(lib.dvc_gan_conv4s2_dgrad(ctypes.byref(d), _p(dz), _p(w_bar), _p(inv_sigma), _p(mask_act), _p(dx), _stream()),
               "dvc_gan_conv4s2_dgrad")
    return dx


def gan_last(x, w_bar, bias, inv_sigma):
    """dvc_gan_last: mean over positions of conv [3, 6] valid (x, w_bar [1, Cin, 3, 6]) / sigma + bias -> [N, 1]."""
    lib = _lib.load()
    _need_all(x=x, w_bar=w_bar, bias=bias, inv_sigma=inv_sigma)
    N, Cin, H, W = x.shape
    assert tuple(w_bar.shape) == (1, Cin, 3, 6), (w_bar.shape, x.shape)
    out = torch.empty((N, 1), device=x.device, dtype=torch.float32)
    _lib.check(lib.dvc_gan_last(_p(x), _p(w_bar), _p(bias), _p(inv_sigma), N, Cin, H, W, 0, _p(out), _stream()), "dvc_gan_last")
    return out


def gan_last_bwd(g, w_bar, inv_sigma, x, *, mask=True, slope=0.2):
    """dvc_gan_last_bwd: d loss / d x of gan_last for g [N, 1]; mask=True: times the derivative of the LeakyReLU that made x."""
    lib = _lib.load()
    _need_all(g=g, w_bar=w_bar, inv_sigma=inv_sigma, x=x)
    N, Cin, H, W = x.shape
    assert g.numel() == N and tuple(w_bar.shape) == (1, Cin, 3, 6), (g.shape, w_bar.shape, x.shape)
    dx = torch.empty_like(x)
    _lib.check(lib.dvc_gan_last_bwd(_p(g), _p(w_bar), _p(inv_sigma), _p(x) if mask else None, float(slope), N, Cin, H, W, _p(dx),
                                    _stream()), "dvc_gan_last_bwd")
    return dx


def gan_softmax_rows(e, out=None):
    """dvc_gan_softmax_rows: softmax over the last dimension with the row maximum subtracted; out may be e."""
    lib = _lib.load()
    _need_all(e=e, out=out)
    if out is None:
        out = torch.empty_like(e)
    P = e.shape[-1]
    _lib.check(lib.dvc_gan_softmax_rows(_p(e), e.numel() // P, P, _p(out), _stream()), "dvc_gan_softmax_rows")
    return out


def gan_softmax_rows_bwd(a, dA, out=None):
    """dvc_gan_softmax_rows_bwd: a * (dA - sum_j a dA) over the last dimension; out may be dA."""
    lib = _lib.load()
    _need_all(a=a, dA=dA, out=out)
    assert a.shape == dA.shape, (a.shape, dA.shape)
    if out is None:
        out = torch.empty_like(a)
    P = a.shape[-1]
    _lib.check(lib.dvc_gan_softmax_rows_bwd(_p(a), _p(dA), a.numel() // P, P, _p(out), _stream()), "dvc_gan_softmax_rows_bwd")
    return out


def gan_scale_add(o, gamma, x=None):
    """dvc_gan_scale_add: gamma * o (+ x), gamma a one-element device tensor."""
    lib = _lib.load()
    _need_all(o=o, gamma=gamma, x=x)
    assert x is None or x.shape == o.shape, (x.shape, o.shape)
    y = torch.empty_like(o)
    _lib.check(lib.dvc_gan_scale_add(_p(o), _p(x), _p(gamma), o.numel(), _p(y), _stream()), "dvc_gan_scale_add")
    return y


def gan_lrelu_bwd(d, g, act, slope=0.2):
    """dvc_gan_lrelu_bwd: (d + g) * (act > 0 ? 1 : slope); d or g may be None (not both)."""
    lib = _lib.load()
    _need_all(d=d, g=g, act=act)
    for t in (d, g):
        assert t is None or t.shape == act.shape, (t.shape, act.shape)
    out = torch.empty_like(act)
    _lib.check(lib.dvc_gan_lrelu_bwd(_p(d), _p(g), _p(act), float(slope), act.numel(), _p(out), _stream()), "dvc_gan_lrelu_bwd")
    return out


# ---- Discriminator_x64, parameter gradients (csrc/gan_wgrad.hip; dvc_amd/gan.py launches them behind set_parameter_training)
def gan_conv4s2_wgrad_splits(N, Cin, H, W, Cout):
    """The default number of pixel slots dvc_gan_conv4s2_wgrad splits a layer's sum over."""
    d = _gan_desc(N, Cin, H, W, Cout, slope=0.2, act=ACT_LEAKY)
    return int(_lib.load().dvc_gan_conv4s2_wgrad_splits(ctypes.byref(d)))


def gan_conv4s2_wgrad(dz, x, *, splits=None):
    """dvc_gan_conv4s2_wgrad: (G [Cout, Cin, 4, 4], db [Cout]), the plain weight gradient and the bias gradient of a 4x4 stride-2
    pad-1 layer from dz [N, Cout, H // 2, W // 2], the gradient at its pre-activation, and its input x [N, Cin, H, W]."""
    lib = _lib.load()
    _need_all(dz=dz, x=x)
    (N, Cout, OH, OW), (Cin, H, W) = dz.shape, x.shape[1:]
    assert x.shape[0] == N and (OH, OW) == (H // 2, W // 2), (dz.shape, x.shape)
    d = _gan_desc(N, Cin, H, W, Cout, slope=0.2, act=ACT_LEAKY)
    S = int(lib.dvc_gan_conv4s2_wgrad_splits(ctypes.byref(d))) if splits is None else int(splits)
    return _slotted_wgrad("dvc_gan_conv4s2_wgrad", lambda part, out: lib.dvc_gan_conv4s2_wgrad(
        ctypes.byref(d), _p(dz), _p(x), S, _p(part), part.numel(), _p(out), _stream()), S, Cout, Cin, 4, dz.device)


def _gan_dot_workspace(device, count):
    return _workspace(device, int(_lib.load().dvc_gan_dot_workspace_bytes(count)), "gan_dot")


def gan_sn_wgrad(G, w_bar, u, v, inv_sigma, out=None):
    """dvc_gan_sn_wgrad: d loss / d w_bar = (G - <G, w_bar> / sigma * u v^T) / sigma in w_bar's shape, for the plain weight
    gradient G and the vectors u [Cout], v [K] the forward's power step left.  `out` (a contiguous tensor of that shape) is
    overwritten."""
    lib = _lib.load()
    _need_all(G=G, w_bar=w_bar, u=u, v=v, inv_sigma=inv_sigma, out=out)
    Cout = w_bar.shape[0]
    K = w_bar.numel() // Cout
    assert G.numel() == Cout * K and u.numel() == Cout and v.numel() == K and inv_sigma.numel() == 1, (G.shape, w_bar.shape, u.shape, v.shape)
    if out is None:
        out = torch.empty_like(w_bar)
    assert out.shape == w_bar.shape, (out.shape, w_bar.shape)
    ws = _gan_dot_workspace(G.device, Cout * K)
    _lib.check(lib.dvc_gan_sn_wgrad(_p(G), _p(w_bar), _p(u), _p(v), _p(inv_sigma), Cout, K, _p(out), _p(ws), ws.numel(), _stream()),
               "dvc_gan_sn_wgrad")
    return out


def gan_last_wgrad(g, x):
    """dvc_gan_last_wgrad: (G [1, Cin, 3, 6], db [1]) of gan_last on x [N, Cin, H, W] for g [N, 1] = d loss / d out."""
    lib = _lib.load()
    _need_all(g=g, x=x)
    N, Cin, H, W = x.shape
    assert g.numel() == N, (g.shape, x.shape)
    out = torch.empty(Cin * 18 + 1, device=x.device, dtype=torch.float32)
    _lib.check(lib.dvc_gan_last_wgrad(_p(g), _p(x), N, Cin, H, W, 0, _p(out), _stream()), "dvc_gan_last_wgrad")
    return out[:Cin * 18].view(1, Cin, 3, 6), out[Cin * 18:]


def gan_dot(a, b):
    """dvc_gan_dot: sum(a * b) in double in a fixed order, rounded once -> a one-element tensor."""
    lib = _lib.load()
    _need_all(a=a, b=b)
    assert a.numel() == b.numel(), (a.shape, b.shape)
    out = torch.empty(1, device=a.device, dtype=torch.float32)
    ws = _gan_dot_workspace(a.device, a.numel())
    _lib.check(lib.dvc_gan_dot(_p(a), _p(b), a.numel(), _p(out), _p(ws), ws.numel(), _stream()), "dvc_gan_dot")
    return out


# ---- the optimiser step (csrc/optim.hip; dvc_amd/optim.py fills the tables)
def _need_table(t, name, nbytes):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise RuntimeError(f"dvc_amd: `{name}` must be a ROCm device tensor; the HIP path has no CPU fallback")
    if t.dtype != torch.uint8 or not t.is_contiguous() or t.numel() < nbytes or t.data_ptr() % 8:
        raise RuntimeError(f"dvc_amd: `{name}` must be a contiguous 8-byte aligned uint8 tensor of at least {nbytes} bytes")
    if t.device.index != _current_device():
        raise RuntimeError(f"dvc_amd: `{name}` lives on {t.device} but the current device is cuda:{_current_device()}")


def adam_step(tensor_table, n_tensors, chunk_table, n_chunks):
    """dvc_adam_step: ONE launch that applies Adam to every tensor of the two device-resident tables — uint8 device tensors that
    hold n_tensors DvcAdamTensor and n_chunks DvcAdamChunk records (dvc_amd.optim.build_tables lays them out)."""
    lib = _lib.load()
    _need_table(tensor_table, "tensor_table", n_tensors * ctypes.sizeof(_lib.DvcAdamTensor))
    _need_table(chunk_table, "chunk_table", n_chunks * ctypes.sizeof(_lib.DvcAdamChunk))
    _lib.check(lib.dvc_adam_step(_p(tensor_table), n_tensors, _p(chunk_table), n_chunks, _stream()), "dvc_adam_step")


def adam_advance(advance_table, tensor_table, n_tensors):
    """dvc_adam_advance: ONE launch that advances every tensor's device-resident step count and rewrites the step_size and
    inv_sqrt_bc2 columns of `tensor_table` from it — uint8 device tensors that hold n_tensors DvcAdamAdvance and DvcAdamTensor
    records (dvc_amd.optim.CapturableAdam lays them out).  dvc_adam_step follows on the same table and stream."""
    lib = _lib.load()
    _need_table(advance_table, "advance_table", n_tensors * ctypes.sizeof(_lib.DvcAdamAdvance))
    _need_table(tensor_table, "tensor_table", n_tensors * ctypes.sizeof(_lib.DvcAdamTensor))
    _lib.check(lib.dvc_adam_advance(_p(advance_table), _p(tensor_table), n_tensors, _stream()), "dvc_adam_advance")


# ---- the gradient guard (csrc/optim.hip; dvc_amd.optim.GuardedAdam / grad_norm / clip_grad_norm_ own the record)
GRAD_NORM_KEEP_NONFINITE = 1        # == DVC_GRAD_NORM_KEEP_NONFINITE of include/dvc_hip.h


def _need_guard(guard):
    _need_table(guard, "guard", ctypes.sizeof(_lib.DvcGradGuard))


def grad_norm(tensor_table, n_tensors, chunk_table, n_chunks, partials, max_norm, guard, keep_nonfinite=False):
    """dvc_grad_norm: two launches that reduce sum g^2 over every tensor of the two tables (those of adam_step) into `partials`
    (float64, n_chunks) and write the DvcGradGuard record `guard` (a 24-byte uint8 device tensor): norm, clip_grad_norm_'s
    coefficient for `max_norm` (float("inf"): none), the non-finite flag (left 0 with keep_nonfinite) and the skip count."""
    lib = _lib.load()
    _need_table(tensor_table, "tensor_table", n_tensors * ctypes.sizeof(_lib.DvcAdamTensor))
    _need_table(chunk_table, "chunk_table", n_chunks * ctypes.sizeof(_lib.DvcAdamChunk))
    if not isinstance(partials, torch.Tensor) or not partials.is_cuda:
        raise RuntimeError("dvc_amd: `partials` must be a ROCm device tensor; the HIP path has no CPU fallback")
    if partials.dtype != torch.float64 or not partials.is_contiguous() or partials.numel() < n_chunks:
        raise RuntimeError(f"dvc_amd: `partials` must be a contiguous float64 device tensor of at least {n_chunks} elements")
    _need_guard(guard)
    _lib.check(lib.dvc_grad_norm(_p(tensor_table), n_tensors, _p(chunk_table), n_chunks, _p(partials), float(max_norm),
                                 GRAD_NORM_KEEP_NONFINITE if keep_nonfinite else 0, _p(guard), _stream()), "dvc_grad_norm")


def adam_advance_guarded(advance_table, tensor_table, n_tensors, guard):
    """dvc_adam_advance_guarded: adam_advance, unless `guard` has its non-finite flag set — then nothing is touched."""
    lib = _lib.load()
    _need_table(advance_table, "advance_table", n_tensors * ctypes.sizeof(_lib.DvcAdamAdvance))
    _need_table(tensor_table, "tensor_table", n_tensors * ctypes.sizeof(_lib.DvcAdamTensor))
    _need_guard(guard)
    _lib.check(lib.dvc_adam_advance_guarded(_p(advance_table), _p(tensor_table), n_tensors, _p(guard), _stream()),
               "dvc_adam_advance_guarded")


def adam_step_guarded(tensor_table, n_tensors, chunk_table, n_chunks, guard):
    """dvc_adam_step_guarded: adam_step on clip_coef * g, or nothing at all when `guard` has its non-finite flag set."""
    lib = _lib.load()
    _need_table(tensor_table, "tensor_table", n_tensors * ctypes.sizeof(_lib.DvcAdamTensor))
    _need_table(chunk_table, "chunk_table", n_chunks * ctypes.sizeof(_lib.DvcAdamChunk))
    _need_guard(guard)
    _lib.check(lib.dvc_adam_step_guarded(_p(tensor_table), n_tensors, _p(chunk_table), n_chunks, _p(guard), _stream()),
               "dvc_adam_step_guarded")


def grad_scale(tensor_table, n_tensors, chunk_table, n_chunks, guard):
    """dvc_grad_scale: ONE launch that multiplies every gradient of the tables by the coefficient in `guard`, in place."""
    lib = _lib.load()
    _need_table(tensor_table, "tensor_table", n_tensors * ctypes.sizeof(_lib.DvcAdamTensor))
    _need_table(chunk_table, "chunk_table", n_chunks * ctypes.sizeof(_lib.DvcAdamChunk))
    _need_guard(guard)
    _lib.check(lib.dvc_grad_scale(_p(tensor_table), n_tensors, _p(chunk_table), n_chunks, _p(guard), _stream()), "dvc_grad_scale")


# ---- the pixel losses (csrc/loss.hip; dvc_amd/losses.py fills the tables)
def _need_host_table(t, name, nbytes):
    if not isinstance(t, torch.Tensor) or t.device.type != "cpu":
        raise RuntimeError(f"dvc_amd: `{name}` must be the host copy of the table (a CPU uint8 tensor)")
    if t.dtype != torch.uint8 or not t.is_contiguous() or t.numel() < nbytes or t.data_ptr() % 8:
        raise RuntimeError(f"dvc_amd: `{name}` must be a contiguous 8-byte aligned uint8 tensor of at least {nbytes} bytes")


def loss_fwd(term_table, term_table_host, n_terms, chunk_table, n_chunks, partials, values):
    """dvc_loss_fwd: two launches that reduce every term of the device-resident tables — uint8 device tensors that hold n_terms
    DvcLossTerm and n_chunks DvcLossChunk records (dvc_amd.losses.build_tables lays them out; `term_table_host` is the host copy
    the library validates) — into `partials` (float64, n_chunks) and `values` (float32, n_terms + 1: the terms, then the total)."""
    lib = _lib.load()
    _need_table(term_table, "term_table", n_terms * ctypes.sizeof(_lib.DvcLossTerm))
    _need_host_table(term_table_host, "term_table_host", n_terms * ctypes.sizeof(_lib.DvcLossTerm))
    _need_table(chunk_table, "chunk_table", n_chunks * ctypes.sizeof(_lib.DvcLossChunk))
    if not partials.is_cuda or partials.dtype != torch.float64 or not partials.is_contiguous() or partials.numel() < n_chunks:
        raise RuntimeError(f"dvc_amd: `partials` must be a contiguous float64 device tensor of at least {n_chunks} elements")
    _need(values, "values")
    if values.numel() < n_terms + 1:
        raise RuntimeError(f"dvc_amd: `values` must hold {n_terms + 1} floats")
    _lib.check(lib.dvc_loss_fwd(_p(term_table), _p(term_table_host), n_terms, _p(chunk_table), n_chunks, _p(partials), _p(values),
                                _stream()), "dvc_loss_fwd")


def loss_bwd(term_table, term_table_host, n_terms, chunk_table, n_chunks, grad_total, grad_values=None):
    """dvc_loss_bwd: ONE launch that writes dx / dt of every term of the tables (as for loss_fwd, with the gradient addresses
    filled in) from the device scalars `grad_total` (1 float) and `grad_values` (n_terms floats, or None for zeros)."""
    lib = _lib.load()
    _need_table(term_table, "term_table", n_terms * ctypes.sizeof(_lib.DvcLossTerm))
    _need_host_table(term_table_host, "term_table_host", n_terms * ctypes.sizeof(_lib.DvcLossTerm))
    _need_table(chunk_table, "chunk_table", n_chunks * ctypes.sizeof(_lib.DvcLossChunk))
    _need(grad_total, "grad_total")
    _need(grad_values, "grad_values")
    if grad_total.numel() < 1 or (grad_values is not None and grad_values.numel() < n_terms):
        raise RuntimeError(f"dvc_amd: `grad_total` must hold 1 float and `grad_values` {n_terms}")
    _lib.check(lib.dvc_loss_bwd(_p(term_table), _p(term_table_host), n_terms, _p(chunk_table), n_chunks, _p(grad_total),
                                _p(grad_values), _stream()), "dvc_loss_bwd")


# ---- loss plans (csrc/loss_plan.hip; dvc_amd.losses.Plan owns the resident tables)
def loss_plan_scratch_doubles(n_terms, n_chunks, n_ychunks):
    """DVC_LOSS_PLAN_SCRATCH of include/dvc_hip.h: [partials | partials of sum d | partials of y | per slot {m, sum d}]."""
    return 2 * n_chunks + n_ychunks + 2 * n_terms


def loss_plan_check(terms_host, n_chunks, n_ychunks):
    """dvc_loss_plan_check: every refusal of a plan's term table, from its HOST copy (a numpy array of DvcPlanTerm records);
    no device is touched and nothing is launched."""
    lib = _lib.load()
    if terms_host.dtype.itemsize != ctypes.sizeof(_lib.DvcPlanTerm) or not terms_host.flags["C_CONTIGUOUS"]:
        raise RuntimeError("dvc_amd: `terms_host` must be a contiguous array of DvcPlanTerm records")
    _lib.check(lib.dvc_loss_plan_check(ctypes.c_void_p(terms_host.ctypes.data), len(terms_host), n_chunks, n_ychunks),
               "dvc_loss_plan_check")


def _need_plan_tables(term_table, n_terms, chunk_table, n_chunks, n_ychunks, scratch):
    _need_table(term_table, "term_table", n_terms * ctypes.sizeof(_lib.DvcPlanTerm))
    _need_table(chunk_table, "chunk_table", (n_chunks + n_ychunks) * ctypes.sizeof(_lib.DvcLossChunk))
    need = loss_plan_scratch_doubles(n_terms, n_chunks, n_ychunks)
    if (not isinstance(scratch, torch.Tensor) or not scratch.is_cuda or scratch.dtype != torch.float64 or not scratch.is_contiguous()
            or scratch.numel() < need):
        raise RuntimeError(f"dvc_amd: `scratch` must be a contiguous float64 device tensor of at least {need} elements; the HIP path "
                           "has no CPU fallback")


def loss_plan_fwd(term_table, n_terms, chunk_table, n_chunks, n_ychunks, scratch, values):
    """dvc_loss_plan_fwd: two launches (four with a relativistic term) that reduce every term of the device-resident tables —
    uint8 device tensors that hold n_terms DvcPlanTerm and n_chunks + n_ychunks DvcLossChunk records, checked by loss_plan_check
    when they were built — into `values` (float32, n_terms + 1: the terms, then the total); `scratch`: loss_plan_scratch_doubles."""
    lib = _lib.load()
    _need_plan_tables(term_table, n_terms, chunk_table, n_chunks, n_ychunks, scratch)
    _need(values, "values")
    if values.numel() < n_terms + 1:
        raise RuntimeError(f"dvc_amd: `values` must hold {n_terms + 1} floats")
    _lib.check(lib.dvc_loss_plan_fwd(_p(term_table), n_terms, _p(chunk_table), n_chunks, n_ychunks, _p(scratch), _p(values),
                                     _stream()), "dvc_loss_plan_fwd")


def loss_plan_bwd(term_table, n_terms, chunk_table, n_chunks, n_ychunks, scratch, grad_total, grad_values=None):
    """dvc_loss_plan_bwd: ONE launch that writes dx / dt / dy of every term of the tables (those of the forward, with the gradient
    addresses filled in) from the device scalars `grad_total` and `grad_values`; `scratch` is the one the forward wrote."""
    lib = _lib.load()
    _need_plan_tables(term_table, n_terms, chunk_table, n_chunks, n_ychunks, scratch)
    _need(grad_total, "grad_total")
    _need(grad_values, "grad_values")
    if grad_total.numel() < 1 or (grad_values is not None and grad_values.numel() < n_terms):
        raise RuntimeError(f"dvc_amd: `grad_total` must hold 1 float and `grad_values` {n_terms}")
    _lib.check(lib.dvc_loss_plan_bwd(_p(term_table), n_terms, _p(chunk_table), n_chunks, n_ychunks, _p(scratch), _p(grad_total),
                                     _p(grad_values), _stream()), "dvc_loss_plan_bwd")
