"""CPU: the C-ABI library loads and exports every symbol include/dvc_hip.h declares (no compute calls
without a GPU), host-side logic (weight packing, geometry, state_dict contract, loud failures)."""
import ctypes
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header_symbols(debug=False):
    """Entry points include/dvc_hip.h declares: outside (production) or inside (debug=True) its `#ifdef DVC_DEBUG` block."""
    txt = open(os.path.join(ROOT, "include", "dvc_hip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    dbg = re.findall(r"#ifdef DVC_DEBUG(.*?)#endif", txt, flags=re.S)
    txt = "".join(dbg) if debug else re.sub(r"#ifdef DVC_DEBUG.*?#endif", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(dvc_[a-z0-9_]+)\s*\(", txt)))


def test_library_exports_every_declared_symbol():
    from dvc_amd import _lib
    lib = _lib.load()
    syms = _header_symbols()
    assert len(syms) >= 18
    for s in syms:
        assert hasattr(lib, s), f"{s} declared in dvc_hip.h but not exported"
        assert s in _lib.SIGNATURES, f"{s} has no ctypes signature"
    assert set(_lib.SIGNATURES) == set(syms)
    assert lib.dvc_abi_version() == _lib.ABI_VERSION
    assert lib.dvc_corr_workspace_bytes(1, 5184) > 0
    # ... and nothing with C linkage is exported that the header does not declare
    import subprocess
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if len(ln.split()) == 3}
    # -fvisibility=hidden + csrc/exports.map: no C++ internals, no host-side kernel handles, no debug hooks
    assert exported == set(syms), (sorted(exported - set(syms)), sorted(set(syms) - exported))
    assert set(_lib.DEBUG_SIGNATURES) == set(_header_symbols(debug=True)) and not (set(_lib.DEBUG_SIGNATURES) & exported)
    dbg_lib = os.path.join(os.path.dirname(_lib.LIB_PATH), "libdvc_hip_debug.so")
    if os.path.exists(dbg_lib):     # the -DDVC_DEBUG build (tools/ only) adds exactly the four hooks
        out = subprocess.run(["nm", "-D", "--defined-only", dbg_lib], capture_output=True, text=True).stdout
        assert {ln.split()[-1] for ln in out.splitlines() if len(ln.split()) == 3} == set(syms) | set(_lib.DEBUG_SIGNATURES)


def test_argument_validation_without_gpu():
    """Validation errors are reported through the return code + dvc_last_error, before any launch."""
    from dvc_amd import _lib
    lib = _lib.load()
    d = _lib.DvcConvDesc(1, 4, 8, 8, 6, 3, 1, 1, 1, 0, 1, 1, 0, 0.0, 0, -1, 0, 0, 0, 0)   # Cout % 4 != 0
    one = ctypes.c_void_p(16)
    rc = lib.dvc_conv2d(ctypes.byref(d), one, one, None, None, None, None, None, None, one, None, 0, None)
    assert rc != 0 and b"multiple of 4" in lib.dvc_last_error()
    oh, ow = ctypes.c_int32(), ctypes.c_int32()
    d2 = _lib.DvcConvDesc(1, 4, 27, 45, 8, 3, 2, 1, 1, 1, 1, 1, 0, 0.0, 0, -1, 0, 0, 0, 0)
    assert lib.dvc_conv2d_out_hw(ctypes.byref(d2), ctypes.byref(oh), ctypes.byref(ow)) == 0
    assert (oh.value, ow.value) == (14, 23)
    # dvc_conv2d_winograd_pool: dilation 1 only, an output of at least one pooling window, a pooled destination
    dp = _lib.DvcConvDesc(1, 64, 27, 48, 64, 3, 1, 2, 2, 0, 1, 1, 1, 0.0, 0, -1, 0, 0, 0, 0, 0)
    rc = lib.dvc_conv2d_winograd_pool(ctypes.byref(dp), one, one, None, None, one, one, 0, None, 0, None)
    assert rc != 0 and b"dilation 1" in lib.dvc_last_error()
    dp = _lib.DvcConvDesc(1, 64, 1, 48, 64, 3, 1, 1, 1, 0, 1, 1, 1, 0.0, 0, -1, 0, 0, 0, 0, 0)
    rc = lib.dvc_conv2d_winograd_pool(ctypes.byref(dp), one, one, None, None, one, one, 0, None, 0, None)
    assert rc != 0 and b"pooling window" in lib.dvc_last_error()
    dp = _lib.DvcConvDesc(1, 64, 27, 48, 64, 3, 1, 1, 1, 0, 1, 1, 1, 0.0, 0, -1, 0, 0, 0, 0, 0)
    rc = lib.dvc_conv2d_winograd_pool(ctypes.byref(dp), one, one, None, None, one, None, 0, None, 0, None)
    assert rc != 0 and b"null argument" in lib.dvc_last_error()


def test_conv_geometry_matches_torch():
    import torch.nn.functional as F

    from dvc_amd import ops
    for (H, W, ks, s, d, p, up, sub) in [(27, 48, 3, 1, 2, 2, 1, 1), (54, 96, 3, 2, 1, 1, 1, 1),
                                         (13, 24, 3, 1, 1, 1, 2, 1), (27, 45, 3, 1, 1, 1, 1, 2),
                                         (12, 20, 1, 1, 1, 0, 1, 1)]:
        x = torch.zeros(1, 1, H, W)
        if sub == 2:
            x = x[:, :, ::2, ::2]
        if up == 2:
            x = F.interpolate(x, scale_factor=2)
        y = F.conv2d(x, torch.zeros(1, 1, ks, ks), stride=s, padding=p, dilation=d)
        assert ops.conv_out_hw(H, W, ks, s, d, p, up, sub) == tuple(y.shape[2:])


def test_pack_conv_weight_layout():
    from dvc_amd import ops
    w = torch.arange(2 * 3 * 3 * 3, dtype=torch.float32).view(2, 3, 3, 3)
    p = ops.pack_conv_weight(w)
    assert p.shape == (3, 9, 2)
    for co in range(2):
        for ci in range(3):
            for t in range(9):
                assert p[ci, t, co] == w[co, ci, t // 3, t % 3]


def test_state_dict_contract_and_loud_cpu_failure(weights, capsys):
    from models.ColorVidNet import ColorVidNet
    from models.NonlocalNet import VGG19_pytorch, WarpNet
    vgg, warp, col = VGG19_pytorch(), WarpNet(1), ColorVidNet(7)
    out = capsys.readouterr().out
    assert "replace all deconv with [nearest + conv]" in out      # ColorVidNet.py:80,85
    for m, sd in zip((vgg, warp, col), weights):
        m.load_state_dict(sd, strict=True)
        assert list(m.state_dict().keys()) == list(sd.keys())
        assert all(torch.equal(m.state_dict()[k], sd[k]) for k in sd)
        assert sum(p.numel() for p in m.parameters()) == sum(v.numel() for v in sd.values())
    assert len(weights[0]) == 32 and len(weights[1]) == 43 and len(weights[2]) == 65
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        vgg(torch.zeros(1, 3, 16, 16), ["r11"])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        col(torch.zeros(1, 7, 16, 16))
    from utils.util import feature_normalize, uncenter_l
    assert uncenter_l(-50.0) == 0.0
    with pytest.raises(RuntimeError):
        feature_normalize(torch.zeros(1, 4, 2, 2))


def test_product_code_never_imports_oracle():
    """The oracle is test infrastructure; nothing under the product package may import it."""
    pkg = os.path.join(ROOT, "deep-exemplar-based-video-colorization_amd")
    for dp, _, fs in os.walk(pkg):
        for f in fs:
            if f.endswith(".py"):
                for ln in open(os.path.join(dp, f)).read().splitlines():
                    assert not re.match(r"\s*(from|import)\s+oracle", ln), (f, ln)
                    assert "dvc_oracle" not in ln, (f, ln)


def test_fma_division_by_constant_is_correctly_rounded():
    """csrc/corr.hip computes ATen's s = fl32(f / T) for the fixed divisor T as q = f*y followed by two fma
    residual corrections (y = fl32(1/T)).  Check the recipe against exact rational arithmetic: it must
    give the correctly rounded quotient, otherwise ties at T = 1e-10 would differ from the reference."""
    import math
    from fractions import Fraction

    import numpy as np

    def rn32(x):
        """Round a Fraction to the nearest float32 (ties to even); returns a python float."""
        if x == 0:
            return 0.0
        sign = -1 if x < 0 else 1
        x = abs(x)
        e = math.floor(math.log2(x.numerator) - math.log2(x.denominator))
        while Fraction(2) ** e > x:
            e -= 1
        while Fraction(2) ** (e + 1) <= x:
            e += 1
        e = max(e, -126)
        ulp = Fraction(2) ** (e - 23)
        q = x / ulp
        n = q.numerator // q.denominator
        rem = q - n
        if rem > Fraction(1, 2) or (rem == Fraction(1, 2) and n % 2 == 1):
            n += 1
        return float(sign * n * ulp)

    def fma(a, b, c):
        return rn32(Fraction(a) * Fraction(b) + Fraction(c))

    rng = np.random.default_rng(0)
    for T in (1e-10, 0.01, 0.005, 1.0, 3.3e-7, 1e-4, 0.7):
        T = float(np.float32(T))
        y = rn32(Fraction(1) / Fraction(T))
        fs = np.concatenate([rng.uniform(-1, 1, 160), rng.uniform(0.2, 0.3, 60), rng.uniform(-1e-3, 1e-3, 20),
                             [1.0, -1.0, 0.0, 0.5, 2.0 ** -20, 1 - 2.0 ** -24]]).astype(np.float32)
        for f in fs:
            f = float(f)
            q = rn32(Fraction(f) * Fraction(y))
            q = fma(fma(-T, q, f), y, q)
            q = fma(fma(-T, q, f), y, q)
            assert q == rn32(Fraction(f) / Fraction(T)), (T, f)


def test_winograd_plan_is_a_pure_function_of_the_layer_not_of_the_batch():
    """Host logic, no GPU: the split over input channels the Winograd launcher would use (dvc_conv2d_winograd_split) and the
    engine choice (ops.winograd_selected) must not depend on the batch size — the clip driver's batched front ends and the
    bit-identical-batch tests rest on it — and the split is one the kernel supports."""
    import ctypes
    from dvc_amd import _lib, ops
    lib = _lib.load()
    ws = 64 << 20
    layers = [(256, 256, 54, 96, 1, 1), (512, 512, 27, 48, 1, 1), (512, 512, 27, 48, 2, 1), (128, 128, 216, 384, 1, 1),
              (64, 64, 216, 384, 1, 1), (512, 512, 13, 24, 1, 1), (256, 64, 13, 24, 1, 2), (128, 256, 54, 96, 1, 1)]
    for (ci, co, H, W, dil, up) in layers:
        got = []
        for N in (1, 2, 5):
            d = _lib.DvcConvDesc(N, ci, H, W, co, 3, 1, dil, dil, 0, up, 1, 1, 0.0, 0, -1, 0, 0, 0, 0, 0)
            sp, ipl = ctypes.c_int32(0), ctypes.c_int32(0)
            assert lib.dvc_conv2d_winograd_split(ctypes.byref(d), ws, ctypes.byref(sp), ctypes.byref(ipl)) == 0, lib.dvc_last_error()
            got.append(sp.value)
            # images one launch covers: the whole batch unless the workspace (partial sums of the split) or the
            # 65535-workgroup cap says otherwise — then the host must not defer the reduce (ops.conv2d_winograd)
            cap = ws // (sp.value * co * (H * up) * (W * up) * 4) if sp.value > 1 else N
            assert 1 <= ipl.value <= N and ipl.value <= max(cap, 1)
            assert ops.winograd_selected(N, ci, H, W, co, dil=dil, pad=dil, in_up=up) == \
                ops.winograd_selected(1, ci, H, W, co, dil=dil, pad=dil, in_up=up)
        assert got[0] == got[1] == got[2] and 1 <= got[0] <= 8, (ci, co, H, W, got)
    # without a workspace there is nothing to split into
    d = _lib.DvcConvDesc(1, 256, 54, 96, 256, 3, 1, 1, 1, 0, 1, 1, 1, 0.0, 0, -1, 0, 0, 0, 0, 0)
    sp, ipl = ctypes.c_int32(0), ctypes.c_int32(0)
    assert lib.dvc_conv2d_winograd_split(ctypes.byref(d), 0, ctypes.byref(sp), ctypes.byref(ipl)) == 0 and sp.value == 1
    # a batch whose partial sums do not fit the workspace is covered in several launches: images_per_launch < N
    big = _lib.DvcConvDesc(64, 64, 216, 384, 64, 3, 1, 1, 1, 0, 1, 1, 1, 0.0, 0, -1, 2, 0, 0, 0, 0)
    assert lib.dvc_conv2d_winograd_split(ctypes.byref(big), ws, ctypes.byref(sp), ctypes.byref(ipl)) == 0
    assert sp.value == 2 and ipl.value == ws // (2 * 64 * 216 * 384 * 4) < 64
    # a layer the kernel does not take is refused with a message, not planned
    bad = _lib.DvcConvDesc(1, 3, 54, 96, 64, 3, 1, 1, 1, 0, 1, 1, 1, 0.0, 0, -1, 0, 0, 0, 0, 0)
    assert lib.dvc_conv2d_winograd_split(ctypes.byref(bad), ws, ctypes.byref(sp), ctypes.byref(ipl)) != 0
    assert b"Cin" in lib.dvc_last_error()


def test_batch_plan_flag_trades_the_split_for_the_batch():
    """DVC_CONV_BATCH_PLAN (include/dvc_hip.h): the plan of the WHOLE batch — the multi-reference pass runs R ColorVidNet
    recurrences in lock step, so the R images' workgroups fill the chip together and an under-filled layer needs a smaller
    split over input channels (or none).  Host logic: the flag never changes a single image's plan, never raises the split,
    lowers it on the network's under-filled layers at R = 4, and `ops.batch_plan` sets it only while active."""
    import ctypes
    from dvc_amd import _lib, ops
    lib = _lib.load()
    ws = 64 << 20

    def split(N, ci, co, H, W, dil, flags):
        d = _lib.DvcConvDesc(N, ci, H, W, co, 3, 1, dil, dil, 0, 1, 1, 1, 0.0, 0, -1, 0, 0, 0, 0, flags)
        sp, ipl = ctypes.c_int32(0), ctypes.c_int32(0)
        assert lib.dvc_conv2d_winograd_split(ctypes.byref(d), ws, ctypes.byref(sp), ctypes.byref(ipl)) == 0, lib.dvc_last_error()
        return sp.value

    lowered = 0
    for (ci, co, H, W, dil) in [(256, 256, 54, 96, 1), (512, 512, 27, 48, 1), (512, 512, 27, 48, 2), (128, 128, 216, 384, 1),
                                (256, 256, 108, 192, 1), (128, 256, 54, 96, 1)]:
        base = split(1, ci, co, H, W, dil, 0)
        assert split(1, ci, co, H, W, dil, ops.BATCH_PLAN) == base
        assert split(4, ci, co, H, W, dil, 0) == base
        s4 = split(4, ci, co, H, W, dil, ops.BATCH_PLAN)
        assert 1 <= s4 <= base, (ci, co, H, W, base, s4)
        lowered += s4 < base
    assert lowered >= 2
    assert ops._plan_flags(4) == 0
    with ops.batch_plan(True):
        assert ops._plan_flags(4) == ops.BATCH_PLAN and ops._plan_flags(1) == 0
        with ops.batch_plan(False):
            assert ops._plan_flags(4) == 0
    assert not ops.batch_plan_enabled()


def _wino_split(lib, ws, *shape, **kw):
    import ctypes
    from dvc_amd import ops
    d = ops._conv_desc(*shape, **kw)
    sp, ipl = ctypes.c_int32(0), ctypes.c_int32(0)
    assert lib.dvc_conv2d_winograd_split(ctypes.byref(d), ws, ctypes.byref(sp), ctypes.byref(ipl)) == 0, lib.dvc_last_error()
    return sp.value, ipl.value


def test_winograd_plans_of_the_multi_pass_cases():
    """Host logic, no GPU: the (split, images_per_launch) of every case of tests/test_gpu_conv_batch_passes.py, so that a change
    of the planner that would quietly turn those cases into single-pass launches fails here first; and the two refusals of
    dvc_conv2d_winograd that are decided before any launch."""
    import ctypes
    from dvc_amd import _lib, ops
    lib = _lib.load()
    H, W, N = 13, 23, 5
    per = 64 * H * W * 4                      # bytes of one image's output, Cout = 64
    # workspace-limited: the workspace holds the partial sums of k of the 5 images
    for dil, S, k in [(1, 2, 2), (1, 3, 2), (2, 2, 2), (1, 2, 1)]:
        assert _wino_split(lib, k * S * per, N, 64, H, W, 64, dil=dil, act=1, split_k=S) == (S, k)
    assert _wino_split(lib, 2 * 2 * per, N, 16, H, W, 64, act=1, split_k=2) == (2, 2)                                  # pool
    assert _wino_split(lib, 2 * 2 * 64 * 14 * 22 * 4, N, 16 + 24, 14, 22, 64, act=1, cfg=9, split_k=2) == (2, 2)       # dual
    # the 65535-workgroup cap: cfg, split, Cin, H x W, dil, workgroups per image, N
    for cfg, S, Cin, h, dil, per_image, n in [(12, 1, 8, 2, 1, 2, 32770), (8, 2, 16, 2, 1, 2, 32770), (8, 1, 8, 4, 2, 4, 16386)]:
        ws = 64 << 20 if S > 1 else 4096
        sp, ipl = _wino_split(lib, ws, n, Cin, h, h, 64, dil=dil, act=1, cfg=cfg, split_k=S)
        assert (sp, ipl) == (S, 65535 // per_image) and n - ipl == 3
        assert ipl * per_image < 65536 <= (ipl + 1) * per_image       # index 65536 is never handed to the 16-bit decode
        if S > 1:
            assert ws // (S * 64 * h * h * 4) == 32768 > ipl          # the workspace alone would allow one image more
    # dvc_amd.ops cases: 8192 images at 8 workgroups each are one workgroup too many; conv3x3_group's two layers
    assert _wino_split(lib, 64 << 20, 8192, 64, 2, 2, 64, act=1, split_k=8) == (8, 8191)
    assert 8 * 8192 * 64 * 2 * 2 * 4 == ops.CONV_WORKSPACE_BYTES
    for Cin in (64, 128):
        S = _wino_split(lib, ops.CONV_WORKSPACE_BYTES, N, Cin, 13, 25, 64, act=1)[0]
        assert S > 1 and _wino_split(lib, 2 * S * 64 * 13 * 25 * 4, N, Cin, 13, 25, 64, act=1) == (S, 2)
    # a single image that needs 65536 workgroups or more is not planned into a launch (-1; the launcher refuses it)
    assert _wino_split(lib, 4096, 1, 8, 2048, 2048, 64, cfg=12, split_k=1) == (1, -1)
    # refused before any launch (no pointer is read): a workspace one byte short of ONE image at the forced split ...
    one = ctypes.c_void_p(16)
    d = ops._conv_desc(N, 64, H, W, 64, act=1, split_k=2)
    rc = lib.dvc_conv2d_winograd(ctypes.byref(d), one, one, None, None, None, one, one, 2 * per - 1, None)
    assert rc != 0 and b"too small for one image" in lib.dvc_last_error(), lib.dvc_last_error()
    # ... and a deferred reduce with room for 2 of the 5 images
    d = ops._conv_desc(N, 64, H, W, 64, act=1, split_k=2, flags=ops.DEFER_REDUCE)
    rc = lib.dvc_conv2d_winograd(ctypes.byref(d), one, one, None, None, None, one, one, 2 * 2 * per, None)
    assert rc != 0 and b"DVC_CONV_DEFER_REDUCE needs a workspace that holds the partial sums of the whole batch" in lib.dvc_last_error()


# ---- every refusal of the convolution entry points of csrc/conv_mfma.hip that is decided before any launch: (entry point,
# descriptor shape (N, Cin, H, W, Cout), descriptor fields, argument overrides, substring of the message).  The messages were
# recorded from the library before its launcher was split into check / plan / launch steps.  Arguments default to a dummy
# non-NULL pointer (16) that nothing reads, since every row is refused; `ws`: workspace bytes (0: no workspace).
_S = (1, 16, 8, 8, 32)
_W = (1, 16, 8, 8, 64)
_BIG = (1, 512, 1024, 1024, 64)
CONV_REFUSALS = [
    ("conv2d", None, {}, {}, "dvc_conv2d: null descriptor"),
    ("conv2d", _S, {}, dict(x=None), "dvc_conv2d: null argument"),
    ("conv2d", _S, {}, dict(y=None), "dvc_conv2d: null argument"),
    ("conv2d", _S, dict(ksize=5, pad=2), {}, "dvc_conv2d: ksize must be 1 or 3 (got 5)"),
    ("conv2d", _S, dict(stride=3), {}, "dvc_conv2d: stride must be 1 or 2"),
    ("conv2d", _S, dict(dil=3, pad=2), {}, "dvc_conv2d: dilation must be 1 or 2"),
    ("conv2d", _S, dict(pad=3), {}, "dvc_conv2d: pad must be 0..2"),
    ("conv2d", (1, 16, 8, 8, 6), {}, {}, "dvc_conv2d: Cout must be a multiple of 4 (got 6)"),
    ("conv2d", _S, dict(in_up=3), {}, "dvc_conv2d: bad in_up/in_sub"),
    ("conv2d", _S, dict(in_up=2, in_sub=2), {}, "dvc_conv2d: bad in_up/in_sub"),
    ("conv2d", _S, {}, dict(in_scale=16), "dvc_conv2d: scale/shift must come together"),
    ("conv2d", _S, dict(in_prelu=True), {}, "dvc_conv2d: in_prelu needs in_slope_ptr"),
    ("conv2d", (1, 0, 8, 8, 32), {}, {}, "dvc_conv2d: bad shape"),
    ("conv2d", _S, {}, dict(w=20), "dvc_conv2d: weights must be 16-byte aligned"),
    ("conv2d", (1, 1024, 2048, 1024, 32), {}, {}, "dvc_conv2d: tensor too large for 32-bit indexing"),
    ("conv2d", (1, 16, 1, 1, 32), dict(pad=0), {}, "dvc_conv2d: empty output"),
    ("conv2d", (1, 16, 1, 8, 32), dict(pad_mode=1), {}, "dvc_conv2d: reflect pad needs pad < input size"),
    ("conv2d", _S, dict(w_batch_stride=6), {}, "dvc_conv2d: w_batch_stride must be a multiple of 4 (got 6)"),
    ("conv2d", _W, dict(w_batch_stride=8, cfg=34), dict(ws=1 << 20), "dvc_conv2d: per-image filters run on the general engine only"),
    ("conv2d", (1, 3, 8, 8, 64), dict(cfg=0, flags=4), {}, "dvc_conv2d: DVC_CONV_GRAY_INPUT is for the 3 -> 64 image-input layer"),
    ("conv2d", _S, dict(ksize=1, stride=2, pad=0), {}, "dvc_conv2d: stride-2 / dilated variant supports ksize 3 only"),
    ("conv2d", _W, dict(cfg=33), dict(ws=1 << 20), "dvc_conv2d: the stream-K path has tile configurations 2, 3 and 4 (cfg 34..36)"),
    ("conv2d", _W, dict(cfg=37), dict(ws=1 << 20), "dvc_conv2d: the stream-K path has tile configurations 2, 3 and 4 (cfg 34..36)"),
    ("conv2d", _W, dict(cfg=36), dict(ws=1 << 20, in_scale=16, in_shift=16),
     "dvc_conv2d: the stream-K path needs a plain stride-1 layer (no fused input transform, Cin % 8 == 0, Cout % 64 == 0)"),
    ("conv2d", _S, dict(cfg=34), dict(ws=1 << 20), "dvc_conv2d: the stream-K path needs a plain stride-1 layer"),
    ("conv2d", _W, dict(cfg=36), {}, "dvc_conv2d: the stream-K path needs a workspace"),
    ("conv2d", _BIG, dict(cfg=36), dict(ws=1 << 20), "dvc_conv2d: tensor too large for buffer-descriptor staging"),
    ("conv2d", (1, 8, 4096, 4096, 262144), dict(cfg=36), dict(ws=1 << 20), "dvc_conv2d: too many tiles"),
    ("conv2d", _W, dict(cfg=36), dict(ws=4096), "dvc_conv2d: workspace too small for the stream-K slots"),
    ("conv2d", _S, dict(cfg=5), {}, "dvc_conv2d: cfg out of range"),
    ("conv2d", _S, dict(cfg=21), {}, "dvc_conv2d: cfg out of range"),
    # (the automatic plan of this stride-2 / dilation-2 layer was refused with "no tile configuration fits this geometry" until the
    # planner learnt to fall back to another tile width; a forced configuration that does not fit is still refused)
    ("conv2d", (1, 16, 64, 64, 32), dict(stride=2, dil=2, pad=2, cfg=2), {}, "dvc_conv2d: tile configuration 2 does not fit this geometry"),
    ("conv2d", (1, 16, 64, 64, 32), dict(stride=2, dil=2, pad=2, cfg=0), {}, "dvc_conv2d: tile configuration 0 does not fit this geometry"),
    ("conv2d", (1, 520, 8, 8, 32), {}, dict(in_scale=16, in_shift=16), "dvc_conv2d: fused input affine supports Cin <= 512"),
    ("conv2d", (1, 24000, 8, 8, 64), dict(stride=2), dict(in_scale=16, in_shift=16), "dvc_conv2d: LDS tile too large ("),
    ("winograd", _W, {}, dict(x=None), "dvc_conv2d_winograd: null argument"),
    ("winograd", _W, dict(ksize=1, pad=0), {}, "dvc_conv2d_winograd: needs a 3x3 stride-1 layer with pad == dilation (1 or 2)"),
    ("winograd", _W, dict(pad=2), {}, "dvc_conv2d_winograd: needs a 3x3 stride-1 layer with pad == dilation (1 or 2)"),
    ("winograd", _W, dict(in_prelu=True), {}, "dvc_conv2d_winograd: no fused input transform on this path"),
    ("winograd", _W, dict(in_sub=3), {}, "dvc_conv2d_winograd: bad in_up/in_sub"),
    ("winograd", (0, 16, 8, 8, 64), {}, {}, "dvc_conv2d_winograd: bad shape"),
    ("winograd", (1, 4, 8, 8, 64), {}, {}, "dvc_conv2d_winograd: needs Cin % 8 == 0 and Cout % 64 == 0 (got 4, 64)"),
    ("winograd", _S, {}, {}, "dvc_conv2d_winograd: needs Cin % 8 == 0 and Cout % 64 == 0 (got 16, 32)"),
    ("winograd", _W, {}, dict(w=20), "dvc_conv2d_winograd: weights must be 16-byte aligned"),
    ("winograd", _BIG, {}, {}, "dvc_conv2d_winograd: tensor too large for buffer-descriptor staging"),
    ("winograd", (1, 16, 1, 8, 64), dict(pad_mode=1), {}, "dvc_conv2d_winograd: reflect pad needs pad < input size"),
    ("winograd", _W, dict(split_k=2), dict(ws=2 * 64 * 64 * 4 - 1),
     "dvc_conv2d_winograd: split-K workspace too small for one image (split_k 2 needs 32768 bytes, got 32767)"),
    ("winograd", _W, dict(cfg=0), {}, "dvc_conv2d_winograd: no configuration for cfg 0 / split_k 0 on this layer"),
    ("winograd", _W, dict(split_k=3), dict(ws=1 << 20), "dvc_conv2d_winograd: no configuration for cfg -1 / split_k 3 on this layer"),
    ("winograd", (1, 8, 2048, 2048, 64), dict(cfg=12, split_k=1), {},
     "dvc_conv2d_winograd: 65536 workgroups per image (feature map too large for this path)"),
    ("winograd", (5, 16, 8, 8, 64), dict(split_k=2, flags=1), dict(ws=2 * 2 * 64 * 64 * 4),
     "dvc_conv2d_winograd: DVC_CONV_DEFER_REDUCE needs a workspace that holds the partial sums of the whole batch"),
    ("winograd", _W, dict(split_k=2, flags=1), dict(ws=1 << 20, residual=16), "dvc_conv2d_winograd: DVC_CONV_DEFER_REDUCE does not carry a residual"),
    ("pool", None, {}, {}, "dvc_conv2d_winograd_pool: null argument"),
    ("pool", _W, {}, dict(y_pool=None), "dvc_conv2d_winograd_pool: null argument"),
    ("pool", _W, dict(dil=2), {}, "dvc_conv2d_winograd_pool: dilation 1, no deferred reduce"),
    ("pool", _W, dict(flags=1), {}, "dvc_conv2d_winograd_pool: dilation 1, no deferred reduce"),
    ("pool", (1, 16, 1, 8, 64), {}, {}, "dvc_conv2d_winograd_pool: output smaller than a pooling window"),
    ("pool", _W, {}, dict(x=None), "dvc_conv2d_winograd: null argument"),
    ("pool", _S, {}, dict(y=None), "dvc_conv2d_winograd: needs Cin % 8 == 0 and Cout % 64 == 0 (got 16, 32)"),
    ("dual", _W, {}, dict(x2=None), "dvc_conv2d_winograd_dual: null argument"),
    ("dual", _W, {}, dict(d2=None), "dvc_conv2d_winograd_dual: null argument"),
    ("dual", _W, {}, dict(d2=((2, 8, 8, 8, 64), {})), "dvc_conv2d_winograd_dual: the two convolutions must agree in batch"),
    ("dual", _W, {}, dict(d2=((1, 8, 8, 8, 64), dict(dil=2))), "dvc_conv2d_winograd_dual: the two convolutions must agree in batch"),
    ("dual", _W, {}, dict(d2=((1, 4, 8, 8, 64), {})), "dvc_conv2d_winograd_dual: both channel counts must be multiples of 8"),
    ("dual", _W, {}, dict(d2=((1, 8, 8, 8, 64), dict(in_up=3))), "dvc_conv2d_winograd_dual: bad in_up/in_sub of the second input"),
    ("dual", _W, dict(flags=1), dict(d2=((1, 8, 8, 8, 64), {})), "dvc_conv2d_winograd_dual: no deferred reduce on this entry"),
    ("dual", _W, {}, dict(d2=((1, 8, 9, 8, 64), {})), "dvc_conv2d_winograd_dual: the two inputs' virtual sizes differ (8 x 8 vs 9 x 8)"),
    ("dual", _W, dict(in_up=2), dict(d2=((1, 8, 8, 8, 64), {})), "dvc_conv2d_winograd_dual: the two inputs' virtual sizes differ (16 x 16 vs 8 x 8)"),
    ("dual", (1, 8, 512, 512, 64), dict(in_up=2), dict(d2=((1, 512, 1024, 1024, 64), {})), "dvc_conv2d_winograd_dual: second input too large"),
    ("dual", _W, dict(ksize=1, pad=0), dict(d2=((1, 8, 8, 8, 64), {})), "dvc_conv2d_winograd: needs a 3x3 stride-1 layer"),
    ("group", [], {}, {}, "dvc_conv2d_winograd_group: 1..4 items"),
    ("group", [(_W, {}, {})] * 5, {}, {}, "dvc_conv2d_winograd_group: 1..4 items"),
    ("group", [(_W, {}, {}), (_W, {}, dict(x=None))], {}, {}, "dvc_conv2d_winograd_group: null argument in item 1"),
    ("group", [(_W, {}, {}), (_W, {}, {})], {}, {}, "dvc_conv2d_winograd_group: items 0 and 1 share an output"),
    ("group", [(_W, {}, {}), (_S, {}, dict(y=32))], {}, {}, "dvc_conv2d_winograd: needs Cin % 8 == 0 and Cout % 64 == 0 (got 16, 32)"),
    ("group", [(_W, dict(split_k=2), dict(ws=1 << 20)), (_W, dict(split_k=2), dict(ws=1 << 20, y=32))], {}, {},
     "dvc_conv2d_winograd_group: the split items 0 and 1 share a workspace"),
    ("split", None, {}, {}, "dvc_conv2d_winograd_split: null argument"),
    ("split", _W, dict(stride=2), {}, "dvc_conv2d_winograd: needs a 3x3 stride-1 layer with pad == dilation (1 or 2)"),
    ("split", _W, dict(cfg=0), {}, "dvc_conv2d_winograd_split: no configuration for cfg 0 / split_k 0 on this layer"),
]


def _refusal_call(lib, entry, shape, fields, args):
    """One row of CONV_REFUSALS as a C-ABI call; returns its return code."""
    from dvc_amd import _lib, ops

    def desc(shape, fields):
        return None if shape is None else ctypes.byref(ops._conv_desc(*shape, **fields))

    def p(name, default=16):
        v = args.get(name, default)
        return ctypes.c_void_p(v) if v else None

    ws = args.get("ws", 0)
    wsp = ctypes.c_void_p(4096) if ws else None
    if entry == "conv2d":
        return lib.dvc_conv2d(desc(shape, fields), p("x"), p("w"), None, p("in_scale", None), p("in_shift", None), None, None,
                              p("residual", None), p("y"), wsp, ws, None)
    if entry == "winograd":
        return lib.dvc_conv2d_winograd(desc(shape, fields), p("x"), p("w"), None, None, p("residual", None), p("y"), wsp, ws, None)
    if entry == "pool":
        return lib.dvc_conv2d_winograd_pool(desc(shape, fields), p("x"), p("w"), None, None, p("y"), p("y_pool"), 0, wsp, ws, None)
    if entry == "dual":
        d2 = args.get("d2", ((1, 8, 8, 8, 64), {}))
        return lib.dvc_conv2d_winograd_dual(desc(shape, fields), desc(*d2) if d2 else None, p("x"), p("x2"), p("w"), None, None, p("y"),
                                            wsp, ws, None)
    if entry == "split":
        sp, ipl = ctypes.c_int32(0), ctypes.c_int32(0)
        return lib.dvc_conv2d_winograd_split(desc(shape, fields), 1 << 20, ctypes.byref(sp) if shape else None, ctypes.byref(ipl))
    assert entry == "group"
    items = (_lib.DvcConvGroupItem * max(len(shape), 1))()
    for it, (s, f, a) in zip(items, shape):
        it.d = ops._conv_desc(*s, **f)
        it.x, it.u_packed, it.y = a.get("x", 16), 16, a.get("y", 16)
        it.workspace, it.workspace_bytes = (4096, a["ws"]) if a.get("ws") else (None, 0)
    return lib.dvc_conv2d_winograd_group(items if shape else None, len(shape), None)


@pytest.mark.parametrize("row", range(len(CONV_REFUSALS)), ids=lambda i: f"{CONV_REFUSALS[i][0]}-{i}")
def test_conv_entry_points_refuse_before_any_launch(row):
    """Host logic, no GPU: every DVC_REQUIRE of dvc_conv2d and of the Winograd entry points that fires before a launch, one bad
    descriptor or argument per row, with the message it must produce (and, where two checks could fire, the one that does)."""
    from dvc_amd import _lib
    lib = _lib.load()
    entry, shape, fields, args, message = CONV_REFUSALS[row]
    rc = _refusal_call(lib, entry, shape, fields, args)
    assert rc != 0 and message.encode() in lib.dvc_last_error(), lib.dvc_last_error()


def test_winograd_reciprocal_decode_is_exact_below_65536():
    """csrc/conv_wino_kernel.h decodes the 1-D workgroup index with wino_div(n, wino_magic(d)) = umulhi(n, ceil(2^32 / d))
    (d == 1: magic 0, quotient n) for d = gx * gy, gx, blk_y * blk_x, blk_x and split, all of them <= the grid size.  Restated
    with integers: exact for every divisor 1 .. 65535 at the quotient boundaries of the index range the 65535-workgroup cap
    allows (wino_images_per_launch).  The argument that makes it exact, n * (d * magic - 2^32) < 2^32, needs n < 65536 for
    d up to 65535: the launcher must never build a grid of 65536 workgroups or more, which the plan test above pins."""
    def magic(d):
        return (2 ** 32 + d - 1) // d if d > 1 else 0

    def div(n, m):
        return (n * m) >> 32 if m else n

    for d in range(1, 65536):
        m = magic(d)
        assert m < 2 ** 32
        top = 65535 - 65535 % d
        for n in (0, d - 1, d, top - 1, top, 65535):
            assert div(n, m) == n // d, (n, d)
        assert d == 1 or (d * m - 2 ** 32) * 65535 < 2 ** 32          # the sufficient condition holds up to n = 65535
    # ... and the reciprocal is NOT exact for every larger index (e.g. 93015 / 46508 decodes as 2): the cap is what keeps the
    # decode right, and 65536 is not claimed
    assert div(93015, magic(46508)) == 2 != 93015 // 46508


def test_bench_torchrun_relaunch_command():
    """`python bench.py --gpus N` re-launches itself as the driver does (one rank per GPU under torch.distributed.run, 127.0.0.1
    rendezvous, its own flags passed through): the command line is built here without launching anything."""
    import importlib.util
    import sys
    spec = importlib.util.spec_from_file_location("bench_under_test", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    argv = ["--gpus", "8", "--steps", "20", "--warmup", "5"]
    cmd, env = bench.torchrun_command(8, argv, 29511, environ={"PATH": "/usr/bin"})
    assert cmd[:3] == [sys.executable, "-m", "torch.distributed.run"]
    assert "--nnodes=1" in cmd and "--nproc-per-node=8" in cmd
    assert cmd[cmd.index("--master-addr") + 1] == "127.0.0.1" and cmd[cmd.index("--master-port") + 1] == "29511"
    script = cmd.index(os.path.join(ROOT, "bench.py"))
    assert cmd[script + 1:] == argv                       # the ranks get exactly the caller's flags (--gpus N included)
    assert env["HSA_ENABLE_IPC_MODE_LEGACY"] == "0" and env["PATH"] == "/usr/bin"
    _, env1 = bench.torchrun_command(2, [], 1, environ={"HSA_ENABLE_IPC_MODE_LEGACY": "1"})
    assert env1["HSA_ENABLE_IPC_MODE_LEGACY"] == "1"      # an explicit setting of the caller is kept


def test_error_aware_engine_map_host_logic():
    """ops.winograd_selected with named layers: under `auto` the layers of the engine map stay on the direct engine, `speed` is
    the geometry rule alone, `winograd` / `direct` force one engine; the map never depends on the batch size; every name in the
    built-in map is a real 3x3 layer of one of the three networks."""
    from dvc_amd import arch, ops
    old_algo, old_map = ops.conv_algo(), ops._direct_layers
    try:
        geo = dict(dil=1, pad=1)
        ops.set_conv_algo("auto")
        ops.set_direct_layers(["cvn.conv2_2"])
        assert not ops.winograd_selected(1, 128, 108, 192, 128, layer="cvn.conv2_2", **geo)
        assert not ops.winograd_selected(4, 128, 108, 192, 128, layer="cvn.conv2_2", **geo)
        assert ops.winograd_selected(1, 128, 108, 192, 128, layer="cvn.conv9_2", **geo)
        assert ops.winograd_selected(1, 128, 108, 192, 128, **geo)                  # unnamed calls: geometry rule
        ops.set_conv_algo("speed")
        assert ops.winograd_selected(1, 128, 108, 192, 128, layer="cvn.conv2_2", **geo)
        ops.set_conv_algo("winograd")
        assert ops.winograd_selected(1, 128, 108, 192, 128, layer="cvn.conv2_2", **geo)
        ops.set_conv_algo("direct")
        assert not ops.winograd_selected(1, 128, 108, 192, 128, layer="cvn.conv9_2", **geo)
        ops.set_direct_layers(None)
        assert ops.direct_layers() == arch.DIRECT_LAYERS
        with pytest.raises(ValueError):
            ops.set_conv_algo("fastest")
    finally:
        ops.set_conv_algo(old_algo)
        ops._direct_layers = old_map
    names = {"vgg." + n for n, _, _ in arch.VGG_CONVS}
    names |= {f"warp.{h}.{ci}" for h in arch.WARP_HEAD_ORDER for (ci, _, _, _, _) in arch.WARP_HEADS[h]["convs"]}
    names |= {f"warp.layer.{b}.conv{k}" for b in range(arch.WARP_NUM_RESBLOCKS) for k in (1, 2)}
    names |= {"cvn." + c["key"] for c in arch.CVN_CONVS}
    assert arch.DIRECT_LAYERS <= names, sorted(arch.DIRECT_LAYERS - names)


def test_exemplar_memo_keys_on_identity_versions_and_weights():
    """nets.WarpNet._memo_exemplar_side (the cache behind the reference's unmodified call pattern), on CPU tensors with a
    counting stand-in for the exemplar side: hit on the same tensor objects, miss on new objects, on an in-place write
    (version counter), on a parameter update, on another regime / engine choice; off switch."""
    import contextlib
    import io
    from dvc_amd import ops
    from dvc_amd.nets import WarpNet
    with contextlib.redirect_stdout(io.StringIO()):
        net = WarpNet(1)
    calls = []

    def compute():
        calls.append(1)
        return ("phi%d" % len(calls), "blab")

    a, b = torch.zeros(3), torch.zeros(4)
    v1 = net._memo_exemplar_side((a, b), ("warp_color", False), compute)
    assert net._memo_exemplar_side((a, b), ("warp_color", False), compute) is v1 and len(calls) == 1
    assert net._memo_exemplar_side((a.clone(), b), ("warp_color", False), compute) is not v1 and len(calls) == 2     # new object
    net._memo_exemplar_side((a, b), ("warp_color", False), compute)
    n = len(calls)
    a.add_(1.0)                                                                                                      # in-place write
    net._memo_exemplar_side((a, b), ("warp_color", False), compute)
    assert len(calls) == n + 1
    net._memo_exemplar_side((a, b), ("warp_color", True), compute)                                                   # other regime
    assert len(calls) == n + 2
    with torch.no_grad():
        net.theta.weight.mul_(2.0)                                                                                    # parameter update
    net._memo_exemplar_side((a, b), ("warp_color", True), compute)
    assert len(calls) == n + 3
    old = ops.conv_algo()
    try:
        ops.set_conv_algo("direct")
        net._memo_exemplar_side((a, b), ("warp_color", True), compute)
        assert len(calls) == n + 4
    finally:
        ops.set_conv_algo(old)
    ops.set_exemplar_memo(False)
    try:
        net._memo_exemplar_side((a, b), ("warp_color", True), compute)
        net._memo_exemplar_side((a, b), ("warp_color", True), compute)
        assert len(calls) == n + 6
    finally:
        ops.set_exemplar_memo(True)
    # the memo is not part of the module's state
    assert not any("memo" in k for k in net.state_dict())
    # r06: tensors without a version counter (torch.inference_mode) bypass the memo instead of raising
    with torch.inference_mode():
        ai = torch.zeros(3)
    n = len(calls)
    net._memo_exemplar_side((ai, b), ("warp_color", True), compute)
    net._memo_exemplar_side((ai, b), ("warp_color", True), compute)
    assert len(calls) == n + 2
    # "verify": every hit recomputes and compares; a stand-in whose value changes between calls is reported and replaced
    import warnings
    ops.set_exemplar_memo("verify")
    try:
        state = {"v": torch.ones(2)}
        comp = lambda: (calls.append(1), (state["v"].clone(), "blab"))[1]        # noqa: E731
        net._memo_exemplar_side((a, b), ("warp_color", False), comp)
        n = len(calls)
        with warnings.catch_warnings(record=True) as w:
            warnings.simplefilter("always")
            r = net._memo_exemplar_side((a, b), ("warp_color", False), comp)
        assert len(calls) == n + 1 and not w and torch.equal(r[0], torch.ones(2))
        state["v"] = torch.full((2,), 2.0)          # "the exemplar changed through .data": same identities, same versions
        with warnings.catch_warnings(record=True) as w:
            warnings.simplefilter("always")
            r = net._memo_exemplar_side((a, b), ("warp_color", False), comp)
        assert torch.equal(r[0], torch.full((2,), 2.0)) and any(issubclass(x.category, RuntimeWarning) for x in w)
    finally:
        ops.set_exemplar_memo(True)
    assert ops.exemplar_memo_mode() == "on"


def test_training_side_gemm_guard_refuses_reduced_precision_and_cpu_tensors():
    """ops.bmm (r06: the training side's plain batched GEMMs on the vendor library) computes in plain fp32 or not at all: a
    relaxed float32 matmul precision raises (with the way out in the message), and so do CPU tensors — no silent fallback."""
    import torch
    from dvc_amd import ops
    before = torch.get_float32_matmul_precision()
    try:
        torch.set_float32_matmul_precision("high")
        with pytest.raises(RuntimeError, match="DVC_GEMM_LIB=0"):
            ops.bmm(torch.zeros(1, 2, 2), torch.zeros(1, 2, 2))
    finally:
        torch.set_float32_matmul_precision(before)
    with pytest.raises(RuntimeError, match="ROCm tensor"):
        ops.bmm(torch.zeros(1, 2, 2), torch.zeros(1, 2, 2))
    assert ops.gemm_lib() in (True, False)


# ---- the switch registry of dvc_amd/ops.py.  Getter value for the variable unset, "0", "1" and "yes", recorded from the commit
# before the registry (93d8697), where every switch parsed its variable by hand: `== "1"` for some, `!= "0"` for the others.
_DL = ["cvn.conv1_1.2", "cvn.conv1_2", "cvn.conv2_1", "cvn.conv2_2", "cvn.conv3_1", "cvn.conv3_2"]
ENV_PARSE = {
    # variable:            (getter,              unset,  "0",    "1",   "yes")
    "DVC_AUTOTUNE":        ("autotune_enabled",   False,  False,  True,  False),
    "DVC_WS_CONV":         ("ws_conv_enabled",    True,   False,  True,  True),
    "DVC_POOL_FUSION":     ("pool_fusion",        True,   False,  True,  True),
    "DVC_DUAL_CONV":       ("dual_conv_enabled",  True,   False,  True,  False),
    "DVC_FUSE_REDUCE":     ("fuse_reduce",        True,   False,  True,  False),
    "DVC_CONV_ALGO":       ("conv_algo",          "auto", "0",    "1",   "yes"),
    "DVC_EXEMPLAR_MEMO":   ("exemplar_memo_mode", "on",   "off",  "on",  "on"),
    "DVC_GEMM_LIB":        ("gemm_lib",           True,   False,  True,  True),
    "DVC_GRAY_FUSION":     ("gray_fusion",        True,   False,  True,  True),
    "DVC_GROUP_HEADS":     ("group_heads",        True,   False,  True,  True),
    "DVC_FOLD_MERGE":      ("fold_merge",         True,   False,  True,  False),
    "DVC_DIRECT_LAYERS":   ("direct_layers",      _DL,    ["0"],  ["1"], ["yes"]),
}


def test_switch_registry_parses_each_variable_as_before():
    """A fresh interpreter per setting (the variables are read at import), every variable of the registry set to the same string:
    each getter reports what the hand-written parse of the parent commit reported.  Importing ops loads no library."""
    import json
    import subprocess
    import sys
    from dvc_amd import ops
    envs = {sw.env: sw.getter for sw in ops._SWITCHES if sw.env}
    assert envs == {k: v[0] for k, v in ENV_PARSE.items()}                   # every entry of the registry is covered, by its getter
    code = ("import json, sys; from dvc_amd import ops, _lib; assert _lib._lib is None; "
            "v = {g: getattr(ops, g)() for g in sys.argv[1:]}; v['direct_layers'] = sorted(v['direct_layers']); print(json.dumps(v))")
    pkg = os.path.join(ROOT, "deep-exemplar-based-video-colorization_amd")
    for col, value in enumerate((None, "0", "1", "yes")):
        env = {k: v for k, v in os.environ.items() if k not in ENV_PARSE}
        env["PYTHONPATH"] = pkg + os.pathsep + env.get("PYTHONPATH", "")
        if value is not None:
            env.update({k: value for k in ENV_PARSE})
        out = subprocess.run([sys.executable, "-c", code] + list(envs.values()), env=env, capture_output=True, text=True)
        assert out.returncode == 0, out.stderr
        got = json.loads(out.stdout)
        for var, row in ENV_PARSE.items():
            assert got[row[0]] == row[1 + col], (var, value, got[row[0]], row[1 + col])


def test_graph_epoch_follows_every_launch_deciding_switch():
    """graph._epoch() is nets.pack_epoch() plus the registry's launch-deciding entries: flipping each of them through its public
    setter changes the tuple and restoring it restores the tuple; gemm_lib and exemplar_memo (not launch-deciding) do not."""
    from dvc_amd import graph, ops
    flips = {
        "autotune_enabled": (lambda: ops.set_autotune(not ops.autotune_enabled()),) * 2,
        "ws_conv_enabled": (lambda: ops.set_ws_conv(not ops.ws_conv_enabled()),) * 2,
        "pool_fusion": (lambda: ops.set_pool_fusion(not ops.pool_fusion()),) * 2,
        "dual_conv_enabled": (lambda: ops.set_dual_conv(not ops.dual_conv_enabled()),) * 2,
        "fuse_reduce": (lambda: ops.set_fuse_reduce(not ops.fuse_reduce()),) * 2,
        "conv_algo": (lambda: ops.set_conv_algo("direct"), lambda old=ops.conv_algo(): ops.set_conv_algo(old)),
        "gray_fusion": (lambda: ops.set_gray_fusion(not ops.gray_fusion()),) * 2,
        "group_heads": (lambda: ops.set_group_heads(not ops.group_heads()),) * 2,
        "fold_merge": (lambda: ops.set_fold_merge(not ops.fold_merge()),) * 2,
        "direct_layers": (lambda: ops.set_direct_layers(["vgg.conv3_1"]), lambda old=ops._direct_layers: ops.set_direct_layers(old)),
    }
    launch = [sw.getter for sw in ops._SWITCHES if sw.launch]
    assert sorted(launch) == sorted(list(flips) + ["batch_plan_enabled"])
    assert sorted(sw.getter for sw in ops._SWITCHES if not sw.launch) == ["exemplar_memo_mode", "gemm_lib"]
    base = graph._epoch()
    assert len(base) == 1 + len(launch)
    for name, (flip, restore) in flips.items():
        flip()
        try:
            assert graph._epoch() != base, name
        finally:
            restore()
        assert graph._epoch() == base, name
    with ops.batch_plan(not ops.batch_plan_enabled()):
        assert graph._epoch() != base
    assert graph._epoch() == base
    old_gemm, old_memo = ops.gemm_lib(), ops.exemplar_memo_mode()
    try:
        ops.set_gemm_lib(not old_gemm)
        ops.set_exemplar_memo(old_memo == "off")
        assert graph._epoch() == base
    finally:
        ops.set_gemm_lib(old_gemm)
        ops.set_exemplar_memo("verify" if old_memo == "verify" else old_memo == "on")
    assert (ops.gemm_lib(), ops.exemplar_memo_mode()) == (old_gemm, old_memo)


# what the five convolution wrappers (and the grouped launch) appended to ops.conv_record at 93d8697 for the calls below
_R = dict(ksize=3, stride=1, dil=1, pad=1, pad_mode=0, in_up=1, in_sub=1, affine=False, in_prelu=False, residual=False)
CONV_RECORDS = [
    dict(N=2, Cin=8, H=27, W=45, Cout=16, ksize=3, stride=2, dil=1, pad=1, pad_mode=1, in_up=1, in_sub=1, affine=True, in_prelu=True,
         residual=False, act=1),                                                                          # conv2d: no `algo`
    dict(N=1, Cin=16, H=12, W=20, Cout=8, ksize=1, stride=1, dil=1, pad=0, pad_mode=0, in_up=1, in_sub=1, affine=False,
         in_prelu=False, residual=True, act=0),
    dict(_R, N=2, Cin=64, H=24, W=40, Cout=128, act=3, algo="direct-ws"),                                 # conv2d_ws
    dict(_R, N=2, Cin=64, H=13, W=24, Cout=128, dil=2, pad=2, pad_mode=1, in_up=2, residual=True, act=2, algo="winograd"),
    dict(_R, N=1, Cin=64, H=24, W=40, Cout=64, act=1, algo="winograd"),                                   # conv2d_winograd_pool
    dict(_R, N=2, Cin=192, H=24, W=40, Cout=64, act=3, algo="winograd-dual"),              # virtual size, summed input channels
    dict(_R, N=1, Cin=64, H=54, W=96, Cout=64, act=0, algo="winograd"),                                   # conv3x3_group, item 0
    dict(_R, N=1, Cin=64, H=27, W=48, Cout=64, pad_mode=1, in_up=2, act=0, algo="winograd"),              # conv3x3_group, item 1
]
LAYER_RECORDS = [
    dict(layer="warp.layer2_1.3", Cin=64, Cout=64, H=54, W=96, dil=1, in_up=1, in_sub=1, eligible=True),
    dict(layer=None, Cin=64, Cout=64, H=27, W=48, dil=1, in_up=2, in_sub=1, eligible=True),
    dict(layer="x.y", Cin=8, Cout=16, H=20, W=30, dil=1, in_up=1, in_sub=1, eligible=False),
]


def test_conv_and_layer_records_are_what_they_were(monkeypatch):
    """ops._record_conv / ops.record_layer, directly and through the wrappers' call sites (CPU tensors, a library stand-in that
    launches nothing): key for key and value for value the dicts the parent commit wrote out by hand —
    including the general engine's missing `algo` and the dual launch's virtual size."""
    from dvc_amd import _lib, ops

    d = ops._conv_desc(2, 64, 13, 24, 128, dil=2, pad_mode=ops.PAD_REFLECT, in_up=2, act=ops.ACT_PRELU)
    r = ops._record_conv(d, affine=False, in_prelu=False, residual=True, algo="winograd")
    assert r == CONV_RECORDS[3]
    d = ops._conv_desc(2, 8, 27, 45, 16, stride=2, pad=1, pad_mode=ops.PAD_REFLECT, act=ops.ACT_RELU, in_prelu=True)
    r = ops._record_conv(d, affine=True, in_prelu=True, residual=False)
    assert r == CONV_RECORDS[0] and "algo" not in r
    assert (d.in_prelu, d.cfg, d.split_k, d.x_batch_stride, d.y_batch_stride, d.res_batch_stride, d.flags, d.w_batch_stride) == \
        (1, -1, 0, 0, 0, 0, 0, 0)

    class Stub:
        def __getattr__(self, name):
            def call(*args):
                if name == "dvc_conv2d_winograd_split":
                    args[2]._obj.value, args[3]._obj.value = 2, 99
                return 0
            return call

    monkeypatch.setattr(_lib, "_lib", Stub())
    monkeypatch.setattr(ops, "_need", lambda t, name: None)
    monkeypatch.setattr(ops, "_stream", lambda: None)
    monkeypatch.setattr(ops, "_stream_handle", lambda: 0)
    monkeypatch.setattr(ops, "_ws_cache", {})
    monkeypatch.setattr(ops, "conv_record", [])
    monkeypatch.setattr(ops, "layer_record", [])
    T = torch.zeros
    ops.conv2d(T(2, 8, 27, 45), T(8, 9, 16), None, stride=2, pad=1, pad_mode=ops.PAD_REFLECT, act=ops.ACT_RELU, in_scale=T(16),
               in_shift=T(16), in_slope_t=T(1))
    ops.conv2d(T(1, 16, 12, 20), T(16, 1, 8), None, ksize=1, pad=0, residual=T(1, 8, 12, 20))
    ops.conv2d_ws(T(2, 64, 24, 40), T(128 * 64 * 9), None, 128, act=ops.ACT_LEAKY, act_slope=0.2)
    ops.conv2d_winograd(T(2, 64, 13, 24), T(4, 64, 4, 32, 4), None, dil=2, pad_mode=ops.PAD_REFLECT, in_up=2, act=ops.ACT_PRELU,
                        residual=T(2, 128, 26, 48))
    ops.conv2d_winograd_pool(T(1, 64, 24, 40), T(2, 64, 4, 32, 4), None, act=ops.ACT_RELU)
    ops.conv2d_winograd_dual(T(2, 128, 12, 20), T(2, 64, 24, 40), T(2, 192, 4, 32, 4), None, in_upA=2, act=ops.ACT_LEAKY, act_slope=0.2)
    w, u = T(64, 64, 3, 3), T(2, 64, 4, 32, 4)
    ops.conv3x3_group([dict(x=T(1, 64, 54, 96), weight=w, packs=lambda kind: u, bias=None, defer_reduce=True, layer="warp.layer2_1.3"),
                       dict(x=T(1, 64, 27, 48), weight=w, packs=lambda kind: u, bias=None, in_up=2, pad_mode=ops.PAD_REFLECT)])
    assert ops.conv_record == CONV_RECORDS
    ops.conv3x3(T(1, 8, 20, 30), T(16, 8, 3, 3), lambda kind: T(8, 9, 16), None, layer="x.y")
    assert ops.layer_record == LAYER_RECORDS
    assert "algo" not in ops.conv_record[-1]                        # (the 8 -> 16 layer went to the general engine)


def test_instnorm_fma_form_error_bound_is_satisfiable():
    """The bound tests/test_gpu_glue_edges.py asserts of the InstanceNorm kernels over the mean / sigma sweep, checked here on
    the same inputs against a numpy emulation of a CORRECT y = fma(x, sc, sh) (float32-rounded sc and sh, one rounding of the
    result): the bound 2^-23 * (max|x| * rstd + max|y| + 1) holds for every ratio, so a kernel that misses it is wrong."""
    import numpy as np

    import instnorm_bound as IB
    errs = []
    for R in IB.RATIOS:
        x = IB.sweep_plane(R)
        y, rstd, mean = IB.reference(x)
        assert abs(mean - R) < 0.1 and abs(rstd - 1.0) < 0.05       # the sweep is what it says: sigma = 1, mean = R
        err = np.abs(IB.emulate_fma(x).astype(np.float64) - y).max()
        assert err <= IB.bound(x), (R, err, IB.bound(x))
        errs.append(err)
    # the error of this form grows with the ratio (ATen's (x - mean) * rstd stays at an ulp of y): the bound is not idle
    assert errs[-1] > 20 * errs[0]
