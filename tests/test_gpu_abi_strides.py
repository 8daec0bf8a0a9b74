"""GPU: the input-side batch strides of the C-ABI (include/dvc_hip.h) — DvcConvDesc.x_batch_stride / res_batch_stride,
pool_batch_stride of dvc_conv2d_winograd_pool, x / res strides of the InstanceNorm entries, l_batch_stride of dvc_gray2rgb.
dvc_amd/ops.py passes 0 for all of them but the gray-input conv1_1, so the entries are called directly.

Harness: the input is channels [8 : 8 + Cin] of a wider [N, Cin + 16, H, W] tensor, the residual channels [8 : 8 + Cout] of a
wider [N, Cout + 16, OH, OW] tensor, every other channel NaN (a neighbour's value times a zero mask is still a defect).  N = 2,
so image 1's base matters.  Per case: no NaN in the output; bit-identical to the same entry on contiguous copies with
strides 0 (every plan is per image); the float64 reference at the engine's existing tolerance (direct 2e-5, Winograd 5e-5)."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

from cabi_helpers import NAN, check as _check, lib, ops, ptr as _p  # noqa: F401  (ops, lib: fixtures)
from test_gpu_ops import ref_conv, relerr

pytestmark = pytest.mark.gpu
DIRECT_TOL, WINO_TOL = 2e-5, 5e-5


def _wide(t):
    """(view, batch stride in elements): `t` [N, C, H, W] as channels [8 : 8 + C] of a NaN-filled [N, C + 16, H, W] tensor."""
    if t is None:
        return None, 0
    N, C, H, W = t.shape
    big = torch.full((N, C + 16, H, W), NAN, device="cuda")
    big[:, 8:8 + C] = t.cuda()
    return big[:, 8:8 + C], (C + 16) * H * W


def _dense(t):
    return (None, 0) if t is None else (t.cuda().contiguous(), 0)


def _ws(ops):
    ws = ops._workspace(torch.device("cuda", torch.cuda.current_device()), ops.CONV_WORKSPACE_BYTES, "conv")
    return ctypes.c_void_p(ws.data_ptr()), ws.numel()


def _both(run, x, res, OUT):
    """run(x_view, x_bs, res_view, res_bs, y) on the strided and on the contiguous operands, into NaN-filled outputs."""
    outs = []
    for place in (_wide, _dense):
        xv, xbs = place(x)
        rv, rbs = place(res)
        y = torch.full(OUT, NAN, device="cuda")
        run(xv, xbs, rv, rbs, y)
        torch.cuda.synchronize()
        outs.append(y)
    return outs


def _assert_case(strided, dense, ref, tol, what):
    assert not torch.isnan(strided).any(), what
    assert torch.equal(strided, dense), what
    e = relerr(strided, ref)
    assert e < tol, (what, e)


def _data(seed, N, Cin, Cout, H, W, ks, OH, OW, res):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(N, Cin, H, W, generator=g)
    w = torch.randn(Cout, Cin, ks, ks, generator=g) / (Cin * ks * ks) ** 0.5
    b = torch.randn(Cout, generator=g) * 0.1
    r = torch.randn(N, Cout, OH, OW, generator=g) if res else None
    return g, x, w, b, r


# ---- dvc_conv2d: general engine (register and LDS-DMA staging), split-K, stream-K
#   name, Cin, Cout, H, W, ks, dil, pad, in_up, in_sub, affine + PReLU, residual, act, [(cfg, split_k), ...]
CONV2D = [
    ("plain", 16, 64, 13, 24, 3, 1, 1, 1, 1, False, False, 1, [(-1, 0), (18, 0)]),
    ("affine_prelu", 20, 36, 13, 24, 3, 1, 1, 1, 1, True, False, 0, [(-1, 0)]),            # fused input transform: register staging
    ("up_res", 32, 64, 13, 24, 3, 1, 1, 2, 1, False, True, 1, [(-1, 0)]),
    ("sub", 16, 64, 27, 48, 3, 1, 1, 1, 2, False, False, 1, [(-1, 0)]),
    ("k1_res", 64, 64, 13, 24, 1, 1, 0, 1, 1, False, True, 0, [(-1, 0)]),
    ("dil2_res_splitk", 96, 64, 13, 24, 3, 2, 2, 1, 1, False, True, 1, [(-1, 2), (-1, 3)]),   # the reduce kernel reads the residual
    ("res_streamk", 32, 64, 13, 24, 3, 1, 1, 1, 1, False, True, 1, [(34, 1), (34, 2), (36, 1), (36, 2)]),
]


@pytest.mark.parametrize("case", CONV2D, ids=[c[0] for c in CONV2D])
def test_conv2d_input_and_residual_strides(ops, lib, case):
    name, Cin, Cout, H, W, ks, dil, pad, in_up, in_sub, transform, use_res, act, plans = case
    N = 2
    OH, OW = ops.conv_out_hw(H, W, ks, 1, dil, pad, in_up, in_sub)
    g, x, w, b, res = _data(len(name) * 101 + Cin, N, Cin, Cout, H, W, ks, OH, OW, use_res)
    scale = shift = slope = None
    if transform:
        scale, shift = torch.rand(N * Cin, generator=g) + 0.5, torch.randn(N * Cin, generator=g) * 0.3
        slope = torch.tensor([0.25])
    ref = ref_conv(x, w, b, ks, 1, dil, pad, 0, in_up, in_sub, scale, shift, slope, res, act, 0.2)
    wp, bd = ops.pack_conv_weight(w.cuda()), b.cuda()
    cu = lambda t: None if t is None else t.cuda()        # noqa: E731
    scd, shd, sld = cu(scale), cu(shift), cu(slope)
    wsp, wsn = _ws(ops)
    for cfg, split_k in plans:
        def run(xv, xbs, rv, rbs, y):
            d = ops._conv_desc(N, Cin, H, W, Cout, ksize=ks, dil=dil, pad=pad, in_up=in_up, in_sub=in_sub, act=act, act_slope=0.2,
                               in_prelu=transform, cfg=cfg, split_k=split_k, x_batch_stride=xbs, res_batch_stride=rbs)
            _check(lib.dvc_conv2d(ctypes.byref(d), _p(xv), _p(wp), _p(bd), _p(scd), _p(shd), _p(sld), None, _p(rv), _p(y),
                                       wsp, wsn, ops._stream()), "dvc_conv2d")
        strided, dense = _both(run, x, res, (N, Cout, OH, OW))
        _assert_case(strided, dense, ref, DIRECT_TOL, (name, cfg, split_k))


def test_conv2d_gray_input_reads_the_l_plane_of_a_lab_tensor(ops, lib):
    """DVC_CONV_GRAY_INPUT (VGG19 conv1_1): x is the L plane of a [N, 3, H, W] Lab tensor, x_batch_stride = 3 H W; the a / b
    planes are NaN here.  Bit-identical to the call on a contiguous [N, 1, H, W] luminance with stride 0 (=> H W)."""
    N, H, W, Cout = 2, 8, 32, 64
    g = torch.Generator().manual_seed(3)
    L = torch.rand(N, 1, H, W, generator=g) * 100 - 50
    w = torch.randn(Cout, 3, 3, 3, generator=g) / 27 ** 0.5
    b = torch.randn(Cout, generator=g) * 0.1
    scale, shift = torch.rand(N * 3, generator=g) + 0.5, torch.randn(N * 3, generator=g) * 0.3
    rgb = ((L + 50.0) / 100.0).expand(N, 3, H, W)                 # gray2rgb_batch(uncenter_l(L)), in float32 as the kernel does
    ref = ref_conv(rgb, w, b, 3, 1, 1, 1, 0, 1, 1, scale, shift, None, None, 1, 0.0)
    lab = torch.full((N, 3, H, W), NAN, device="cuda")
    lab[:, 0:1] = L.cuda()
    wp, bd, scd, shd = ops.pack_conv_weight(w.cuda()), b.cuda(), scale.cuda(), shift.cuda()
    wsp, wsn = _ws(ops)
    outs = []
    for xt, xbs in ((lab, 3 * H * W), (L.cuda().contiguous(), 0)):
        d = ops._conv_desc(N, 3, H, W, Cout, act=1, x_batch_stride=xbs, flags=ops.GRAY_INPUT)
        y = torch.full((N, Cout, H, W), NAN, device="cuda")
        _check(lib.dvc_conv2d(ctypes.byref(d), _p(xt), _p(wp), _p(bd), _p(scd), _p(shd), None, None, None, _p(y), wsp, wsn,
                                   ops._stream()), "dvc_conv2d")
        torch.cuda.synchronize()
        outs.append(y)
    _assert_case(outs[0], outs[1], ref, DIRECT_TOL, "gray input")


# ---- dvc_conv2d_winograd: the three workgroup shapes, the split-K reduce with a residual, dilation 2, reflect + upsample
#   name, Cin, Cout, H, W, dil, pad_mode, in_up, residual, [(cfg, split_k), ...]
WINO = [
    ("shapes", 24, 64, 13, 23, 1, 0, 1, False, [(6, 0), (10, 0)]),          # 64 x 64 and 64 x 32 workgroups
    ("shape_128", 24, 128, 13, 23, 1, 0, 1, False, [(2, 0)]),               # the 128-channel workgroup needs Cout % 128 == 0
    ("res_split2", 32, 128, 13, 24, 1, 0, 1, True, [(1, 2)]),
    ("dil2", 32, 64, 13, 24, 2, 0, 1, False, [(-1, 0)]),
    ("reflect_up", 16, 64, 13, 24, 1, 1, 2, False, [(-1, 0)]),
]


@pytest.mark.parametrize("case", WINO, ids=[c[0] for c in WINO])
def test_conv2d_winograd_input_and_residual_strides(ops, lib, case):
    name, Cin, Cout, H, W, dil, pad_mode, in_up, use_res, plans = case
    N = 2
    OH, OW = ops.conv_out_hw(H, W, 3, 1, dil, dil, in_up, 1)
    g, x, w, b, res = _data(len(name) * 211 + Cin, N, Cin, Cout, H, W, 3, OH, OW, use_res)
    ref = ref_conv(x, w, b, 3, 1, dil, dil, pad_mode, in_up, 1, None, None, None, res, 3, 0.2)
    u, bd = ops.pack_winograd_weight(w.cuda()), b.cuda()
    wsp, wsn = _ws(ops)
    for cfg, split_k in plans:
        def run(xv, xbs, rv, rbs, y):
            d = ops._conv_desc(N, Cin, H, W, Cout, dil=dil, pad_mode=pad_mode, in_up=in_up, act=3, act_slope=0.2, cfg=cfg,
                               split_k=split_k, x_batch_stride=xbs, res_batch_stride=rbs)
            if split_k > 1:
                assert ops._winograd_split(lib, d, wsn)[0] == split_k
            _check(lib.dvc_conv2d_winograd(ctypes.byref(d), _p(xv), _p(u), _p(bd), None, _p(rv), _p(y), wsp, wsn, ops._stream()),
                   "dvc_conv2d_winograd")
        strided, dense = _both(run, x, res, (N, Cout, OH, OW))
        _assert_case(strided, dense, ref, WINO_TOL, (name, cfg, split_k))


def test_winograd_refuses_plans_a_layer_cannot_take(ops, lib):
    """Why two cases above and below are not 24 -> 64 with cfg 2 and 8 -> 64 with split_k 2: the 128-channel workgroup shape
    (cfg 0..3) needs Cout % 128 == 0, and a split needs two chunks of four input channels per part.  Both are refused cleanly."""
    wsn = ops.CONV_WORKSPACE_BYTES
    with pytest.raises(RuntimeError, match="no configuration"):
        ops._winograd_split(lib, ops._conv_desc(2, 24, 13, 23, 64, cfg=2), wsn)
    with pytest.raises(RuntimeError, match="no configuration"):
        ops._winograd_split(lib, ops._conv_desc(2, 8, 13, 25, 64, split_k=2), wsn)


@pytest.mark.parametrize("Cin,split_k", [(8, 0), (16, 2)], ids=["epilogue", "split_reduce"])
def test_conv2d_winograd_pool_strides(ops, lib, Cin, split_k):
    """8 -> 64 at 13 x 25 (floor-mode pool of odd sizes): x sliced, `y` a channel slice through y_batch_stride and `y_pool` a
    channel slice through pool_batch_stride — written by the convolution's epilogue; and 16 -> 64 (the fewest input channels
    that can be split in two) split over input channels, where the reduce kernel writes both."""
    N, Cout, H, W = 2, 64, 13, 25
    g, x, w, b, _ = _data(77, N, Cin, Cout, H, W, 3, H, W, False)
    ref = ref_conv(x, w, b, 3, 1, 1, 1, 0, 1, 1, None, None, None, None, 1, 0.0)
    ref_pool = F.max_pool2d(ref, 2, 2)
    u, bd = ops.pack_winograd_weight(w.cuda()), b.cuda()
    wsp, wsn = _ws(ops)
    PH, PW = H // 2, W // 2
    got = []
    for sliced in (True, False):
        xv, xbs = (_wide if sliced else _dense)(x)
        CW = Cout + 16 if sliced else Cout
        yb = torch.full((N, CW, H, W), NAN, device="cuda")
        pb = torch.full((N, CW, PH, PW), NAN, device="cuda")
        c0 = 8 if sliced else 0
        d = ops._conv_desc(N, Cin, H, W, Cout, act=1, split_k=split_k, x_batch_stride=xbs, y_batch_stride=CW * H * W if sliced else 0)
        if split_k > 1:
            assert ops._winograd_split(lib, d, wsn)[0] == split_k
        _check(lib.dvc_conv2d_winograd_pool(ctypes.byref(d), _p(xv), _p(u), _p(bd), None, _p(yb[:, c0:]), _p(pb[:, c0:]),
                                                 CW * PH * PW if sliced else 0, wsp, wsn, ops._stream()), "dvc_conv2d_winograd_pool")
        torch.cuda.synchronize()
        if sliced:      # the channels around both destinations are untouched
            for t in (yb, pb):
                assert torch.isnan(t[:, :8]).all() and torch.isnan(t[:, 8 + Cout:]).all()
        got.append((yb[:, c0:c0 + Cout].clone(), pb[:, c0:c0 + Cout].clone()))
    _assert_case(got[0][0], got[1][0], ref, WINO_TOL, ("pool: y", split_k))
    _assert_case(got[0][1], got[1][1], ref_pool, WINO_TOL, ("pool: y_pool", split_k))
    assert torch.equal(got[0][1], F.max_pool2d(got[0][0], 2, 2))


def test_conv2d_winograd_dual_both_inputs_sliced(ops, lib):
    """16 (x2 upsampled) + 8 -> 64 at 26 x 46: each input has its own batch stride (dA / dB)."""
    N, CA, CB, Cout, H, W = 2, 16, 8, 64, 26, 46
    g = torch.Generator().manual_seed(9)
    xA, xB = torch.randn(N, CA, H // 2, W // 2, generator=g), torch.randn(N, CB, H, W, generator=g)
    wA = torch.randn(Cout, CA, 3, 3, generator=g) / (CA * 9) ** 0.5
    wB = torch.randn(Cout, CB, 3, 3, generator=g) / (CB * 9) ** 0.5
    b = torch.randn(Cout, generator=g)
    up = F.interpolate(xA.double(), scale_factor=2, mode="nearest")
    ref = F.relu(F.conv2d(up, wA.double(), b.double(), padding=1) + F.conv2d(xB.double(), wB.double(), None, padding=1))
    u = torch.cat((ops.pack_winograd_weight(wA.cuda()), ops.pack_winograd_weight(wB.cuda())), dim=1).contiguous()
    bd = b.cuda()
    wsp, wsn = _ws(ops)
    outs = []
    for place in (_wide, _dense):
        (av, abs_), (bv, bbs) = place(xA), place(xB)
        dA = ops._conv_desc(N, CA, H // 2, W // 2, Cout, in_up=2, act=1, x_batch_stride=abs_)
        dB = ops._conv_desc(N, CB, H, W, Cout, act=1, x_batch_stride=bbs)
        y = torch.full((N, Cout, H, W), NAN, device="cuda")
        _check(lib.dvc_conv2d_winograd_dual(ctypes.byref(dA), ctypes.byref(dB), _p(av), _p(bv), _p(u), _p(bd), None, _p(y), wsp, wsn,
                                                 ops._stream()), "dvc_conv2d_winograd_dual")
        torch.cuda.synchronize()
        outs.append(y)
    _assert_case(outs[0], outs[1], ref, WINO_TOL, "dual")


@pytest.mark.parametrize("Cin,Cout,H,W", [(32, 64, 9, 70), (64, 64, 13, 37)])
def test_conv2d_ws_input_stride(ops, lib, Cin, Cout, H, W):
    """dvc_conv2d_ws honours x_batch_stride (ragged 32-pixel strips, odd heights)."""
    N = 2
    g, x, w, b, _ = _data(Cin + H, N, Cin, Cout, H, W, 3, H, W, False)
    ref = ref_conv(x, w, b, 3, 1, 1, 1, 0, 1, 1, None, None, None, None, 1, 0.0)
    u, bd = ops.pack_ws_weight(w.cuda()), b.cuda()

    def run(xv, xbs, rv, rbs, y):
        d = ops._conv_desc(N, Cin, H, W, Cout, act=1, x_batch_stride=xbs)
        assert lib.dvc_conv2d_ws_eligible(ctypes.byref(d))
        _check(lib.dvc_conv2d_ws(ctypes.byref(d), _p(xv), _p(u), _p(bd), None, _p(y), ops._stream()), "dvc_conv2d_ws")
    strided, dense = _both(run, x, None, (N, Cout, H, W))
    _assert_case(strided, dense, ref, DIRECT_TOL, ("ws", Cin, Cout, H, W))


# ---- InstanceNorm entries and gray2rgb
@pytest.mark.parametrize("shape", [(2, 5, 27, 45), (2, 8, 26, 48)], ids=["unaligned_scalar", "float4"])
def test_instnorm_entries_with_sliced_input_and_residual(ops, lib, shape):
    """dvc_instnorm_stats, dvc_affine_act and dvc_instnorm_apply (also with scale_out / shift_out, and with the second output y2
    at sub2 = 2) on a sliced x and a sliced residual: planes of 1215 elements (bases off 16 bytes, scalar paths) and of 1248 (the
    float4 paths).  Float64 instance norm at the existing 5e-6; bit-identical to the contiguous call."""
    N, C, H, W = shape
    g = torch.Generator().manual_seed(C)
    x = torch.randn(N, C, H, W, generator=g) * 3 + 1.5
    res = torch.randn(N, C, H, W, generator=g)
    cs2 = (torch.rand(C, generator=g) + 0.5).cuda()
    slope = torch.tensor([0.2], device="cuda")
    norm = F.instance_norm(x.double(), eps=1e-5)
    ref = F.prelu(norm + res.double(), torch.tensor([0.2], dtype=torch.float64))
    ref2 = (norm * cs2.double().cpu().view(1, C, 1, 1))[:, :, ::2, ::2]
    st = ops._stream()
    runs = []
    for place in (_wide, _dense):
        (xv, xbs), (rv, rbs) = place(x), place(res)
        new = lambda *s: torch.full(s, NAN, device="cuda")         # noqa: E731
        sc, sh, ya, yf, yo, y2, so, ho = new(N * C), new(N * C), new(N, C, H, W), new(N, C, H, W), new(N, C, H, W), \
            new(N, C, (H + 1) // 2, (W + 1) // 2), new(N * C), new(N * C)
        _check(lib.dvc_instnorm_stats(_p(xv), N, C, H * W, xbs, 1e-5, None, _p(sc), _p(sh), st), "dvc_instnorm_stats")
        _check(lib.dvc_affine_act(_p(xv), _p(sc), _p(sh), _p(rv), _p(slope), N, C, H, W, 1, 0, xbs, rbs, 0, _p(ya), st), "dvc_affine_act")
        _check(lib.dvc_instnorm_apply(_p(xv), _p(rv), _p(slope), None, 1e-5, N, C, H, W, 1, 1, 0, xbs, rbs, 0, _p(yf), None, None, None,
                                           1, None, st), "dvc_instnorm_apply")
        _check(lib.dvc_instnorm_apply(_p(xv), None, None, None, 1e-5, N, C, H, W, 1, 1, 0, xbs, 0, 0, _p(yo), _p(so), _p(ho), _p(cs2),
                                           2, _p(y2), st), "dvc_instnorm_apply")
        torch.cuda.synchronize()
        runs.append((sc, sh, ya, yf, yo, y2, so, ho))
    for a, b in zip(*runs):
        assert not torch.isnan(a).any() and torch.equal(a, b)
    sc, sh, ya, yf, yo, y2, so, ho = runs[0]
    assert torch.equal(ya, yf) and torch.equal(so, sc) and torch.equal(ho, sh)
    assert (ya.double().cpu() - ref).abs().max().item() < 5e-6
    assert (yo.double().cpu() - norm).abs().max().item() < 5e-6
    assert (y2.double().cpu() - ref2).abs().max().item() < 1e-5         # (the existing tolerance of the scaled, subsampled form)


def test_gray2rgb_on_the_l_plane_of_a_lab_tensor(ops, lib):
    N, H, W = 2, 9, 31
    L = torch.rand(N, 1, H, W, generator=torch.Generator().manual_seed(1)) * 100 - 50
    lab = torch.full((N, 3, H, W), NAN, device="cuda")
    lab[:, 0:1] = L.cuda()
    y = torch.full((N, 3, H, W), NAN, device="cuda")
    _check(lib.dvc_gray2rgb(_p(lab), N, H * W, 3 * H * W, _p(y), ops._stream()), "dvc_gray2rgb")
    assert torch.equal(y.cpu(), ((L + 50.0) / 100.0).expand(N, 3, H, W))
