"""GPU: the small glue kernels (csrc/norm_pool.hip, dvc_conv1x1_small) at the shapes where they can go wrong — sizes of one,
sizes the window or the vector width does not divide, every code path's threshold — against float64 references on the CPU.
Every tolerance is a formula of the inputs or the one the op already has in tests/test_gpu_ops.py."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import instnorm_bound as IB
from cabi_helpers import ops  # noqa: F401  (fixture)
from test_gpu_ops import report

pytestmark = pytest.mark.gpu


def _gen(*key):
    return torch.Generator().manual_seed(sum((i + 1) * 7919 * int(k) for i, k in enumerate(key)) % (2 ** 31))


# ---- dvc_conv1x1_small
@pytest.mark.parametrize("Cout", [1, 2, 3, 4])
@pytest.mark.parametrize("Cin", [1, 5, 128, 130])
def test_conv1x1_small_edges(ops, Cout, Cin):
    """Every Cout instantiation, channel counts below / not a multiple of the four channel groups, planes of one pixel, less
    than one and several 64-pixel workgroups, batches, with and without bias (the entry takes NULL), with and without tanh*128.
    Per element: |err| <= 2e-6 * (sum |w x| + |b|) without activation (fp32 accumulation over at most 130 terms), and
    128 * that + 128 * 2^-22 behind tanh*128 (|tanh'| <= 1; fp32 tanh within 2^-22 of a value in [-1, 1])."""
    for HW in (1, 7, 391, 1024):
        for N in (1, 3):
            g = _gen(Cout, Cin, HW, N)
            x = torch.randn(N, Cin, HW, 1, generator=g)
            w = torch.randn(Cout, Cin, generator=g) * 0.2
            b = torch.randn(Cout, generator=g)
            for bias in (b, None):
                pre = torch.einsum("oc,nchw->nohw", w.double(), x.double())
                mag = torch.einsum("oc,nchw->nohw", w.double().abs(), x.double().abs())
                if bias is not None:
                    pre = pre + bias.double().view(1, Cout, 1, 1)
                    mag = mag + bias.double().abs().view(1, Cout, 1, 1)
                lin = 2e-6 * mag
                for act in (ops.ACT_NONE, ops.ACT_TANH128):
                    ref = torch.tanh(pre) * 128 if act == ops.ACT_TANH128 else pre
                    tol = 128 * lin + 128 * 2.0 ** -22 if act == ops.ACT_TANH128 else lin
                    y = ops.conv1x1_small(x.cuda(), w.cuda(), None if bias is None else bias.cuda(), act=act)
                    assert tuple(y.shape) == (N, Cout, HW, 1)
                    ratio = ((y.double().cpu() - ref).abs() / tol.clamp_min(1e-300)).max().item()
                    assert ratio <= 1.0, (Cout, Cin, HW, N, bias is not None, act, ratio)


# ---- pools
@pytest.mark.parametrize("planes", [1, 7])
@pytest.mark.parametrize("H,W", [(2, 2), (3, 3), (2, 3), (27, 49)])
def test_maxpool_edges(ops, planes, H, W):
    x = torch.randn(1, planes, H, W, generator=_gen(planes, H, W))
    assert torch.equal(ops.maxpool2x2(x.cuda()).cpu(), F.max_pool2d(x, 2, 2))


@pytest.mark.parametrize("planes", [1, 7])
def test_maxpool_scalar_kernel_on_a_4_byte_aligned_view(ops, planes):
    """Even W, but the base sits on 4 bytes only: the float2 kernel must not be taken (its loads would be misaligned)."""
    H, W = 26, 48
    x = torch.randn(1, planes, H, W, generator=_gen(planes, 5))
    flat = torch.zeros(1 + x.numel(), device="cuda")
    view = flat[1:].view(1, planes, H, W)
    view.copy_(x)
    assert view.data_ptr() % 8 == 4 and view.is_contiguous()
    assert torch.equal(ops.maxpool2x2(view).cpu(), F.max_pool2d(x, 2, 2))


@pytest.mark.parametrize("k,H,W", [(2, 27, 49), (2, 2, 2), (4, 7, 9), (4, 43, 66)])
def test_avgpool_edges(ops, k, H, W):
    """Floor mode at sizes the window does not divide (trailing rows / columns ignored) and at exactly one window.
    (a) Inputs on a 2^-6 grid, |x| <= 8: every partial sum of up to 16 such values and the mean are float32 numbers, so any
        correct summation order is exact — the result must be within 1 ulp of the float64 mean per element (the kernel's fp32
        window sum is tied bit for bit to ATen's, tests/test_tail.py, and on arbitrary data neither is within 1 ulp of the
        float64 mean where a window's terms cancel: that case is (b)).
    (b) Standard normal inputs: the running fp32 sum of n = k * k terms is within (n - 1) * 2^-24 * sum |x_i| of the exact
        sum (one rounding per addition, each at most half an ulp of a partial sum <= sum |x_i|); the scaling by 1 / n is exact."""
    fn = ops.avgpool2x2 if k == 2 else ops.avgpool4x4
    g = _gen(k, H, W)
    n = k * k
    xg = torch.randint(-512, 513, (2, 3, H, W), generator=g).float() / 64
    got = fn(xg.cuda()).cpu()
    ref = F.avg_pool2d(xg.double(), k)
    assert tuple(got.shape) == (2, 3, H // k, W // k)
    ulp = torch.from_numpy(np.spacing(ref.abs().float().numpy())).double()
    assert ((got.double() - ref).abs() <= ulp).all()
    xr = torch.randn(2, 3, H, W, generator=g)
    got = fn(xr.cuda()).cpu()
    ref = F.avg_pool2d(xr.double(), k)
    tol = (n - 1) * 2.0 ** -24 * F.avg_pool2d(xr.double().abs(), k)
    assert ((got.double() - ref).abs() <= tol).all()


@pytest.mark.parametrize("f", [1, 2, 3, 4])
@pytest.mark.parametrize("H,W", [(1, 1), (5, 7)])
def test_upsample_nearest_edges(ops, f, H, W):
    x = torch.randn(2, 3, H, W, generator=_gen(f, H, W))
    ref = x.repeat_interleave(f, 2).repeat_interleave(f, 3)
    assert torch.equal(ref, F.interpolate(x, scale_factor=f, mode="nearest"))
    assert torch.equal(ops.upsample_nearest(x.cuda(), f).cpu(), ref)


# ---- channel L2 norm
L2_C = [1, 3, 33, 100, 130, 224]        # below / across the 4 (scalar) and 32 (float4) channel groups; 130, 224: the unrolled loop


def _l2_input(C, H, W):
    x = torch.randn(2, C, H, W, generator=_gen(C, H, W)) * 3
    x[0, :, 0, 0] = 0.0                 # a pixel whose channels are all zero: 0 / (0 + eps) = 0
    x[1] *= 1e-12                       # a map of tiny values: the squares (1e-24) are still normal fp32 numbers
    return x


@pytest.mark.parametrize("C", L2_C)
@pytest.mark.parametrize("H,W", [(1, 1), (9, 14), (2, 2), (6, 6), (40, 50)])       # H*W = 1, 126: scalar kernel; 4, 36, 2000: float4
def test_channel_l2norm_edges(ops, C, H, W):
    from oracle import dvc_oracle as O
    x = _l2_input(C, H, W)
    y = ops.channel_l2norm(x.cuda()).cpu()
    assert not torch.isnan(y).any()
    assert (y[0, :, 0, 0] == 0).all()
    assert (y.double() - O.feature_normalize(x.double())).abs().max().item() < 2e-7


def test_channel_l2norm_multi_takes_eight_maps_and_rejects_nine(ops):
    from dvc_amd import _lib
    from oracle import dvc_oracle as O
    shapes = [(c, h, w) for c, (h, w) in zip(L2_C + [64, 512], [(2, 2), (6, 6), (40, 50), (2, 2), (6, 6), (40, 50), (1, 4), (3, 8)])]
    xs = [_l2_input(c, h, w).cuda() for c, h, w in shapes]
    assert len(xs) == 8
    ys = ops.channel_l2norm_multi(xs)
    for x, y in zip(xs, ys):
        assert (y.double().cpu() - O.feature_normalize(x.double().cpu())).abs().max().item() < 2e-7
        assert torch.equal(y, ops.channel_l2norm(x))
    # nine maps: one more than DVC_L2NORM_MAX_TENSORS — refused by the entry itself (the Python wrapper would split the list)
    lib = _lib.load()
    xs9 = xs + [xs[0]]
    ys9 = [torch.empty_like(x) for x in xs9]
    px = (ctypes.c_void_p * 9)(*[x.data_ptr() for x in xs9])
    py = (ctypes.c_void_p * 9)(*[y.data_ptr() for y in ys9])
    cs = (ctypes.c_int32 * 9)(*[x.shape[1] for x in xs9])
    hw = (ctypes.c_int32 * 9)(*[x.shape[2] * x.shape[3] for x in xs9])
    rc = lib.dvc_channel_l2norm_multi(ctypes.cast(px, ctypes.c_void_p), ctypes.cast(py, ctypes.c_void_p), ctypes.cast(cs, ctypes.c_void_p),
                                      ctypes.cast(hw, ctypes.c_void_p), 9, 2, ops.EPS64, ops._stream())
    assert rc != 0 and b"dvc_channel_l2norm_multi" in lib.dvc_last_error()


# ---- dvc_cx_prepare: the same normalise with 16 channel groups, an optional mean and the norms
# C = 8, 3: fewer channels than groups (empty groups); 66: uneven groups and the tail of the four-in-flight loop; 130: one full
# round of it.  P = 1, 63, 100: below one 64-position tile, ragged across two.  Unit-scale inputs, |out| <= 1: the tolerance of
# the channel_l2norm cases above (the centring adds one rounding of the mean and one of the subtraction per value).
@pytest.mark.parametrize("centre", ["own", "given", "none"])
@pytest.mark.parametrize("C,P", [(8, 100), (3, 1), (66, 63), (130, 100)])
def test_cx_prepare_edges(ops, C, P, centre):
    from cabi_helpers import check, nan_tensor, ptr
    from dvc_amd import _lib
    from oracle import contextual_oracle as CO
    lib = _lib.load()
    B = 2
    x = torch.randn(B, C, P, generator=_gen(C, P))
    x[0, :, 0] = 0.0                    # a position whose channels are all zero
    given = torch.randn(B * C, generator=_gen(P, C)) * 0.1
    xd = x.cuda()
    out, mean, norm = nan_tensor(B, C, P), nan_tensor(B * C), nan_tensor(B, P)
    if centre == "own":
        rc = lib.dvc_cx_prepare(ptr(xd), None, 1, B, C, P, ops.EPS64, ptr(mean), None, ptr(out), ops._stream())
        mu = x.double().mean(-1)
        assert (mean.cpu().double() - mu.flatten()).abs().max().item() < 2e-7
    elif centre == "given":
        rc = lib.dvc_cx_prepare(ptr(xd), ptr(given.cuda()), 1, B, C, P, ops.EPS64, None, ptr(norm), ptr(out), ops._stream())
        mu = given.double().view(B, C)
    else:
        rc = lib.dvc_cx_prepare(ptr(xd), None, 0, B, C, P, ops.EPS64, None, ptr(norm), ptr(out), ops._stream())
        mu = torch.zeros(B, C, dtype=torch.float64)
    check(rc, "dvc_cx_prepare")
    xc = x.double() - mu.unsqueeze(-1)
    assert not torch.isnan(out).any()
    assert (out.cpu().double() - CO.feature_normalize(xc)).abs().max().item() < 2e-7
    if centre == "none":
        assert (out[0, :, 0] == 0).all()
    if centre != "own":
        # the norm: every square carries the subtraction's rounding twice, the sum at most ceil(C / 16) + 16 roundings (fmaf
        # chain per group, then the groups), the root halves the relative error and adds one rounding of its own
        n64 = xc.norm(dim=1)
        rel = ((C + 15) // 16 + 16 + 2) / 2 * 2.0 ** -24 + 2.0 ** -24
        err = (norm.cpu().double() - n64).abs()
        print(f"norm: max relative error {(err / n64.clamp_min(1e-30)).max().item():.3e}, bound {rel:.3e}")
        assert (err <= rel * n64).all()


# ---- dvc_affine_act / dvc_instnorm_apply index maps
def _rows_replicated(r, rpad):
    if rpad == 0:
        return r
    return torch.cat((r[:, :, :1].expand(-1, -1, rpad, -1), r, r[:, :, -1:].expand(-1, -1, rpad, -1)), 2)


def _inorm64(x, eps=1e-5):
    """InstanceNorm2d (biased variance, no affine) in float64; unlike F.instance_norm it takes planes of one element."""
    x = x.double()
    mean = x.mean((2, 3), keepdim=True)
    return (x - mean) / ((x - mean).pow(2).mean((2, 3), keepdim=True) + eps).sqrt()


def _norm_input(N, C, H, W, *key):
    return torch.randn(N, C, H, W, generator=_gen(N, C, H, W, *key)) * 3 + 1.5


@pytest.mark.parametrize("up", [3, 4])
@pytest.mark.parametrize("rpad", [0, 2, 3])
@pytest.mark.parametrize("H,W", [(5, 7), (1, 1)])
def test_affine_act_and_instnorm_apply_up_rpad(ops, up, rpad, H, W):
    """`up` 3 and 4 with `rpad` 0, 2 and 3 (the contract: up <= 4, any rpad), down to a 1 x 1 plane; scale / shift NULL for
    dvc_affine_act.  Float64 references at the ops' existing 5e-6.  A 1 x 1 plane is a constant plane: InstanceNorm of it is
    exactly 0 and the kernels' x * sc + sh leaves the rounding of sh, |x| * rstd * 2^-24 with rstd = eps^-1/2 = 316 — it is
    held to the constant-plane rule, finite and |y| <= 1e-3."""
    N, C = 2, 3
    x = _norm_input(N, C, H, W, up, rpad)
    slope = torch.tensor([0.2])
    sc, sh = torch.rand(N * C, generator=_gen(up, rpad)) + 0.5, torch.randn(N * C, generator=_gen(rpad, up))

    def expand(r):
        return _rows_replicated(r.repeat_interleave(up, 2).repeat_interleave(up, 3), rpad)

    # dvc_affine_act with a given affine, and with none
    y = ops.affine_act(x.cuda(), sc.cuda(), sh.cuda(), slope_t=slope.cuda(), up=up, rpad=rpad).cpu()
    ref = expand(F.prelu(x.double() * sc.double().view(N, C, 1, 1) + sh.double().view(N, C, 1, 1), slope.double()))
    assert tuple(y.shape) == (N, C, H * up + 2 * rpad, W * up)
    assert (y.double() - ref).abs().max().item() < 5e-6
    y = ops.affine_act(x.cuda(), None, None, up=up, rpad=rpad).cpu()
    assert torch.equal(y, expand(x))
    # dvc_instnorm_apply, and the two-kernel path (bit-identical)
    y = ops.instnorm_apply(x.cuda(), slope_t=slope.cuda(), up=up, rpad=rpad)
    s2, h2 = ops.instnorm_stats(x.cuda(), 1e-5)
    assert torch.equal(y, ops.affine_act(x.cuda(), s2, h2, slope_t=slope.cuda(), up=up, rpad=rpad))
    y = y.cpu()
    assert tuple(y.shape) == (N, C, H * up + 2 * rpad, W * up)
    if H * W == 1:
        assert torch.isfinite(y).all() and y.abs().max().item() <= 1e-3
    else:
        ref = expand(F.prelu(_inorm64(x), slope.double()))
        assert (y.double() - ref).abs().max().item() < 5e-6


@pytest.mark.parametrize("H,W", [(1, 1), (1, 5), (27, 45)])
def test_instnorm_apply_sub2_odd_sizes(ops, H, W):
    """`sub` = 2 and the second output at `sub2` = 2 on odd sizes down to one element: [ceil(H/2)][ceil(W/2)], rows and columns
    0, 2, 4, ... (the 1 x 1 plane: see test_affine_act_and_instnorm_apply_up_rpad)."""
    N, C = 2, 5
    x = _norm_input(N, C, H, W)
    cs = torch.rand(C, generator=_gen(H, W)) + 0.5
    ref = _inorm64(x)
    refs = (ref * cs.double().view(1, C, 1, 1))[:, :, ::2, ::2]
    y = ops.instnorm_apply(x.cuda(), chan_scale=cs.cuda(), sub=2).cpu()
    ya, yb = ops.instnorm_apply(x.cuda(), second=(cs.cuda(), 2))
    ya, yb = ya.cpu(), yb.cpu()
    assert tuple(y.shape) == tuple(yb.shape) == (N, C, (H + 1) // 2, (W + 1) // 2) and tuple(ya.shape) == (N, C, H, W)
    assert torch.equal(y, yb)
    if H * W == 1:
        for t in (y, ya):
            assert torch.isfinite(t).all() and t.abs().max().item() <= 1e-3
        return
    assert (y.double() - refs).abs().max().item() < 1e-5          # (the existing tolerance of the scaled, subsampled form)
    assert (ya.double() - ref).abs().max().item() < 5e-6


# ---- InstanceNorm statistics at awkward planes
def _both_paths(ops, x):
    """InstanceNorm(x) through dvc_instnorm_apply and through dvc_instnorm_stats -> dvc_affine_act: bit-identical."""
    y = ops.instnorm_apply(x)
    sc, sh = ops.instnorm_stats(x, 1e-5)
    assert torch.equal(y, ops.affine_act(x, sc, sh))
    return y.cpu()


@pytest.mark.parametrize("H,W", [(26, 48), (1, 1)])
def test_instnorm_constant_plane(ops, H, W):
    """Variance 0 (clamped at 0 before the eps): rstd = eps^-1/2, the output is finite and 0 up to the rounding of sh."""
    x = torch.full((2, 3, H, W), 3.7)
    x[1] = -0.0421
    y = _both_paths(ops, x.cuda())
    assert torch.isfinite(y).all() and y.abs().max().item() <= 1e-3


def test_instnorm_plane_one_past_the_unrolled_loop(ops):
    """12289 elements: 12288 = 3 * 1024 * 4 float4 pieces is where the four-in-flight loop of plane_stats starts to run, the one
    element more goes through the scalar tail; 512 threads per plane (two virtual threads each)."""
    x = _norm_input(1, 3, 1, 12289)
    y = _both_paths(ops, x.cuda())
    assert (y.double() - _inorm64(x)).abs().max().item() < 5e-6


@pytest.mark.parametrize("R", IB.RATIOS)
def test_instnorm_error_grows_with_mean_over_sigma(ops, R):
    """Planes of sigma 1 and mean R.  The kernels apply y = fma(x, sc, sh) with sh = -mean * sc rounded to float32, so their
    error grows with |mean| / sigma where ATen's (x - mean) * rstd does not: bound 2^-23 * (max|x| * rstd + max|y| + 1) per
    plane (tests/instnorm_bound.py; a numpy emulation of the form meets it on these inputs, tests/test_cabi_and_host.py).
    The measured error and the bound of every R go to the test report; DESIGN.md keeps the table."""
    xn = IB.sweep_plane(R)
    x = torch.from_numpy(xn).view(1, 1, *IB.SHAPE)
    y = _both_paths(ops, x.cuda())
    ref, _, _ = IB.reference(xn)
    err = np.abs(y.numpy().astype(np.float64).reshape(IB.SHAPE) - ref).max()
    emu = np.abs(IB.emulate_fma(xn).astype(np.float64) - ref).max()
    bound = IB.bound(xn)
    report(f"instnorm mean/sigma R={R}: max err {err:.2e}, bound {bound:.2e}, numpy fma emulation {emu:.2e}")
    assert err <= bound, (R, err, bound)
