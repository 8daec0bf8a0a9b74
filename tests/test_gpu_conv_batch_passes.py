"""GPU: convolution launches that cover a batch in SEVERAL passes.

csrc/conv_mfma.hip promises that a batch of N is bit-identical to N single-image calls.  Three host loops stand behind that
promise when one launch cannot take the whole batch: dvc_conv2d / conv2d_images (the split-K workspace holds the partial sums of
fewer images), wino_run (the same, and the 65535-workgroup cap of the kernel's 16-bit reciprocal index decode), and the rule in
dvc_amd.ops that a deferred reduce falls back to the ordinary one when `images_per_launch < N`.  Every pass offsets x, y, the
residual, the pooled output, the second input, the per-image input affine and the per-image filters by `n0 *` its own stride,
and the reduce reads a slab of NB * per_image floats with NB smaller in the last pass.

Every case calls the C ABI directly with a workspace that is a slice of a larger NaN-filled buffer, and asserts
  1. the path: dvc_conv2d_winograd_split reports the expected (split, images_per_launch) with images_per_launch < N.  The direct
     engine has no query, and tests/launch_recorder.py records dvc_amd.ops calls, not kernel launches, so the passes cannot be
     counted; they follow from the sizes: the workspace is k * S * Cout * OH * OW * 4 bytes, the launcher keeps the forced split
     S while one image's S slices fit (conv2d_images: `while (S > 1 && S * Cout * OH * OW * 4 > workspace_bytes) --S`), and then
     covers workspace_bytes / (S * Cout * OH * OW * 4) = k images per pass;
  2. accuracy against the float64 reference at the engine's existing tolerance (direct 2e-5, Winograd 5e-5);
  3. batch identity: every image equals, bit for bit, a single-image call with the full 64 MiB workspace;
  4. containment: the guard floats around the workspace are still NaN, the channels of the wider tensor around a channel-slice
     destination too;
  5. determinism: a second run over a workspace pre-filled with another byte pattern gives the same bits.

Workspace-limited cases: N = 5 at two images per pass (passes of 2, 2 and 1) on 13 x 23 maps, with x, y and the residual each a
channel slice of a wider tensor of its own width (distinct non-default batch strides).  The two-input case reads its first input
through the x2 upsample, so its maps are 14 x 22 (stored 7 x 11).

Each case prints one `conv_batch_passes` line with the figures it asserts on (pytest -s shows them)."""
import ctypes
import time

import pytest
import torch
import torch.nn.functional as F

from cabi_helpers import check as _check, lib, nan_tensor as _nan, ops, ptr as _p  # noqa: F401  (ops, lib: fixtures)
from test_gpu_ops import ref_conv, relerr

pytestmark = pytest.mark.gpu
DIRECT_TOL, WINO_TOL = 2e-5, 5e-5
GUARD = 4096            # NaN floats in front of and behind every workspace
N5, H, W = 5, 13, 23


@pytest.fixture(scope="module", autouse=True)
def _wall_time():
    t0 = time.time()
    yield
    print(f"\nconv_batch_passes file: wall time {time.time() - t0:.1f} s")


def _report(case, err, plan):
    print(f"\nconv_batch_passes {case}: relerr {err:.3e} plan (split, images_per_launch) = {plan}")


class _Guarded:
    """`nbytes` of workspace inside a NaN-filled buffer."""

    def __init__(self, nbytes):
        self.nbytes, self.nfloat = nbytes, (nbytes + 3) // 4
        self.buf = _nan(GUARD + self.nfloat + GUARD)

    @property
    def ptr(self):
        return _p(self.buf[GUARD:])

    def fill(self, byte):
        self.buf[GUARD:GUARD + self.nfloat].view(torch.uint8).fill_(byte)

    def assert_contained(self):
        assert torch.isnan(self.buf[:GUARD]).all() and torch.isnan(self.buf[GUARD + self.nfloat:]).all(), "wrote outside the workspace"


def _full_ws(ops):
    ws = ops._workspace(torch.device("cuda", torch.cuda.current_device()), ops.CONV_WORKSPACE_BYTES, "conv")
    return ctypes.c_void_p(ws.data_ptr()), ws.numel()


def _wide(t, extra):
    """(whole tensor, view, batch stride in elements): `t` [N, C, H, W] as channels [8 : 8 + C] of a NaN-filled
    [N, C + extra, H, W] tensor."""
    if t is None:
        return None, None, 0
    N, C, h, w = t.shape
    big = _nan(N, C + extra, h, w)
    big[:, 8:8 + C] = t.cuda()
    return big, big[:, 8:8 + C], (C + extra) * h * w


def _dest(N, C, h, w, extra):
    big = _nan(N, C + extra, h, w)
    return big, big[:, 8:8 + C], (C + extra) * h * w


def _assert_slice_only(big, C):
    assert torch.isnan(big[:, :8]).all() and torch.isnan(big[:, 8 + C:]).all(), "wrote around the channel slice"
    assert not torch.isnan(big[:, 8:8 + C]).any(), "left part of the destination unwritten"


def _twice(ws, dests, run):
    """run() into the NaN-refilled `dests` (whole wider tensors) over the workspace filled with 0x5A and then 0xFF bytes (NaN as
    floats): the two results agree bit for bit (the untouched NaN around the slices included) and the workspace guards survive."""
    results = []
    for byte in (0x5A, 0xFF):
        ws.fill(byte)
        for t in dests:
            t.fill_(float("nan"))
        run()
        torch.cuda.synchronize()
        ws.assert_contained()
        results.append([t.clone() for t in dests])
    for a, b in zip(*results):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), "the result depends on what the workspace held"
    return results[0]


def _data(seed, N, Cin, Cout, h, w, ks=3, res_hw=None):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(N, Cin, h, w, generator=g)
    wt = torch.randn(Cout, Cin, ks, ks, generator=g) / (Cin * ks * ks) ** 0.5
    b = torch.randn(Cout, generator=g) * 0.1
    r = torch.randn(N, Cout, *res_hw, generator=g) if res_hw else None
    return g, x, wt, b, r


# ---- dvc_conv2d_winograd: workspace-limited
@pytest.mark.parametrize("dil,split_k,k", [(1, 2, 2), (1, 3, 2), (2, 2, 2), (1, 2, 1)],
                         ids=["split2", "split3", "dil2_split2", "one_image_per_pass"])
def test_winograd_workspace_limited(ops, lib, dil, split_k, k):
    """64 -> 64 with residual and ReLU, the workspace holding the partial sums of k of the 5 images: passes of 2, 2, 1 (k = 2) or
    five passes (k = 1)."""
    N, Cin, Cout = N5, 64, 64
    _, x, w, b, res = _data(100 * dil + 10 * split_k + k, N, Cin, Cout, H, W, res_hw=(H, W))
    ref = ref_conv(x, w, b, 3, 1, dil, dil, 0, 1, 1, None, None, None, res, 1, 0.0)
    u, bd = ops.pack_winograd_weight(w.cuda()), b.cuda()
    _, xv, xbs = _wide(x, 16)
    _, rv, rbs = _wide(res, 24)
    ybig, yv, ybs = _dest(N, Cout, H, W, 40)
    assert len({xbs, rbs, ybs, Cin * H * W}) == 4
    ws = _Guarded(k * split_k * Cout * H * W * 4)
    d = ops._conv_desc(N, Cin, H, W, Cout, dil=dil, act=1, split_k=split_k, x_batch_stride=xbs, y_batch_stride=ybs, res_batch_stride=rbs)
    plan = ops._winograd_split(lib, d, ws.nbytes)
    assert plan == (split_k, k) and k < N

    def run():
        _check(lib.dvc_conv2d_winograd(ctypes.byref(d), _p(xv), _p(u), _p(bd), None, _p(rv), _p(yv), ws.ptr, ws.nbytes, ops._stream()),
               "dvc_conv2d_winograd")
    (got,) = _twice(ws, [ybig], run)
    _assert_slice_only(got, Cout)
    y = got[:, 8:8 + Cout]
    err = relerr(y, ref)
    _report(f"winograd dil{dil} split{split_k} k{k}", err, plan)
    assert err < WINO_TOL
    fp, fn = _full_ws(ops)
    d1 = ops._conv_desc(1, Cin, H, W, Cout, dil=dil, act=1, split_k=split_k)
    assert ops._winograd_split(lib, d1, fn) == (split_k, 1)
    xd, resd = x.cuda(), res.cuda()
    for n in range(N):
        one = _nan(1, Cout, H, W)
        _check(lib.dvc_conv2d_winograd(ctypes.byref(d1), _p(xd[n:n + 1]), _p(u), _p(bd), None, _p(resd[n:n + 1]), _p(one), fp, fn,
                                       ops._stream()), "dvc_conv2d_winograd")
        assert torch.equal(y[n:n + 1], one), f"image {n} differs from its single-image call"


# ---- dvc_conv2d_winograd_pool
@pytest.mark.parametrize("want_full", [True, False], ids=["full", "pool_only"])
def test_winograd_pool_workspace_limited(ops, lib, want_full):
    """16 -> 64 split in two, two of five images per pass; `y` (when asked for) and `y_pool` are channel slices with batch strides
    of their own.  Both equal dvc_conv2d_winograd followed by dvc_maxpool2x2 on the single image, bit for bit."""
    N, Cin, Cout, split_k, k = N5, 16, 64, 2, 2
    PH, PW = H // 2, W // 2
    _, x, w, b, _ = _data(31, N, Cin, Cout, H, W)
    ref = ref_conv(x, w, b, 3, 1, 1, 1, 0, 1, 1, None, None, None, None, 1, 0.0)
    ref_pool = F.max_pool2d(ref, 2, 2)
    u, bd = ops.pack_winograd_weight(w.cuda()), b.cuda()
    _, xv, xbs = _wide(x, 16)
    ybig, yv, ybs = _dest(N, Cout, H, W, 24)
    pbig, pv, pbs = _dest(N, Cout, PH, PW, 40)
    assert pbs != Cout * PH * PW and ybs != Cout * H * W
    ws = _Guarded(k * split_k * Cout * H * W * 4)
    d = ops._conv_desc(N, Cin, H, W, Cout, act=1, split_k=split_k, x_batch_stride=xbs, y_batch_stride=ybs)
    plan = ops._winograd_split(lib, d, ws.nbytes)
    assert plan == (split_k, k) and k < N

    def run():
        _check(lib.dvc_conv2d_winograd_pool(ctypes.byref(d), _p(xv), _p(u), _p(bd), None, _p(yv) if want_full else None, _p(pv), pbs,
                                            ws.ptr, ws.nbytes, ops._stream()), "dvc_conv2d_winograd_pool")
    full, pool = _twice(ws, [ybig, pbig], run)
    _assert_slice_only(pool, Cout)
    if want_full:
        _assert_slice_only(full, Cout)
    else:
        assert torch.isnan(full).all()
    y, yp = full[:, 8:8 + Cout], pool[:, 8:8 + Cout]
    err = max(relerr(yp, ref_pool), relerr(y, ref) if want_full else 0.0)
    _report(f"winograd_pool {'full' if want_full else 'pool_only'}", err, plan)
    assert err < WINO_TOL
    fp, fn = _full_ws(ops)
    d1 = ops._conv_desc(1, Cin, H, W, Cout, act=1, split_k=split_k)
    xd = x.cuda()
    for n in range(N):
        one, one_pool = _nan(1, Cout, H, W), _nan(1, Cout, PH, PW)
        _check(lib.dvc_conv2d_winograd(ctypes.byref(d1), _p(xd[n:n + 1]), _p(u), _p(bd), None, None, _p(one), fp, fn, ops._stream()),
               "dvc_conv2d_winograd")
        _check(lib.dvc_maxpool2x2(_p(one), Cout, H, W, _p(one_pool), ops._stream()), "dvc_maxpool2x2")
        assert torch.equal(yp[n:n + 1], one_pool), f"pooled image {n}"
        if want_full:
            assert torch.equal(y[n:n + 1], one), f"image {n}"


# ---- dvc_conv2d_winograd_dual
def test_winograd_dual_workspace_limited(ops, lib):
    """16 (read through the x2 upsample, stored 7 x 11) + 24 -> 64 at 14 x 22, 64 x 32 workgroups with two tile rows (cfg 9) split in
    two — the plan is asked for the summed channel count, as tests/test_gpu_wino_upzero.py asks — two of five images per pass.
    Each input is a slice of a wider tensor of its own, so x2's batch stride differs from x's."""
    N, CA, CB, Cout, cfg, split_k, k = N5, 16, 24, 64, 9, 2, 2
    HA, WA, OH, OW = 7, 11, 14, 22
    g = torch.Generator().manual_seed(17)
    xA, xB = torch.randn(N, CA, HA, WA, generator=g), torch.randn(N, CB, OH, OW, generator=g)
    wA = torch.randn(Cout, CA, 3, 3, generator=g) / (CA * 9) ** 0.5
    wB = torch.randn(Cout, CB, 3, 3, generator=g) / (CB * 9) ** 0.5
    b = torch.randn(Cout, generator=g)
    up = F.interpolate(xA.double(), scale_factor=2, mode="nearest")
    ref = F.relu(F.conv2d(up, wA.double(), b.double(), padding=1) + F.conv2d(xB.double(), wB.double(), None, padding=1))
    u = torch.cat((ops.pack_winograd_weight(wA.cuda()), ops.pack_winograd_weight(wB.cuda())), dim=1).contiguous()
    bd = b.cuda()
    _, av, abs_ = _wide(xA, 16)
    _, bv, bbs = _wide(xB, 24)
    ybig, yv, ybs = _dest(N, Cout, OH, OW, 40)
    assert len({abs_, bbs, CA * HA * WA, CB * OH * OW}) == 4
    ws = _Guarded(k * split_k * Cout * OH * OW * 4)
    plan = ops._winograd_split(lib, ops._conv_desc(N, CA + CB, OH, OW, Cout, act=1, cfg=cfg, split_k=split_k), ws.nbytes)
    assert plan == (split_k, k) and k < N
    dA = ops._conv_desc(N, CA, HA, WA, Cout, in_up=2, act=1, cfg=cfg, split_k=split_k, x_batch_stride=abs_, y_batch_stride=ybs)
    dB = ops._conv_desc(N, CB, OH, OW, Cout, act=1, x_batch_stride=bbs)

    def run():
        _check(lib.dvc_conv2d_winograd_dual(ctypes.byref(dA), ctypes.byref(dB), _p(av), _p(bv), _p(u), _p(bd), None, _p(yv), ws.ptr,
                                            ws.nbytes, ops._stream()), "dvc_conv2d_winograd_dual")
    (got,) = _twice(ws, [ybig], run)
    _assert_slice_only(got, Cout)
    y = got[:, 8:8 + Cout]
    err = relerr(y, ref)
    _report("winograd_dual 16up+24", err, plan)
    assert err < WINO_TOL
    fp, fn = _full_ws(ops)
    d1A = ops._conv_desc(1, CA, HA, WA, Cout, in_up=2, act=1, cfg=cfg, split_k=split_k)
    d1B = ops._conv_desc(1, CB, OH, OW, Cout, act=1)
    xAd, xBd = xA.cuda(), xB.cuda()
    for n in range(N):
        one = _nan(1, Cout, OH, OW)
        _check(lib.dvc_conv2d_winograd_dual(ctypes.byref(d1A), ctypes.byref(d1B), _p(xAd[n:n + 1]), _p(xBd[n:n + 1]), _p(u), _p(bd),
                                            None, _p(one), fp, fn, ops._stream()), "dvc_conv2d_winograd_dual")
        assert torch.equal(y[n:n + 1], one), f"image {n}"


# ---- dvc_conv2d: direct engine, split-K
def test_conv2d_split_k_workspace_limited(ops, lib):
    """96 -> 64, dilation 2, split in two over the twelve 8-channel chunks, the workspace holding two images' partial sums: passes
    of 2, 2, 1.  in_scale / in_shift are [N][Cin] and differ between the images (the `n0 * Cin` offset); residual and channel-slice
    destination as above."""
    N, Cin, Cout, dil, split_k, k = N5, 96, 64, 2, 2, 2
    g, x, w, b, res = _data(41, N, Cin, Cout, H, W, res_hw=(H, W))
    scale, shift = torch.rand(N * Cin, generator=g) + 0.5, torch.randn(N * Cin, generator=g) * 0.3
    ref = ref_conv(x, w, b, 3, 1, dil, dil, 0, 1, 1, scale, shift, None, res, 1, 0.0)
    wp, bd, scd, shd = ops.pack_conv_weight(w.cuda()), b.cuda(), scale.cuda(), shift.cuda()
    _, xv, xbs = _wide(x, 16)
    _, rv, rbs = _wide(res, 24)
    ybig, yv, ybs = _dest(N, Cout, H, W, 40)
    ws = _Guarded(k * split_k * Cout * H * W * 4)
    d = ops._conv_desc(N, Cin, H, W, Cout, dil=dil, act=1, split_k=split_k, x_batch_stride=xbs, y_batch_stride=ybs, res_batch_stride=rbs)

    def run():
        _check(lib.dvc_conv2d(ctypes.byref(d), _p(xv), _p(wp), _p(bd), _p(scd), _p(shd), None, None, _p(rv), _p(yv), ws.ptr, ws.nbytes,
                              ops._stream()), "dvc_conv2d")
    (got,) = _twice(ws, [ybig], run)
    _assert_slice_only(got, Cout)
    # both images' slices of both parts were written: the launch did split in two and did take two images
    assert not torch.isnan(ws.buf[GUARD:GUARD + ws.nfloat]).any()
    y = got[:, 8:8 + Cout]
    err = relerr(y, ref)
    _report("conv2d dil2 split2 affine", err, (split_k, k))
    assert err < DIRECT_TOL
    fp, fn = _full_ws(ops)
    d1 = ops._conv_desc(1, Cin, H, W, Cout, dil=dil, act=1, split_k=split_k)
    xd, resd = x.cuda(), res.cuda()
    for n in range(N):
        one = _nan(1, Cout, H, W)
        _check(lib.dvc_conv2d(ctypes.byref(d1), _p(xd[n:n + 1]), _p(wp), _p(bd), _p(scd[n * Cin:]), _p(shd[n * Cin:]), None, None,
                              _p(resd[n:n + 1]), _p(one), fp, fn, ops._stream()), "dvc_conv2d")
        assert torch.equal(y[n:n + 1], one), f"image {n}"


def test_conv2d_per_image_filters_workspace_limited(ops, lib):
    """The batched-GEMM form (w_batch_stride != 0, ksize 1): B = 5, K = 96, M = 64 on 9 x 11 positions, split in two, the
    workspace holding two images: every pass must move on to ITS images' filters (`n0 * w_batch_stride`)."""
    B, K, M, h, w_, split_k, k = N5, 96, 64, 9, 11, 2, 2
    g = torch.Generator().manual_seed(43)
    x = torch.randn(B, K, h, w_, generator=g)
    w = torch.randn(B, K, 1, M, generator=g) * 0.1
    ref = torch.bmm(w.view(B, K, M).double().transpose(1, 2), x.view(B, K, h * w_).double()).view(B, M, h, w_)
    wd = w.cuda()
    _, xv, xbs = _wide(x, 16)
    ybig, yv, ybs = _dest(B, M, h, w_, 40)
    ws = _Guarded(k * split_k * M * h * w_ * 4)
    d = ops._conv_desc(B, K, h, w_, M, ksize=1, pad=0, split_k=split_k, x_batch_stride=xbs, y_batch_stride=ybs, w_batch_stride=K * M)

    def run():
        _check(lib.dvc_conv2d(ctypes.byref(d), _p(xv), _p(wd), None, None, None, None, None, None, _p(yv), ws.ptr, ws.nbytes, ops._stream()),
               "dvc_conv2d")
    (got,) = _twice(ws, [ybig], run)
    _assert_slice_only(got, M)
    assert not torch.isnan(ws.buf[GUARD:GUARD + ws.nfloat]).any()
    y = got[:, 8:8 + M]
    err = relerr(y, ref)
    _report("conv2d per-image filters split2", err, (split_k, k))
    assert err < DIRECT_TOL
    fp, fn = _full_ws(ops)
    d1 = ops._conv_desc(1, K, h, w_, M, ksize=1, pad=0, split_k=split_k)
    xd = x.cuda()
    for n in range(B):
        one = _nan(1, M, h, w_)
        _check(lib.dvc_conv2d(ctypes.byref(d1), _p(xd[n:n + 1]), _p(wd[n]), None, None, None, None, None, None, _p(one), fp, fn,
                              ops._stream()), "dvc_conv2d")
        assert torch.equal(y[n:n + 1], one), f"image {n}"


def test_conv2d_workspace_smaller_than_one_image(ops, lib):
    """A workspace one float short of ONE image's split-2 partial sums: the launcher lowers the split (here to none) instead of
    failing or overrunning, in one pass.  The plan depends on the workspace size, so the single-image calls get the same
    short workspace (with the full one they would split in two and sum in another order)."""
    N, Cin, Cout, dil, split_k = N5, 96, 64, 2, 2
    _, x, w, b, res = _data(47, N, Cin, Cout, H, W, res_hw=(H, W))
    ref = ref_conv(x, w, b, 3, 1, dil, dil, 0, 1, 1, None, None, None, res, 1, 0.0)
    wp, bd = ops.pack_conv_weight(w.cuda()), b.cuda()
    _, xv, xbs = _wide(x, 16)
    _, rv, rbs = _wide(res, 24)
    ybig, yv, ybs = _dest(N, Cout, H, W, 40)
    ws = _Guarded(split_k * Cout * H * W * 4 - 4)
    d = ops._conv_desc(N, Cin, H, W, Cout, dil=dil, act=1, split_k=split_k, x_batch_stride=xbs, y_batch_stride=ybs, res_batch_stride=rbs)

    def run():
        _check(lib.dvc_conv2d(ctypes.byref(d), _p(xv), _p(wp), _p(bd), None, None, None, None, _p(rv), _p(yv), ws.ptr, ws.nbytes,
                              ops._stream()), "dvc_conv2d")
    (got,) = _twice(ws, [ybig], run)
    _assert_slice_only(got, Cout)
    y = got[:, 8:8 + Cout]
    err = relerr(y, ref)
    _report("conv2d workspace short of one image", err, ("< 2", N))
    assert err < DIRECT_TOL
    d1 = ops._conv_desc(1, Cin, H, W, Cout, dil=dil, act=1, split_k=split_k)
    xd, resd = x.cuda(), res.cuda()
    for n in range(N):
        one = _nan(1, Cout, H, W)
        _check(lib.dvc_conv2d(ctypes.byref(d1), _p(xd[n:n + 1]), _p(wp), _p(bd), None, None, None, None, _p(resd[n:n + 1]), _p(one),
                              ws.ptr, ws.nbytes, ops._stream()), "dvc_conv2d")
        assert torch.equal(y[n:n + 1], one), f"image {n}"
    torch.cuda.synchronize()
    ws.assert_contained()


# ---- the 65535-workgroup cap
#   cfg, split_k, Cin, H, W, dil, workgroups per image (gx * gy * split), N
CAP = [
    (12, 1, 8, 2, 2, 1, 2, 32770),       # 32 x 32 workgroups: gx 1, gy 2
    (8, 2, 16, 2, 2, 1, 2, 32770),       # 64 x 32 workgroups split in two: gx 1, gy 1; the 64 MiB workspace alone would allow 32768
    (8, 1, 8, 4, 4, 2, 4, 16386),        # dilation 2: four parity classes, gx 4, gy 1
]


@pytest.mark.parametrize("cfg,split_k,Cin,h,w_,dil,per_image,N", CAP, ids=["cfg12", "cfg8_split2", "cfg8_dil2"])
def test_winograd_workgroup_cap(ops, lib, cfg, split_k, Cin, h, w_, dil, per_image, N):
    """Tiny images, so many that the 1-D grid would pass 65535 workgroups: images_per_launch = 65535 // per_image, and a second
    pass of 3 images.  The first pass puts every logical workgroup index 0 .. 65535 - 65535 % per_image - 1 through the
    reciprocal decode and the XCD-aware remap, with a grid that is no multiple of 8.  The float64 reference covers the whole
    batch; bit identity is checked against separate three-image calls at the start, across the seam and at the end."""
    Cout = 64
    _, x, w, b, _ = _data(cfg * 10 + dil, N, Cin, Cout, h, w_)
    ref = ref_conv(x, w, b, 3, 1, dil, dil, 0, 1, 1, None, None, None, None, 1, 0.0)
    u, bd, xd = ops.pack_winograd_weight(w.cuda()), b.cuda(), x.cuda()
    ybig, yv, ybs = _dest(N, Cout, h, w_, 16)
    ws = _Guarded(ops.CONV_WORKSPACE_BYTES if split_k > 1 else 4096)
    d = ops._conv_desc(N, Cin, h, w_, Cout, dil=dil, act=1, cfg=cfg, split_k=split_k, y_batch_stride=ybs)
    plan = ops._winograd_split(lib, d, ws.nbytes)
    ipl = 65535 // per_image
    assert plan == (split_k, ipl) and N - ipl == 3 and (ipl * per_image) % 8 != 0
    if split_k > 1:
        assert ws.nbytes // (split_k * Cout * h * w_ * 4) > ipl          # the cap binds, not the workspace

    def run():
        _check(lib.dvc_conv2d_winograd(ctypes.byref(d), _p(xd), _p(u), _p(bd), None, None, _p(yv), ws.ptr, ws.nbytes, ops._stream()),
               "dvc_conv2d_winograd")
    (got,) = _twice(ws, [ybig], run)
    _assert_slice_only(got, Cout)
    y = got[:, 8:8 + Cout]
    err = relerr(y, ref)
    _report(f"winograd cap cfg{cfg} split{split_k} dil{dil} N{N}", err, plan)
    assert err < WINO_TOL
    d3 = ops._conv_desc(3, Cin, h, w_, Cout, dil=dil, act=1, cfg=cfg, split_k=split_k)
    assert ops._winograd_split(lib, d3, ws.nbytes) == (split_k, 3)
    for a in (0, ipl - 1, N - 3):
        three = _nan(3, Cout, h, w_)
        _check(lib.dvc_conv2d_winograd(ctypes.byref(d3), _p(xd[a:a + 3]), _p(u), _p(bd), None, None, _p(three), ws.ptr, ws.nbytes,
                                       ops._stream()), "dvc_conv2d_winograd")
        assert torch.equal(y[a:a + 3], three), f"images {a}..{a + 2}"


# ---- dvc_amd.ops: a deferred reduce needs the whole batch in one launch
def test_ops_deferred_reduce_falls_back_when_the_workspace_is_short(ops, lib, monkeypatch):
    """ops.conv2d_winograd(defer_reduce=True) with a workspace that holds two of the five images' partial sums: an ordinary
    tensor (the library reduces pass by pass), equal to the non-deferred call bit for bit."""
    N, Cin, Cout, split_k = N5, 64, 64, 3
    _, x, w, b, _ = _data(51, N, Cin, Cout, H, W)
    xd, u, bd = x.cuda(), ops.pack_winograd_weight(w.cuda()), b.cuda()
    small = 2 * split_k * Cout * H * W * 4
    monkeypatch.setattr(ops, "CONV_WORKSPACE_BYTES", small)
    with ops.workspace_scope({}):
        assert ops._winograd_split(lib, ops._conv_desc(N, Cin, H, W, Cout, act=1, split_k=split_k), small) == (split_k, 2)
        got = ops.conv2d_winograd(xd, u, bd, act=1, split_k=split_k, defer_reduce=True)
        assert isinstance(got, torch.Tensor) and not isinstance(got, ops.ConvPartials)
        want = ops.conv2d_winograd(xd, u, bd, act=1, split_k=split_k)
        torch.cuda.synchronize()
    assert torch.equal(got, want)
    err = relerr(got, ref_conv(x, w, b, 3, 1, 1, 1, 0, 1, 1, None, None, None, None, 1, 0.0))
    _report("ops deferred reduce, short workspace", err, (split_k, 2))
    assert err < WINO_TOL


def test_ops_deferred_reduce_falls_back_at_the_workgroup_cap(ops, lib):
    """... and when the workspace holds the whole batch (here exactly: 8 x 8192 x 64 x 2 x 2 floats are the 64 MiB) but the
    65535-workgroup cap splits it: 8192 images at eight workgroups each (64 -> 64 split in eight) are 65536, one too many."""
    N, Cin, Cout, h, w_, split_k = 8192, 64, 64, 2, 2, 8
    _, x, w, b, _ = _data(53, N, Cin, Cout, h, w_)
    xd, u, bd = x.cuda(), ops.pack_winograd_weight(w.cuda()), b.cuda()
    with ops.workspace_scope({}):
        plan = ops._winograd_split(lib, ops._conv_desc(N, Cin, h, w_, Cout, act=1, split_k=split_k), ops.CONV_WORKSPACE_BYTES)
        assert plan == (split_k, 65535 // 8) and split_k * N * Cout * h * w_ * 4 == ops.CONV_WORKSPACE_BYTES
        got = ops.conv2d_winograd(xd, u, bd, act=1, split_k=split_k, defer_reduce=True)
        assert isinstance(got, torch.Tensor) and not isinstance(got, ops.ConvPartials)
        want = ops.conv2d_winograd(xd, u, bd, act=1, split_k=split_k)
        torch.cuda.synchronize()
    assert torch.equal(got, want)
    err = relerr(got, ref_conv(x, w, b, 3, 1, 1, 1, 0, 1, 1, None, None, None, None, 1, 0.0))
    _report("ops deferred reduce, workgroup cap", err, plan)
    assert err < WINO_TOL


def test_ops_group_falls_back_to_per_layer_results(ops, lib, monkeypatch):
    """ops.conv3x3_group with two layers the library splits, each asking for a deferred reduce, and a workspace that holds the
    partial sums of fewer images than either batch: per-layer launches with the ordinary reduce, each result the tensor its own
    conv3x3 call returns.  13 x 25: the smallest odd map the engine rule (ops._wino_rule) still sends to the Winograd engine."""
    N, H, W = N5, 13, 25
    shapes = [(64, 64), (128, 64)]
    data = [_data(61 + i, N, ci, co, H, W) for i, (ci, co) in enumerate(shapes)]
    dev = [(x.cuda(), ops.pack_winograd_weight(w.cuda()), w.cuda(), b.cuda()) for _, x, w, b, _ in data]
    splits = [ops._winograd_split(lib, ops._conv_desc(N, ci, H, W, co, act=1), ops.CONV_WORKSPACE_BYTES)[0] for ci, co in shapes]
    assert all(s > 1 for s in splits)
    small = 2 * max(s * co * H * W * 4 for s, (_, co) in zip(splits, shapes))
    monkeypatch.setattr(ops, "CONV_WORKSPACE_BYTES", small)
    plans = [ops._winograd_split(lib, ops._conv_desc(N, ci, H, W, co, act=1), small) for ci, co in shapes]
    assert all(s == s0 and ipl < N for (s, ipl), s0 in zip(plans, splits)), plans
    assert ops.group_heads() and ops.fuse_reduce() and ops.conv_algo() == "auto"
    items = [dict(x=x, weight=w, packs=(lambda kind, u=u: u), bias=b, act=1, defer_reduce=True) for x, u, w, b in dev]
    with ops.workspace_scope({}):
        assert all(ops._item_is_winograd(it) for it in items)
        got = ops.conv3x3_group(items)
        want = [ops.conv3x3(x, w, (lambda kind, u=u: u), b, act=1) for x, u, w, b in dev]
        torch.cuda.synchronize()
    for g_, w_, (_, x, w, b, _), plan in zip(got, want, data, plans):
        assert isinstance(g_, torch.Tensor) and not isinstance(g_, ops.ConvPartials)
        assert torch.equal(g_, w_)
        err = relerr(g_, ref_conv(x, w, b, 3, 1, 1, 1, 0, 1, 1, None, None, None, None, 1, 0.0))
        _report(f"ops conv3x3_group {x.shape[1]} -> {w.shape[0]}", err, plan)
        assert err < WINO_TOL
