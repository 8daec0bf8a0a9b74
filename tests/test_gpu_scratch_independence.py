"""GPU: a launch must not depend on what its scratch and its outputs held before.

ops._workspace hands out a cached torch.empty buffer that is reused from launch to launch; a slot that is read without being
written, or a counter that is not reset on some path, passes on a fresh zero page and fails in the clip loop, where the same
bytes hold the previous layer's data.  Every entry below runs twice — workspace filled with 0x00 bytes, then with 0xFF bytes (a
NaN as float, -1 as int) — into outputs pre-filled with NaN (integer outputs: -1).  The two results must be bit-identical and
free of NaN, and the result is compared once with the entry's float64 reference at its existing tolerance.

Entries that go through dvc_amd.ops have their cached buffer fetched with the same ops._workspace(device, nbytes, tag) call;
where the wrapper allocates scratch or outputs internally the C entry is called with buffers the test owns."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from cabi_helpers import check as _check, lib, nan_tensor as _nan, ops, ptr as _p  # noqa: F401  (ops, lib: fixtures)
from test_gpu_ops import _corr_truth, _tie_case, _y_bound, ref_conv, relerr

pytestmark = pytest.mark.gpu


def _dev():
    return torch.device("cuda", torch.cuda.current_device())


def _conv_ws(ops):
    return ops._workspace(_dev(), ops.CONV_WORKSPACE_BYTES, "conv")


def _twice(workspaces, run):
    """run() -> tuple of output tensors, once per fill pattern of `workspaces`; asserts the two runs agree bit for bit and hold
    no NaN, returns the first run's outputs."""
    results = []
    for byte in (0x00, 0xFF):
        for ws in workspaces:
            ws.view(torch.uint8).fill_(byte)
        outs = run()
        torch.cuda.synchronize()
        results.append(tuple(o.clone() for o in outs))
    for a, b in zip(*results):
        assert torch.equal(a, b), "the result depends on what the workspace held"
        if a.is_floating_point():
            assert not torch.isnan(a).any()
    return results[0]


def _conv_data(seed, N, Cin, Cout, H, W):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(N, Cin, H, W, generator=g)
    w = torch.randn(Cout, Cin, 3, 3, generator=g) / (Cin * 9) ** 0.5
    b = torch.randn(Cout, generator=g) * 0.1
    return x, w, b


# ---- convolutions
@pytest.mark.parametrize("cfg,split_k,Cin,Cout,H,W", [(-1, 2, 96, 64, 13, 24), (-1, 8, 96, 64, 13, 24),
                                                     (34, 0, 64, 128, 21, 40), (36, 0, 64, 128, 21, 40)],
                         ids=["split_k2", "split_k8", "stream_k34", "stream_k36"])
def test_conv2d_split_k_and_stream_k(ops, cfg, split_k, Cin, Cout, H, W):
    N = 2
    x, w, b = _conv_data(Cin + cfg, N, Cin, Cout, H, W)
    xd, wp, bd = x.cuda(), ops.pack_conv_weight(w.cuda()), b.cuda()

    def run():
        y = _nan(N, Cout, H, W)
        ops.conv2d(xd, wp, bd, act=1, cfg=cfg, split_k=split_k, out=y)
        return (y,)
    (y,) = _twice([_conv_ws(ops)], run)
    assert relerr(y, ref_conv(x, w, b, 3, 1, 1, 1, 0, 1, 1, None, None, None, None, 1, 0.0)) < 2e-5


def _norm_tol(conv_ref, eps_rel=5e-5):
    """InstanceNorm of a convolution output that is within e = eps_rel * max|x| of the truth, per plane: the mean moves by at
    most e and sigma by at most e (first order), so |dy| <= rstd * e * (2 + max|y|); + the norm's own 5e-6."""
    e = eps_rel * conv_ref.abs().max().item()
    rstd = 1.0 / (conv_ref.var((2, 3), unbiased=False) + 1e-5).sqrt()
    y = F.instance_norm(conv_ref, eps=1e-5)
    return (rstd.max() * e * (2 + y.abs().max())).item() + 5e-6, y


@pytest.mark.parametrize("defer", [False, True], ids=["reduce", "deferred_partials"])
def test_winograd_split3(ops, lib, defer):
    """64 -> 64 split over three parts of its input channels: the ordinary reduce launch, and DVC_CONV_DEFER_REDUCE with
    dvc_instnorm_apply_partials summing the partial sums straight from the workspace."""
    N, Cin, Cout, H, W = 2, 64, 64, 13, 24
    x, w, b = _conv_data(5, N, Cin, Cout, H, W)
    xd, u, bd = x.cuda(), ops.pack_winograd_weight(w.cuda()), b.cuda()
    ref = ref_conv(x, w, b, 3, 1, 1, 1, 0, 1, 1, None, None, None, None, 1, 0.0)

    def run():
        y = _nan(N, Cout, H, W)
        if not defer:
            ops.conv2d_winograd(xd, u, bd, act=1, split_k=3, out=y)
            return (y,)
        part = ops.conv2d_winograd(xd, u, bd, act=1, split_k=3, defer_reduce=True)
        assert isinstance(part, ops.ConvPartials) and part.S == 3
        ops.instnorm_apply(part, out=y)
        return (y,)
    (y,) = _twice([_conv_ws(ops)], run)
    if not defer:
        assert relerr(y, ref) < 5e-5
    else:
        tol, yref = _norm_tol(ref)
        assert (y.double().cpu() - yref).abs().max().item() < tol


def test_winograd_group_and_instnorm_group(ops):
    """Two independent layers as one dvc_conv2d_winograd_group launch, both split (their partial sums side by side in the
    workspace), summed by one dvc_instnorm_apply_group launch."""
    shapes = [(64, 64, 27, 48), (128, 64, 13, 24)]
    data = [_conv_data(11 + i, 1, ci, co, h, w) for i, (ci, co, h, w) in enumerate(shapes)]
    dev = [(x.cuda(), ops.pack_winograd_weight(w.cuda()), w.cuda(), b.cuda()) for x, w, b in data]

    def run():
        parts = ops.conv3x3_group([dict(x=x, weight=w, packs=(lambda kind, u=u: u), bias=b, act=1, defer_reduce=True) for x, u, w, b in dev])
        assert all(isinstance(p, ops.ConvPartials) and p.S > 1 for p in parts)
        assert parts[0].offset != parts[1].offset
        outs = [_nan(*p.shape) for p in parts]
        ops.instnorm_apply_group([dict(x=p, out=o) for p, o in zip(parts, outs)])
        return tuple(outs)
    assert ops.group_heads() and ops.fuse_reduce() and ops.conv_algo() == "auto"
    ys = _twice([_conv_ws(ops)], run)
    for y, (x, w, b) in zip(ys, data):
        tol, yref = _norm_tol(ref_conv(x, w, b, 3, 1, 1, 1, 0, 1, 1, None, None, None, None, 1, 0.0))
        assert (y.double().cpu() - yref).abs().max().item() < tol


def test_winograd_split_stays_inside_its_workspace(ops, lib):
    """Split 2 with a workspace of exactly the required size ([2][N][Cout][OH][OW] floats) inside a larger NaN-filled buffer: the
    bytes in front of and behind it are untouched."""
    N, Cin, Cout, H, W = 2, 64, 64, 13, 24
    x, w, b = _conv_data(6, N, Cin, Cout, H, W)
    xd, u, bd = x.cuda(), ops.pack_winograd_weight(w.cuda()), b.cuda()
    need = 2 * N * Cout * H * W          # floats
    guard = 4096
    buf = _nan(guard + need + guard)
    y = _nan(N, Cout, H, W)
    d = ops._conv_desc(N, Cin, H, W, Cout, act=1, split_k=2)
    assert ops._winograd_split(lib, d, need * 4) == (2, N)
    _check(lib.dvc_conv2d_winograd(ctypes.byref(d), _p(xd), _p(u), _p(bd), None, None, _p(y), _p(buf[guard:]), need * 4, ops._stream()),
           "dvc_conv2d_winograd")
    torch.cuda.synchronize()
    assert torch.isnan(buf[:guard]).all() and torch.isnan(buf[guard + need:]).all()
    assert not torch.isnan(buf[guard:guard + need]).any()          # every partial sum is written
    assert relerr(y, ref_conv(x, w, b, 3, 1, 1, 1, 0, 1, 1, None, None, None, None, 1, 0.0)) < 5e-5


def test_clip_loop_reuse_pattern(ops):
    """conv (split) -> unrelated conv (split, other shape) -> the first conv again, all through the one cached workspace: the
    third result equals the first bit for bit."""
    xa, wa, ba = _conv_data(21, 2, 96, 64, 13, 24)
    xb, wb, bb = _conv_data(22, 1, 128, 128, 21, 40)
    A = (xa.cuda(), ops.pack_conv_weight(wa.cuda()), ba.cuda())
    B = (xb.cuda(), ops.pack_conv_weight(wb.cuda()), bb.cuda())
    UA = ops.pack_winograd_weight(wa.cuda())
    UB = ops.pack_winograd_weight(wb.cuda())
    first = ops.conv2d(*A, act=1, split_k=4)
    first_w = ops.conv2d_winograd(A[0], UA, A[2], act=1, split_k=3)
    ops.conv2d(*B, act=1, split_k=8)
    ops.conv2d_winograd(B[0], UB, B[2], act=1, split_k=2)
    ops.conv2d(*B, act=1, cfg=36)
    third = ops.conv2d(*A, act=1, split_k=4)
    third_w = ops.conv2d_winograd(A[0], UA, A[2], act=1, split_k=3)
    assert torch.equal(first, third) and torch.equal(first_w, third_w)
    assert relerr(first, ref_conv(xa, wa, ba, 3, 1, 1, 1, 0, 1, 1, None, None, None, None, 1, 0.0)) < 2e-5


# ---- correlation
def _corr_inputs(ops, B, h, w, seed):
    g = torch.Generator().manual_seed(seed)
    P = h * w
    th = ops.corr_prepare((torch.randn(B, 256, P, generator=g) + 0.3).cuda())
    ph = ops.corr_prepare((torch.randn(B, 256, P, generator=g) - 0.2).cuda())
    lab_map = torch.randn(B, 3, 4 * h, 4 * w, generator=g) * 30
    return th, ph, lab_map, ops.avgpool4x4(lab_map.cuda()).view(B, 3, P)


def _assert_corr(out, th, ph, lab_map, T):
    """The checks of test_corr_fwd_vs_oracle against the float64 evaluation on the same fp32 theta / phi."""
    y_small, sim_small, argmax = out
    B, _, P = th.shape
    y64, sim64, am64, gap, S = _corr_truth(th.cpu(), ph.cpu(), lab_map, T)
    safe = gap > 2e-6
    rows = safe.unsqueeze(1).expand(B, 3, P)
    assert (sim_small.cpu().double().view(B, P) - sim64).abs().max().item() < 2e-6
    assert (argmax.cpu().long().view(B, P) == am64)[safe].all()
    assert ((y_small.cpu().double().view(B, 3, P) - y64).abs() / _y_bound(S, T, 1))[rows].max().item() <= 1.0


@pytest.mark.parametrize("T", [0.01, 1e-10])
def test_corr_fwd_ordinary_merge(ops, lib, T):
    B, h, w = 2, 9, 9
    P = h * w
    th, ph, lab_map, blab = _corr_inputs(ops, B, h, w, 31)
    nbytes = lib.dvc_corr_workspace_bytes(B, P)
    ws = torch.empty(nbytes, device="cuda", dtype=torch.uint8)

    def run():
        ys, ss, yu, su = _nan(B, 3, h, w), _nan(B, 1, h, w), _nan(B, 3, 4 * h, 4 * w), _nan(B, 1, 4 * h, 4 * w)
        am = torch.full((B, P), -1, device="cuda", dtype=torch.int32)
        _check(lib.dvc_corr_fwd(_p(th), _p(ph), _p(blab), T, 1.0, B, 256, h, w, _p(ys), _p(ss), _p(yu), _p(su), _p(am), _p(ws), nbytes,
                                ops._stream()), "dvc_corr_fwd")
        return ys, ss, am, yu, su
    ys, ss, am, yu, su = _twice([ws], run)
    assert (am >= 0).all() and (am < P).all()
    _assert_corr((ys, ss, am), th, ph, lab_map, T)
    assert torch.equal(yu, F.interpolate(ys, scale_factor=4, mode="nearest")) and torch.equal(su, F.interpolate(ss, scale_factor=4, mode="nearest"))


@pytest.mark.parametrize("T", [0.01, 1e-10])
def test_corr_fwd_deferred_merge(ops, lib, T):
    """Every output NULL: the partial softmax states stay in the workspace and dvc_corr_merge_pack merges them."""
    h, w = 9, 9
    P, HW = h * w, 16 * h * w
    th, ph, lab_map, blab = _corr_inputs(ops, 1, h, w, 32)
    nbytes = lib.dvc_corr_workspace_bytes(1, P)
    ws = torch.empty(nbytes, device="cuda", dtype=torch.uint8)
    g = torch.Generator().manual_seed(2)
    ia, ll, lab_prev = (torch.randn(HW, generator=g).cuda(), torch.randn(HW, generator=g).cuda(), torch.randn(2, HW, generator=g).cuda())

    def run():
        out7, yu, su = _nan(7, HW), _nan(3, HW), _nan(HW)
        _check(lib.dvc_corr_fwd(_p(th), _p(ph), _p(blab), T, 1.0, 1, 256, h, w, None, None, None, None, None, _p(ws), nbytes, ops._stream()),
               "dvc_corr_fwd")
        _check(lib.dvc_corr_merge_pack(_p(ws), nbytes, T, h, w, _p(ia), _p(ll), _p(lab_prev), _p(out7), _p(yu), _p(su), ops._stream()),
               "dvc_corr_merge_pack")
        return out7, yu, su
    out7, yu, su = _twice([ws], run)
    assert torch.equal(out7, torch.cat((ia.view(1, HW), yu[1:3], su.view(1, HW), ll.view(1, HW), lab_prev)))
    # the x4 nearest maps against the float64 evaluation: sample the top-left element of every 4 x 4 block
    small = lambda t: t.view(-1, 4 * h, 4 * w)[:, ::4, ::4].contiguous()          # noqa: E731
    assert torch.equal(yu.view(3, 4 * h, 4 * w), F.interpolate(small(yu).unsqueeze(0), scale_factor=4, mode="nearest")[0])
    y64, sim64, am64, gap, S = _corr_truth(th.cpu(), ph.cpu(), lab_map, T)
    rows = (gap > 2e-6).unsqueeze(1).expand(1, 3, P)
    assert (small(su).cpu().double().view(1, P) - sim64).abs().max().item() < 2e-6
    assert ((small(yu).cpu().double().view(1, 3, P) - y64).abs() / _y_bound(S, T, 1))[rows].max().item() <= 1.0


def _bf16_run(ops, lib, theta, phi, blab, B, h, w, T):
    """dvc_corr_fwd_bf16 twice over its own workspace (the candidate counters are appended with atomicAdd after an in-kernel
    reset); theta / phi: (fp32 [B,P,C], bf16 bit patterns [B,P,C]) pairs."""
    P = h * w
    nbytes = lib.dvc_corr_bf16_workspace_bytes(B, P)
    ws = torch.empty(nbytes, device="cuda", dtype=torch.uint8)
    (tf, tb), (pf, pb) = theta, phi

    def run():
        ys, ss, yu, su = _nan(B, 3, h, w), _nan(B, 1, h, w), _nan(B, 3, 4 * h, 4 * w), _nan(B, 1, 4 * h, 4 * w)
        am = torch.full((B, P), -1, device="cuda", dtype=torch.int32)
        _check(lib.dvc_corr_fwd_bf16(_p(tb), _p(pb), _p(tf), _p(pf), _p(blab), T, B, 256, h, w, _p(ys), _p(ss), _p(yu), _p(su), _p(am),
                                     _p(ws), nbytes, ops._stream()), "dvc_corr_fwd_bf16")
        return ys, ss, am, yu, su
    return _twice([ws], run)


def test_corr_fwd_bf16(ops, lib):
    B, h, w, T = 2, 12, 20, 1e-10
    P = h * w
    g = torch.Generator().manual_seed(33)
    raw_t, raw_p = torch.randn(B, 256, P, generator=g) + 0.3, torch.randn(B, 256, P, generator=g) - 0.2
    lab_map = torch.randn(B, 3, 4 * h, 4 * w, generator=g) * 30
    blab = ops.avgpool4x4(lab_map.cuda()).view(B, 3, P)
    thb, phb = ops.corr_prepare_bf16(raw_t.cuda()), ops.corr_prepare_bf16(raw_p.cuda())
    ys, ss, am, yu, su = _bf16_run(ops, lib, thb, phb, blab, B, h, w, T)
    th32, ph32 = thb[0].transpose(1, 2).contiguous(), phb[0].transpose(1, 2).contiguous()
    _assert_corr((ys, ss, am), th32, ph32, lab_map, T)
    assert torch.equal(yu, F.interpolate(ys, scale_factor=4, mode="nearest"))


def test_corr_fwd_bf16_exact_ties(ops, lib):
    """Three exactly duplicated exemplar columns spread over the key axis (the construction of
    test_corr_bf16_exact_ties_split_equally): every copy is a candidate, the colour is the mean of the three."""
    h, w, k, T = 12, 20, 3, 1e-10
    P = h * w
    th, ph, lab_map, dups, qs = _tie_case(h, w, k, "ranges", torch.Generator().manual_seed(77 * k + h))
    blab = ops.avgpool4x4(lab_map.cuda()).view(1, 3, P)

    def pair(t):
        t = t.transpose(1, 2).contiguous()
        return t.cuda(), t.to(torch.bfloat16).view(torch.int16).cuda()
    ys, ss, am, yu, su = _bf16_run(ops, lib, pair(th), pair(ph), blab, 1, h, w, T)
    mean_col = blab.cpu().double()[0][:, dups].mean(-1)
    e_mean = (ys.cpu().double().view(3, P)[:, qs] - mean_col[:, None]).abs().max().item()
    assert torch.isin(am[0].cpu().long()[qs], torch.tensor(dups)).all()
    assert e_mean <= 1e-5 + 4e-7 * blab.abs().max().item(), e_mean


# ---- the slot buffers of the weight-gradient kernels
def _rel_l2(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-300))


@pytest.mark.parametrize("S", [1, 5])
def test_cvn_wgrad_slots(ops, lib, S):
    N, Cin, Cout, H, W = 2, 8, 32, 12, 20
    g = torch.Generator().manual_seed(41)
    X, dZ = torch.randn(N, Cin, H, W, generator=g), torch.randn(N, Cout, H, W, generator=g)
    Xd, dZd = X.cuda(), dZ.cuda()
    nw = Cout * Cin * 9
    part = torch.empty(S * (nw + Cout), device="cuda")

    def run():
        out = _nan(nw + Cout)
        _check(lib.dvc_cvn_wgrad(_p(dZd), _p(Xd), N, Cin, Cout, H, W, 1, 1, S, _p(part), part.numel(), _p(out), ops._stream()), "dvc_cvn_wgrad")
        return (out,)
    (out,) = _twice([part], run)
    ref = torch.nn.grad.conv2d_weight(X.double(), (Cout, Cin, 3, 3), dZ.double(), padding=1)
    assert _rel_l2(out[:nw].view(Cout, Cin, 3, 3), ref) < 1e-6
    assert _rel_l2(out[nw:], dZ.double().sum((0, 2, 3))) < 1e-5


def test_warp_k1_wgrad_slots(ops, lib):
    from bwd_audit import SUM_FLOOR, YARD_FACTOR
    N, Cin, Cout, P, S = 2, 64, 32, 240, 3
    g = torch.Generator().manual_seed(42)
    dT, Fin = torch.randn(N, Cout, P, generator=g), torch.randn(N, Cin, P, generator=g) + 0.2
    dTd, Fd = dT.cuda(), Fin.cuda()
    nw = Cout * Cin
    part = torch.empty(S * (nw + Cout), device="cuda")

    def run():
        out = _nan(nw + Cout)
        _check(lib.dvc_warp_k1_wgrad(_p(dTd), _p(Fd), N, Cin, Cout, P, S, _p(part), part.numel(), _p(out), ops._stream()), "dvc_warp_k1_wgrad")
        return (out,)
    (out,) = _twice([part], run)
    rW, rb = torch.einsum("nop,ncp->oc", dT.double(), Fin.double()), dT.double().sum((0, 2))
    yW, yb = torch.einsum("nop,ncp->oc", dT, Fin), dT.sum((0, 2))           # the float32 CPU evaluation: the yardstick
    assert relerr(out[:nw].view(Cout, Cin), rW) <= max(SUM_FLOOR, YARD_FACTOR * relerr(yW, rW))
    assert relerr(out[nw:], rb) <= max(SUM_FLOOR, YARD_FACTOR * relerr(yb, rb))


def test_cvn_head_bwd_slots(ops, lib):
    from bwd_audit import ref_head_bwd
    B, C, H, W = 2, 128, 19, 45
    g = torch.Generator().manual_seed(43)
    R = torch.randn(B, C, H, W, generator=g)
    R = torch.where(R > 0, R, 0.2 * R)
    w = torch.randn(2, C, generator=g) * 0.1
    ab = (torch.tanh(torch.einsum("oc,bchw->bohw", w, R) + torch.randn(2, generator=g).view(1, 2, 1, 1)) * 128).contiguous()
    gr = torch.randn(B, 2, H, W, generator=g)
    abd, grd, wd, Rd = ab.cuda(), gr.cuda(), w.cuda().contiguous(), R.cuda()
    part = torch.empty(int(lib.dvc_cvn_head_bwd_workspace_floats(B, C, H * W)), device="cuda")

    def run():
        dZ, out = _nan(B, C, H, W), _nan(2 * C + 2)
        _check(lib.dvc_cvn_head_bwd(_p(abd), _p(grd), _p(wd), _p(Rd), B, C, H * W, 0.2, _p(dZ), _p(part), part.numel(), _p(out), ops._stream()),
               "dvc_cvn_head_bwd")
        return dZ, out
    dZ, out = _twice([part], run)
    dZ_ref, dW_ref, db_ref = ref_head_bwd(ab, gr, w, R, 0.2)
    assert _rel_l2(dZ, dZ_ref) < 1e-6 and _rel_l2(out[:2 * C].view(2, C), dW_ref) < 1e-6 and _rel_l2(out[2 * C:], db_ref) < 1e-6


# ---- clip-driver tail and ingest
def test_fgs_filter_workspace(ops, lib):
    from oracle import tail_oracle as T
    H, W, it = 33, 70, 3
    g = torch.Generator().manual_seed(51)
    guide = torch.randint(0, 256, (H, W), generator=g, dtype=torch.uint8)
    src = torch.randn(2, H, W, generator=g) * 30
    gd, sd = guide.cuda(), src.cuda()
    nbytes = lib.dvc_fgs_workspace_bytes(H, W, 1, 2, it)
    ws = torch.empty(nbytes, device="cuda", dtype=torch.uint8)

    def run():
        dst = _nan(2, H, W)
        _check(lib.dvc_fgs_filter(_p(gd), _p(sd), 1, 2, H, W, 500.0, 4.0, it, 0.25, _p(dst), _p(ws), nbytes, ops._stream()), "dvc_fgs_filter")
        return (dst,)
    (dst,) = _twice([ws], run)
    ref = np.stack([T.fgs_filter(guide.numpy(), src[k].numpy(), num_iter=it) for k in range(2)])
    assert np.abs(dst.cpu().numpy() - ref).max() < 1e-3


def test_center_pad_three_pass_workspace(ops, lib):
    from oracle import ingest_oracle as G
    src, dst = (37, 53), (16, 24)
    rng = np.random.default_rng(src[0] + 7 * src[1])
    yy, xx = np.mgrid[0:src[0], 0:src[1]]
    img = (127 + 100 * np.sin(yy / 17.0)[..., None] * np.cos(xx / 23.0)[..., None] + rng.normal(0, 12, src + (3,))).clip(0, 255).astype(np.uint8)
    x = torch.from_numpy(img).cuda()
    nbytes = lib.dvc_center_pad_workspace_bytes(*src)
    ws = torch.empty(nbytes, device="cuda", dtype=torch.uint8)

    def run():
        out = torch.full(dst + (3,), 255, device="cuda", dtype=torch.uint8)
        _check(lib.dvc_center_pad(_p(x), src[0], src[1], dst[0], dst[1], _p(out), _p(ws), nbytes, ops._stream()), "dvc_center_pad")
        return (out,)
    (out,) = _twice([ws], run)
    d = np.abs(out.cpu().numpy().astype(np.int32) - G.center_pad(img, dst).astype(np.int32))
    assert d.max() <= 1 and (d > 0).mean() < 0.02


# ---- non-local weighted average
def test_nlwa_fwd_workspace(ops, lib):
    """dvc_nlwa_fwd at the smallest case of tests/test_gpu_nonlocal_avg.py (16 x 25 positions): the zero-bordered feature, the
    resized ab and the partial softmax states all live in the workspace.  The C entry is called with the arguments the wrapper
    derives (dvc_amd.nonlocal_avg), so that `out` is the test's own NaN-filled tensor."""
    import nlwa_reference as R
    from dvc_amd import nonlocal_avg as NL
    from test_gpu_nonlocal_avg import CASES, _inputs
    xs, fs, k, alpha, sf = CASES["c64_k5_q"]
    x, f = _inputs(CASES["c64_k5_q"])
    (B, Cx, Hx, Wx), (C, Hf, Wf) = xs, fs[1:]
    H, W = NL._out_size(Hx, sf), NL._out_size(Wx, sf)
    assert (H, W) == (16, 25)
    sx, sfh, sfw = NL._src_scale_factor(sf), NL._src_scale_size(Hf, H), NL._src_scale_size(Wf, W)
    nbytes = lib.dvc_nlwa_workspace_bytes(B, C, k, H, W)
    ws = torch.empty(nbytes, device="cuda", dtype=torch.uint8)
    assert ws.data_ptr() % 256 == 0

    def run():
        out = _nan(B, 2, H, W)
        _check(lib.dvc_nlwa_fwd(_p(x), Cx, Hx, Wx, _p(f), C, Hf, Wf, B, H, W, sx, sx, sfh, sfw, k, float(alpha), _p(out), _p(ws), nbytes,
                                ops._stream()), "dvc_nlwa_fwd")
        return (out,)
    (got,) = _twice([ws], run)
    with torch.no_grad():
        assert torch.equal(got, NL.nonlocal_weighted_average(x, f, k, alpha, sf))         # the wrapper makes this very call
    ref64 = R.nonlocal_weighted_average(x.cpu(), f.cpu(), k, alpha, sf, dtype=torch.float64)
    ref32 = R.nonlocal_weighted_average(x.cpu(), f.cpu(), k, alpha, sf, dtype=torch.float32).double()
    tol = 4 * (ref32 - ref64).abs().max().item() + 1e-6 * ref64.abs().max().item()
    assert (got.cpu().double() - ref64).abs().max().item() <= tol


# ---- backward of the fused correlation
@pytest.mark.parametrize("with_dst", [True, False], ids=["dST", "no_dST"])
@pytest.mark.parametrize("wta", [1.0, 0.5])
def test_corr_softmax_bwd_rowstat_scratch(ops, lib, wta, with_dst):
    """dvc_corr_softmax_bwd on a block of 70 query rows in buffers laid out for ld_t = 96 (batch 2): the row-statistics kernel
    writes `rows` entries of each of the three [ld_t] arrays of rowstat_scratch, and entries rows .. ld_t - 1 keep whatever the
    scratch held.  dS is written for the block's rows only (the rest of the [ld_t][P] buffer stays as it was); dST [P][ld_t] is
    written whole, columns >= rows with zeros.  Reference: float64 autograd through the reference's op sequence (oracle.wta_scale,
    / T, softmax, the colour product, the row maximum) with the block's affinities as the leaf, at the 2e-3 of the largest
    gradient that tests/test_gpu_corr_backward.py allows the whole backward."""
    from oracle import dvc_oracle as O
    B, rows, ld_t, P, T = 2, 70, 96, 150, 0.01
    g = torch.Generator().manual_seed(61)
    base = torch.randn(B, 64, 6, generator=g)
    th = torch.randn(B, 64, rows, generator=g) + 2.0 * base[:, :, torch.randint(0, 6, (rows,), generator=g)]
    ph = torch.randn(B, 64, P, generator=g) + 2.0 * base[:, :, torch.randint(0, 6, (P,), generator=g)]
    th, ph = th / th.norm(dim=1, keepdim=True), ph / ph.norm(dim=1, keepdim=True)
    f = torch.einsum("bci,bcj->bij", th, ph).contiguous()                           # [B, rows, P] fp32: the kernel's input
    blab = torch.randn(B, 3, P, generator=g) * 30
    gy, gsim = torch.randn(B, 3, rows, generator=g), torch.randn(B, rows, generator=g)
    # float64 truth with f as the leaf; the forward's y (the kernel reads it) from the same evaluation
    f64 = f.double().requires_grad_(True)
    fw = f64 if wta == 1.0 else O.wta_scale(f64, wta)
    y64 = torch.matmul(F.softmax(fw / T, dim=-1), blab.double().permute(0, 2, 1)).permute(0, 2, 1)      # [B, 3, rows]
    ((y64 * gy.double()).sum() + (f64.max(-1)[0] * gsim.double()).sum()).backward()
    ref = f64.grad
    fd = _nan(B, ld_t, P)
    fd[:, :rows] = f.cuda()                 # (rows >= `rows` of the block buffer are never read: NaN there must not matter)
    bd, gyd, yd, gsd = blab.cuda(), gy.cuda().contiguous(), y64.detach().float().cuda().contiguous(), gsim.cuda().contiguous()
    amd = f.argmax(-1).to(torch.int32).cuda().contiguous()
    scratch = torch.empty(B * 3 * ld_t, device="cuda")

    def run():
        dS = _nan(B, ld_t, P)
        dST = _nan(B, P, ld_t) if with_dst else None
        _check(lib.dvc_corr_softmax_bwd(_p(fd), _p(bd), _p(gyd), _p(yd), None, _p(gsd), _p(amd), T, wta, B, rows, P, rows, ld_t, _p(scratch),
                                        _p(dS), _p(dST), ops._stream()), "dvc_corr_softmax_bwd")
        # (NaN marks what the launch left alone: compared as bit patterns, judged below)
        return (dS.view(torch.int32),) + ((dST,) if with_dst else ())
    outs = _twice([scratch], run)
    dS = outs[0].view(torch.float32)
    assert not torch.isnan(dS[:, :rows]).any() and torch.isnan(dS[:, rows:]).all()
    err, scale = (dS[:, :rows].double().cpu() - ref).abs().max().item(), ref.abs().max().item()
    assert err <= 2e-3 * scale, (err, scale)
    if with_dst:
        dST = outs[1]
        assert torch.equal(dST[:, :, :rows], dS[:, :rows].transpose(1, 2)) and (dST[:, :, rows:] == 0).all()
