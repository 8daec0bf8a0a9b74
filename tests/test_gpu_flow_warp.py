"""GPU: WarpingLayer (dvc_flow_warp_fwd / dvc_flow_warp_bwd, csrc/flow_warp.hip) against the float64 restatement
(tests/flow_warp_reference.py): forward and both gradients, out-of-range / huge / non-finite / integer flows, the many-to-one
scatter, scale independence of the integer accumulation, bitwise reproducibility and batch independence, the
one-gradient paths, non-contiguous inputs, train.py's chain and a workspace that starts as garbage.

Error = max-abs / max-abs of the float64 restatement on the same fp32 inputs; yardstick = the float32 CPU restatement's own;
forward <= 4 yard + 1e-6, each gradient <= max(1e-6, 4 yard)."""
import functools
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import flow_warp_reference as R  # noqa: E402

pytestmark = pytest.mark.gpu

SHAPES = {
    "train": (2, 3, 24, 40),
    "odd": (1, 3, 37, 53),       # no multiple of any tile
    "tiny": (1, 1, 2, 2),
    "wide": (1, 5, 9, 70),       # more than one x tile, one ragged
    "batch": (3, 2, 17, 33),
}
ALIGN = [False, True]
# U(-4, 4) px on a 2 x 2 map mostly samples outside it: at this seed the float64 restatement has 1 (align_corners=False) and
# 3 (True) samples with an in-range corner, so y, dx and dflow are non-zero in both modes (chosen on the reference alone)
SEEDS = {"tiny": 247}


def _off_integer(flow, align_corners):
    """Nudge the flows whose SAMPLE coordinate is within 2e-3 of an integer (the derivative is one-sided there)."""
    flow = flow.clone()
    for _ in range(6):
        px, py = R.sample_coords(flow, align_corners)
        flow[:, 0] += ((px - px.round()).abs() < 2e-3).float() * 0.013
        flow[:, 1] += ((py - py.round()).abs() < 2e-3).float() * 0.013
    return flow


def _assert_off_integer(flow, align_corners, keep=None):
    px, py = R.sample_coords(flow, align_corners)
    d = torch.minimum((px - px.round()).abs(), (py - py.round()).abs())
    if keep is not None:
        d = d[keep]
    assert (d >= 1e-3).all()


def _inputs(shape, align_corners, seed=0, kind="uniform"):
    """CPU float32 (x, flow, G): x ~ 50 N(0, 1), G ~ N(0, 1), flows U(-4, 4) px, or integer + U(0.05, 0.95) reaching
    +-(H + W) px ("far"), both kept 1e-3 away from integer sample coordinates."""
    B, C, H, W = shape
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(shape, generator=g) * 50
    G = torch.randn(shape, generator=g)
    if kind == "uniform":
        flow = torch.rand(B, 2, H, W, generator=g) * 8 - 4
    else:
        far = torch.randint(-(H + W), H + W + 1, (B, 2, H, W), generator=g).float()
        near = torch.randint(-2, 3, (B, 2, H, W), generator=g).float()
        flow = torch.where(torch.rand(B, 2, H, W, generator=g) < 0.35, far, near) + 0.05 + 0.9 * torch.rand(B, 2, H, W, generator=g)
    return x, _off_integer(flow, align_corners), G


@functools.lru_cache(maxsize=None)
def _reference(name, align_corners, kind="uniform"):
    """Computed once per case and shared: inputs, float64 (y, dx, dflow) and the float32 CPU composition's own."""
    x, flow, G = _inputs(SHAPES[name], align_corners, seed=SEEDS.get(name, 0), kind=kind)
    return (x, flow, G), R.gradients(x, flow, G, align_corners, torch.float64), R.gradients(x, flow, G, align_corners, torch.float32)


def _layer(align_corners):
    from dvc_amd.flow_warp import WarpingLayer
    return WarpingLayer(align_corners)


def _fwd_bwd(x, flow, G, align_corners, x_grad=True, flow_grad=True):
    """(y, dx or None, dflow or None) of the module on the device."""
    x = x.cuda().requires_grad_(x_grad)
    flow = flow.cuda().requires_grad_(flow_grad)
    y = _layer(align_corners)(x, flow)
    y.backward(G.cuda())
    torch.cuda.synchronize()
    return y.detach(), x.grad, flow.grad


def _rel(got, ref):
    return (got.cpu().double() - ref.double()).abs().max().item() / ref.abs().max().item()


def _check_fwd(tag, got, y64, y32):
    err, yard = _rel(got, y64), _rel(y32, y64)
    tol = 4 * yard + 1e-6
    print(f"{tag}: forward rel err {err:.3e}, fp32 CPU restatement {yard:.3e}, bound {tol:.3e}")
    assert err <= tol, (tag, err, yard)


def _check_grad(tag, what, got, g64, g32):
    err, yard = _rel(got, g64), _rel(g32, g64)
    tol = max(1e-6, 4 * yard)
    print(f"{tag}: {what} rel err {err:.3e}, fp32 CPU autograd {yard:.3e}, bound {tol:.3e} (max |{what}| {g64.abs().max().item():.3e})")
    assert torch.isfinite(got).all() and err <= tol, (tag, what, err, yard)


@pytest.mark.parametrize("align_corners", ALIGN)
@pytest.mark.parametrize("name", list(SHAPES))
def test_forward_and_gradients_match_float64_restatement(name, align_corners):
    (x, flow, G), (y64, dx64, df64), (y32, dx32, df32) = _reference(name, align_corners)
    _assert_off_integer(flow, align_corners)
    with torch.no_grad():
        y_ng = _layer(align_corners)(x.cuda(), flow.cuda())
    y, dx, df = _fwd_bwd(x, flow, G, align_corners)
    assert y.shape == y64.shape and y.dtype == torch.float32 and torch.isfinite(y).all()
    assert torch.equal(y_ng, y)                      # the no-grad forward is the grad-mode forward
    tag = f"{name} align={align_corners}"
    _check_fwd(tag, y, y64, y32)
    assert dx.shape == x.shape and df.shape == flow.shape
    assert df64.abs().max().item() > 1e-3 * G.abs().max().item()      # not an all-but-zero tensor
    _check_grad(tag, "dx", dx, dx64, dx32)
    _check_grad(tag, "dflow", df, df64, df32)


def test_frame_size_forward_and_backward():
    """One size-of-workload check, (2, 3, 216, 384), align_corners=False as train.py runs it."""
    shape = (2, 3, 216, 384)
    x, flow, G = _inputs(shape, False, seed=2)
    _assert_off_integer(flow, False)
    y64, dx64, df64 = R.gradients(x, flow, G, False, torch.float64)
    y32, dx32, df32 = R.gradients(x, flow, G, False, torch.float32)
    y, dx, df = _fwd_bwd(x, flow, G, False)
    _check_fwd("frame", y, y64, y32)
    _check_grad("frame", "dx", dx, dx64, dx32)
    _check_grad("frame", "dflow", df, df64, df32)


@pytest.mark.parametrize("align_corners", ALIGN)
def test_far_flows_leave_the_image(align_corners):
    """Flows of +-(H + W) px: whole regions and single corners at each border fall outside; zeros where all four are out."""
    (x, flow, G), (y64, dx64, df64), (y32, dx32, df32) = _reference("train", align_corners, "far")
    B, C, H, W = x.shape
    _assert_off_integer(flow, align_corners)
    px, py = R.sample_coords(flow, align_corners)
    x0, y0 = px.floor(), py.floor()
    assert (x0 == -1).any() and (x0 == W - 1).any() and (y0 == -1).any() and (y0 == H - 1).any()
    all_out = (x0 < -1) | (x0 > W - 1) | (y0 < -1) | (y0 > H - 1)
    assert all_out.any() and not all_out.all()
    y, dx, df = _fwd_bwd(x, flow, G, align_corners)
    mask = all_out[:, None].expand(B, C, H, W)
    assert (y.cpu()[mask] == 0).all() and (df.cpu()[all_out[:, None].expand(B, 2, H, W)] == 0).all()
    tag = f"far align={align_corners}"
    _check_fwd(tag, y, y64, y32)
    _check_grad(tag, "dx", dx, dx64, dx32)
    _check_grad(tag, "dflow", df, df64, df32)


@pytest.mark.parametrize("align_corners", ALIGN)
def test_huge_flows_give_zeros_and_touch_nothing(align_corners):
    """+-1e30 is finite: exact zeros there, a dx that ignores those pixels, a zero dflow."""
    (x, flow, G), _, _ = _reference("train", align_corners)
    flow = flow.clone()
    huge = torch.zeros(flow.shape[0], *flow.shape[2:], dtype=torch.bool)
    huge[0, 3, 5] = huge[0, 0, 0] = huge[1, 23, 39] = huge[1, 10, 7:30] = True
    flow[:, 0][huge] = 1e30
    flow[:, 1][huge & (torch.arange(flow.shape[3]) % 2 == 0)] = -1e30
    flow[1, 1, 2, 2] = 3e38
    huge[1, 2, 2] = True
    Gz = G * (~huge)[:, None]
    fz = torch.where(huge[:, None], torch.full_like(flow, 1e4), flow)    # the float64 reference: far out, no overflow games
    y64, dx64, _ = R.gradients(x, fz, Gz, align_corners, torch.float64)
    y32, dx32, _ = R.gradients(x, fz, Gz, align_corners, torch.float32)
    y, dx, df = _fwd_bwd(x, flow, G, align_corners)
    m = huge[:, None].expand_as(x)
    assert (y.cpu()[m] == 0).all() and (df.cpu()[huge[:, None].expand_as(flow)] == 0).all()
    assert torch.isfinite(y).all() and torch.isfinite(dx).all() and torch.isfinite(df).all()
    tag = f"huge align={align_corners}"
    _check_fwd(tag, y, y64, y32)
    _check_grad(tag, "dx", dx, dx64, dx32)


@pytest.mark.parametrize("align_corners", ALIGN)
def test_non_finite_flows(align_corners):
    """NaN and +-inf at three pixels: the forward is NaN exactly there; dx is finite and is the reference's with those
    pixels' G zeroed; their dflow is NaN."""
    (x, flow, G), _, _ = _reference("train", align_corners)
    flow = flow.clone()
    bad = torch.zeros(flow.shape[0], *flow.shape[2:], dtype=torch.bool)
    flow[0, 0, 4, 9] = float("nan")
    flow[0, 1, 20, 0] = float("inf")
    flow[1, 0, 0, 39] = float("-inf")
    bad[0, 4, 9] = bad[0, 20, 0] = bad[1, 0, 39] = True
    Gz = G * (~bad)[:, None]
    fz = torch.where(bad[:, None], torch.full_like(flow, 0.37), flow)
    y64, dx64, df64 = R.gradients(x, fz, Gz, align_corners, torch.float64)
    y32, dx32, df32 = R.gradients(x, fz, Gz, align_corners, torch.float32)
    y, dx, df = _fwd_bwd(x, flow, G, align_corners)
    y, dx, df = y.cpu(), dx.cpu(), df.cpu()
    m = bad[:, None].expand_as(x)
    assert torch.isnan(y[m]).all() and torch.isfinite(y[~m]).all()
    mf = bad[:, None].expand_as(flow)
    assert torch.isnan(df[mf]).all() and torch.isfinite(df[~mf]).all()
    tag = f"nonfinite align={align_corners}"
    keep = (~bad)[:, None]
    _check_fwd(tag, torch.where(keep, y, torch.zeros_like(y)), y64 * keep, y32 * keep)
    assert torch.isfinite(dx).all()
    _check_grad(tag, "dx", dx, dx64, dx32)
    _assert_off_integer(fz, align_corners)
    _check_grad(tag, "dflow", torch.where(keep, df, torch.zeros_like(df)), df64 * keep, df32 * keep)


@pytest.mark.parametrize("align_corners", ALIGN)
@pytest.mark.parametrize("zero", [True, False], ids=["zero", "integer"])
def test_integer_flows(zero, align_corners):
    """Integer flows (all zero included): with align_corners=True y is the shifted x bit for bit; forward and dx within
    bound for both modes.  dflow is not compared: the derivative is one-sided at integer coordinates."""
    shape = SHAPES["train"]
    B, C, H, W = shape
    x, _, G = _inputs(shape, align_corners, seed=4)
    g = torch.Generator().manual_seed(6)
    flow = torch.zeros(B, 2, H, W) if zero else torch.randint(-5, 6, (B, 2, H, W), generator=g).float()
    y64, dx64, _ = R.gradients(x, flow, G, align_corners, torch.float64)
    y32, dx32, _ = R.gradients(x, flow, G, align_corners, torch.float32)
    y, dx, _ = _fwd_bwd(x, flow, G, align_corners, flow_grad=False)
    if align_corners:
        sx = torch.arange(W).view(1, 1, W) + flow[:, 0].long()
        sy = torch.arange(H).view(1, H, 1) + flow[:, 1].long()
        ok = (sx >= 0) & (sx < W) & (sy >= 0) & (sy < H)
        bi = torch.arange(B).view(B, 1, 1).expand(B, H, W)
        want = torch.stack([torch.where(ok, x[bi, c, sy.clamp(0, H - 1), sx.clamp(0, W - 1)], torch.zeros(())) for c in range(C)], 1)
        assert torch.equal(y.cpu(), want)
        if zero:
            assert torch.equal(y.cpu(), x)
    tag = f"{'zero' if zero else 'integer'} align={align_corners}"
    _check_fwd(tag, y, y64, y32)
    _check_grad(tag, "dx", dx, dx64, dx32)


@pytest.mark.parametrize("align_corners", ALIGN)
def test_many_to_one_scatter(align_corners):
    """Every flow points at one source pixel plus U(0, 0.9): 960 contributions land on four destinations."""
    B, C, H, W = 1, 3, 24, 40
    g = torch.Generator().manual_seed(7)
    x = torch.randn(B, C, H, W, generator=g) * 50
    G = torch.randn(B, C, H, W, generator=g)
    ty, tx = 11, 17
    frac = torch.rand(B, 2, H, W, generator=g) * 0.9
    if align_corners:
        u = tx + frac[:, 0] - torch.arange(W).view(1, 1, W)
        v = ty + frac[:, 1] - torch.arange(H).view(1, H, 1)
    else:    # solve px = tx + frac for the flow
        u = (tx + frac[:, 0] + 0.5) * (W - 1) / W - torch.arange(W).view(1, 1, W)
        v = (ty + frac[:, 1] + 0.5) * (H - 1) / H - torch.arange(H).view(1, H, 1)
    flow = torch.stack((u, v), 1)
    px, py = R.sample_coords(flow, align_corners)
    assert (px.floor() == tx).float().mean() > 0.95 and (py.floor() == ty).float().mean() > 0.95
    _, dx64, _ = R.gradients(x, flow, G, align_corners, torch.float64)
    _, dx32, _ = R.gradients(x, flow, G, align_corners, torch.float32)
    assert (dx64 != 0).sum().item() <= 9 * C * B and dx64.abs().max().item() > 1.0
    _, dx, _ = _fwd_bwd(x, flow, G, align_corners, flow_grad=False)
    assert dx.abs().max().item() > 1.0
    _check_grad(f"many-to-one align={align_corners}", "dx", dx, dx64, dx32)


@pytest.mark.parametrize("scale", [1e20, 1e-20])
def test_dx_quantum_follows_the_scale_of_G(scale):
    """The same relative bound against the float64 reference of the scaled G: an absolute quantum fails one of the two."""
    (x, flow, G), _, _ = _reference("train", False)
    Gs = G * scale
    _, dx64, _ = R.gradients(x, flow, Gs, False, torch.float64)
    _, dx32, _ = R.gradients(x, flow, Gs, False, torch.float32)
    _, dx, _ = _fwd_bwd(x, flow, Gs, False, flow_grad=False)
    assert dx.abs().max().item() > 0
    _check_grad(f"G x {scale:g}", "dx", dx, dx64, dx32)


def test_zero_and_non_finite_G():
    """amax == 0 gives dx = 0; a NaN / inf in one image's G gives a NaN dx for that image only."""
    (x, flow, G), _, _ = _reference("batch", False)
    _, dx, _ = _fwd_bwd(x, flow, torch.zeros_like(G), False, flow_grad=False)
    assert (dx == 0).all()
    Gn = G.clone()
    Gn[1, 0, 3, 3] = float("inf")
    _, dxn, _ = _fwd_bwd(x, flow, Gn, False, flow_grad=False)
    _, dx0, _ = _fwd_bwd(x, flow, G, False, flow_grad=False)
    assert torch.isnan(dxn[1]).all() and torch.equal(dxn[0], dx0[0]) and torch.equal(dxn[2], dx0[2])


@pytest.mark.parametrize("align_corners", ALIGN)
def test_reproducible_and_batch_independent(align_corners):
    (x, flow, G), _, _ = _reference("batch", align_corners, "far")
    y, dx, df = _fwd_bwd(x, flow, G, align_corners)
    for _ in range(2):
        y2, dx2, df2 = _fwd_bwd(x, flow, G, align_corners)
        assert torch.equal(y, y2) and torch.equal(dx, dx2) and torch.equal(df, df2)
    # image 1 alone: a per-call amax would change dx's quantum.  Make the images' scales differ to be sure of it.
    Gs = G * torch.tensor([1.0, 1e-3, 64.0]).view(3, 1, 1, 1)
    y, dx, df = _fwd_bwd(x, flow, Gs, align_corners)
    y1, dx1, df1 = _fwd_bwd(x[1:2], flow[1:2], Gs[1:2], align_corners)
    assert torch.equal(y1, y[1:2]) and torch.equal(dx1, dx[1:2]) and torch.equal(df1, df[1:2])
    # one gradient at a time: the other launch's pieces are not needed and the bits do not change
    _, dxo, none = _fwd_bwd(x, flow, Gs, align_corners, flow_grad=False)
    assert none is None and torch.equal(dxo, dx)
    _, none, dfo = _fwd_bwd(x, flow, Gs, align_corners, x_grad=False)
    assert none is None and torch.equal(dfo, df)


def test_non_contiguous_inputs_and_grad_output():
    """x a channel slice [:, 1:3] of a Lab tensor, G non-contiguous (a transposed buffer)."""
    (x, flow, G), _, _ = _reference("train", False)
    lab = x.cuda().requires_grad_(True)
    fl = flow.cuda().requires_grad_(True)
    xs = lab[:, 1:3]
    assert not xs.is_contiguous()
    Gnc = G[:, 1:3].cuda().permute(0, 1, 3, 2).contiguous().permute(0, 1, 3, 2)
    assert not Gnc.is_contiguous()
    y = _layer(False)(xs, fl)
    y.backward(Gnc)
    yb, dxb, dfb = _fwd_bwd(x[:, 1:3].contiguous(), flow, G[:, 1:3].contiguous(), False)
    assert torch.equal(y.detach(), yb) and torch.equal(lab.grad[:, 1:3], dxb) and torch.equal(fl.grad, dfb)
    assert (lab.grad[:, 0] == 0).all()


def test_train_chain_matches_float64_autograd():
    """train.py's temporal term: loss = mean(((warp(lab_pred, flow))[:, 1:3] - last[:, 1:3])^2 mask), flow without grad."""
    (x, flow, _), _, _ = _reference("train", False)
    g = torch.Generator().manual_seed(12)
    last = torch.randn(x.shape, generator=g) * 50
    mask = (torch.rand(x.shape[0], 1, *x.shape[2:], generator=g) < 0.7).float()

    def chain(layer, lab_pred, flow, last, mask):
        lab_pred = lab_pred.detach().clone().requires_grad_(True)
        loss = torch.mean((layer(lab_pred, flow)[:, 1:3] - last[:, 1:3]) ** 2 * mask)
        loss.backward()
        return loss.detach(), lab_pred.grad

    l64, g64 = chain(lambda a, b: R.compose(a, b, False), x.double(), flow.double(), last.double(), mask.double())
    l32, g32 = chain(lambda a, b: R.compose(a, b, False), x, flow, last, mask)
    lg, gg = chain(_layer(None), x.cuda(), flow.cuda(), last.cuda(), mask.cuda())
    torch.cuda.synchronize()
    err, yard = _rel(gg, g64), _rel(g32, g64)
    tol = max(1e-6, 4 * yard)
    print(f"train chain: d lab_pred rel err {err:.3e}, fp32 CPU autograd {yard:.3e}, bound {tol:.3e}; loss {lg.item():.6e} / {l64.item():.6e}")
    assert err <= tol, (err, yard)
    assert (gg[:, 0] == 0).all() and gg[:, 1:3].abs().max().item() > 0


def test_workspace_may_start_as_garbage():
    """The int64 workspace is zeroed by the call itself: garbage in its backing memory changes nothing — through the module
    (a same-sized allocation filled with garbage and released just before the backward) and through the C-ABI on a
    workspace this test fills itself."""
    import ctypes
    from dvc_amd import _lib
    lib = _lib.load()
    (x, flow, G), _, _ = _reference("train", False)
    _, dx, _ = _fwd_bwd(x, flow, G, False, flow_grad=False)
    B, C, H, W = x.shape
    nbytes = lib.dvc_flow_warp_bwd_workspace_bytes(B, C, H, W)
    xd, fd, Gd = x.cuda().requires_grad_(True), flow.cuda(), G.cuda()
    y = _layer(False)(xd, fd)
    junk = torch.full((nbytes // 8,), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    del junk                         # back to the caching allocator: the backward's workspace has the same size
    y.backward(Gd)
    torch.cuda.synchronize()
    assert torch.equal(xd.grad, dx)
    ws = torch.full((nbytes // 8,), -0x0123456789ABCDEF, dtype=torch.int64, device="cuda")
    out = torch.empty_like(Gd)
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    rc = lib.dvc_flow_warp_bwd(p(xd.detach()), p(fd), p(Gd), B, C, H, W, 0, p(out), None, p(ws), nbytes, stream)
    torch.cuda.synchronize()
    assert rc == 0, lib.dvc_last_error()
    assert torch.equal(out, dx)
