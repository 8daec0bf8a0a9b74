"""GPU: Discriminator_x64 as a frozen critic (dvc_amd/gan.py, csrc/gan.hip) — every new kernel alone through the C ABI against
its float64 restatement (tests/gan_reference.py) on the same float32 inputs, then the whole network: both outputs and the input
gradient, seeded through `output`, through `feature4` and through both; bit-identity with the no-grad forward, reproducibility,
the u / v vectors after one and two forwards, gamma = 0.

Bound, per tensor (the yardstick of tests/test_gpu_warp_heads.py): error = max-abs difference / max-abs of the float64
restatement; error <= max(1e-6, 4 x the error of the float32 CPU restatement on the same inputs)."""
import ctypes
import functools
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gan_reference as R  # noqa: E402
from cabi_helpers import check, lib, nan_tensor, ops, ptr  # noqa: E402,F401

pytestmark = pytest.mark.gpu
NAN = float("nan")


def _rel(got, ref):
    return (got.detach().cpu().double() - ref.double()).abs().max().item() / max(ref.double().abs().max().item(), 1e-300)


def _assert_close(tag, got, r64, r32):
    err, yard = _rel(got, r64), _rel(r32, r64)
    bound = max(1e-6, 4 * yard)
    print(f"{tag}: hip {err:.3e}  float32 CPU restatement {yard:.3e}  bound {bound:.3e}")
    assert torch.isfinite(got).all(), tag
    assert err <= bound, (tag, err, bound)


def _inv(sigma):
    return torch.tensor([1.0 / sigma], dtype=torch.float32, device="cuda")


# ================================================================================================ conv4s2 and its input gradient
CONV_SHAPES = [(3, 5, 4, 4), (6, 8, 9, 14), (16, 40, 27, 48), (64, 64, 13, 24),
               (6, 8, 9, 13)]      # beyond the specified four: an odd width (the right-hand edge of both kernels)
SIGMA = 1.7


@functools.lru_cache(maxsize=None)
def _conv_case(shape, N):
    Cin, Cout, H, W = shape
    g = torch.Generator().manual_seed(Cin * 1000 + Cout + N)
    x = torch.randn(N, Cin, H, W, generator=g)
    w = torch.randn(Cout, Cin, 4, 4, generator=g) * (2.0 / (16 * Cin)) ** 0.5
    b = torch.randn(Cout, generator=g) * 0.5
    dz = torch.randn(N, Cout, H // 2, W // 2, generator=g)
    ref = {}
    for dt in (torch.float64, torch.float32):
        y = R.conv4s2(x.to(dt), w.to(dt), b.to(dt), SIGMA)
        dx = R.conv4s2_dgrad(dz.to(dt), w.to(dt), SIGMA, (H, W))
        ref[dt] = (y, dx, dx * R.lrelu_grad(x.to(dt)))
    return x, w, b, dz, ref


LEAD = 64      # floats of NaN guard in front of the first image (16-byte aligned behind it)


def _guarded(N, dense, pad):
    """(flat, body): a NaN-filled flat device buffer and its view body [N, dense + pad] that starts LEAD floats in — the guard in
    front of the first image, `pad` floats behind every image."""
    flat = nan_tensor(LEAD + N * (dense + pad))
    return flat, flat[LEAD:].view(N, dense + pad)


def _lead(n):
    """(flat, body): n NaN floats behind a LEAD-float NaN guard."""
    flat = nan_tensor(LEAD + n)
    return flat, flat[LEAD:]


def _guards_intact(flat, body, dense):
    return bool(torch.isnan(flat[:LEAD]).all() and torch.isnan(body[:, dense:]).all())


def _padded(t, pad):
    """t in the first `dense` floats of every row of a guarded buffer; (body, batch stride)."""
    N, dense = t.shape[0], t[0].numel()
    _, body = _guarded(N, dense, pad)
    body[:, :dense] = t.reshape(N, dense).cuda()
    return body, dense + pad


@pytest.mark.parametrize("N", [1, 3])
@pytest.mark.parametrize("shape", CONV_SHAPES)
def test_conv4s2_forward_alone(lib, ops, shape, N):
    Cin, Cout, H, W = shape
    x, w, b, _, ref = _conv_case(shape, N)
    OH, OW = H // 2, W // 2
    xbuf, xbs = _padded(x, 5)
    yflat, ybuf = _guarded(N, Cout * OH * OW, 7)
    d = ops._conv_desc(N, Cin, H, W, Cout, ksize=4, stride=2, pad=1, act=ops.ACT_LEAKY, act_slope=0.2, x_batch_stride=xbs,
                       y_batch_stride=ybuf.shape[1])
    wd, bd, inv = w.cuda(), b.cuda(), _inv(SIGMA)        # (named: a temporary's memory is reused before the launch reads it)
    check(lib.dvc_gan_conv4s2(ctypes.byref(d), ptr(xbuf), ptr(wd), ptr(bd), ptr(inv), ptr(ybuf), None), "conv4s2")
    torch.cuda.synchronize()
    assert _guards_intact(yflat, ybuf, Cout * OH * OW)          # in front of the first image and behind every image: untouched
    y = ybuf[:, :Cout * OH * OW].view(N, Cout, OH, OW)
    _assert_close(f"conv4s2 {shape} N={N}", y, ref[torch.float64][0], ref[torch.float32][0])
    # the wrapper, dense, is the same launch: same bits; without activation the pre-activation comes out
    y2 = ops.gan_conv4s2(x.cuda(), w.cuda(), b.cuda(), _inv(SIGMA))
    assert torch.equal(y2, y)
    z = ops.gan_conv4s2(x.cuda(), w.cuda(), b.cuda(), _inv(SIGMA), act=ops.ACT_NONE)
    assert torch.equal(torch.where(z > 0, z, z * 0.2), y)


@pytest.mark.parametrize("N", [1, 3])
@pytest.mark.parametrize("shape", CONV_SHAPES)
def test_conv4s2_dgrad_alone(lib, ops, shape, N):
    Cin, Cout, H, W = shape
    x, w, _, dz, ref = _conv_case(shape, N)
    zbuf, zbs = _padded(dz, 3)
    wd, xd, inv = w.cuda(), x.cuda(), _inv(SIGMA)
    for masked in (False, True):
        dxflat, dxbuf = _guarded(N, Cin * H * W, 9)
        d = ops._conv_desc(N, Cin, H, W, Cout, ksize=4, stride=2, pad=1, act=ops.ACT_LEAKY, act_slope=0.2,
                           x_batch_stride=dxbuf.shape[1], y_batch_stride=zbs)
        check(lib.dvc_gan_conv4s2_dgrad(ctypes.byref(d), ptr(zbuf), ptr(wd), ptr(inv), ptr(xd) if masked else None,
                                        ptr(dxbuf), None), "dgrad")
        torch.cuda.synchronize()
        assert _guards_intact(dxflat, dxbuf, Cin * H * W)
        dx = dxbuf[:, :Cin * H * W].view(N, Cin, H, W)
        i = 2 if masked else 1
        _assert_close(f"dgrad {shape} N={N} masked={masked}", dx, ref[torch.float64][i], ref[torch.float32][i])
        dx2 = ops.gan_conv4s2_dgrad(dz.cuda(), w.cuda(), _inv(SIGMA), (H, W), mask_act=x.cuda() if masked else None)
        assert torch.equal(dx2, dx)


# ================================================================================================ spectral norm
@pytest.mark.parametrize("Cout,K", [(8, 96), (1, 18 * 16), (1024, 8192)])
def test_spectral_sigma_alone(ops, Cout, K):
    g = torch.Generator().manual_seed(Cout + K)
    W = torch.randn(Cout, K, generator=g) * (2.0 / K) ** 0.5
    u0, v0 = R.l2n(torch.randn(Cout, generator=g)), R.l2n(torch.randn(K, generator=g))
    r64, r32 = (R.sigma_step(W.to(dt), u0.to(dt), v0.to(dt)) for dt in (torch.float64, torch.float32))
    u, v = u0.cuda(), v0.cuda()
    guard = nan_tensor(4)
    inv = ops.gan_spectral_sigma(W.cuda(), u, v)
    torch.cuda.synchronize()
    assert torch.isnan(guard).all()
    for name, got, a, b in (("u", u, r64[0], r32[0]), ("v", v, r64[1], r32[1]), ("sigma", 1.0 / inv, r64[2].view(1), r32[2].view(1))):
        _assert_close(f"sigma {Cout}x{K} {name}", got, a, b)
    # a second step from the device's own u (v is recomputed from u alone): against the restatement from the same u
    u1 = u.cpu()
    r64b = R.sigma_step(W.double(), u1.double(), v0.double())
    r32b = R.sigma_step(W, u1, v0)
    inv2 = ops.gan_spectral_sigma(W.cuda(), u, v)
    _assert_close(f"sigma {Cout}x{K} second step u", u, r64b[0], r32b[0])
    _assert_close(f"sigma {Cout}x{K} second step sigma", 1.0 / inv2, r64b[2].view(1), r32b[2].view(1))


def test_sn_weight_both_layouts(ops):
    g = torch.Generator().manual_seed(5)
    W, inv = torch.randn(12, 20, generator=g), torch.tensor([0.37])
    ws, wt = nan_tensor(12, 20), nan_tensor(20, 40)
    ops.gan_sn_weight(W.cuda(), inv.cuda(), scaled=ws, scaled_t=wt, col=12)
    assert torch.equal(ws.cpu(), W * inv) and torch.equal(wt[:, 12:24].cpu(), (W * inv).t())
    assert torch.isnan(wt[:, :12]).all() and torch.isnan(wt[:, 24:]).all()


# ================================================================================================ attention
@pytest.mark.parametrize("C,P,peak", R.ATTENTION_CASES)
def test_attention_core(ops, C, P, peak):
    from dvc_amd.gan import attention_core, attention_core_bwd
    q, k, v, do = R.attention_inputs(C, P, peak=peak)
    ref = {}
    for dt in (torch.float64, torch.float32):
        qq, kk, vv, dd = (t.to(dt) for t in (q, k, v, do))
        o, a = R.attention_core(qq, kk, vv)
        ref[dt] = (o, a) + tuple(R.attention_core_bwd(qq, kk, vv, a, dd))
    # q, k, v as the channel slices of one stacked tensor, as the module passes them
    qkv = torch.cat((q, k, v), 1).cuda()
    qd, kd, vd = qkv[:, :C], qkv[:, C:2 * C], qkv[:, 2 * C:]
    o, a = attention_core(qd, kd, vd)
    d = attention_core_bwd(qd, kd, vd, a, do.cuda())
    torch.cuda.synchronize()
    got = (o, a, d[:, :C], d[:, C:2 * C], d[:, 2 * C:])
    for name, t, r64, r32 in zip(("o", "a", "dq", "dk", "dv"), got, ref[torch.float64], ref[torch.float32]):
        assert torch.isfinite(t).all(), name
        if r64.abs().max() < 1e-20:
            assert t.abs().max().item() < 1e-20, name
        else:
            _assert_close(f"attention C={C} P={P} peak={peak} {name}", t, r64, r32)
    assert (a.sum(-1) - 1).abs().max().item() < 1e-5


@pytest.mark.parametrize("P", [1, 7, 33, 312])
def test_softmax_kernels_alone(lib, P):
    g = torch.Generator().manual_seed(P)
    rows = 9
    e, dA = torch.randn(rows, P, generator=g) * 4, torch.randn(rows, P, generator=g)
    e[0] += 200.0                                                       # a row that overflows without the max subtraction
    a64, a32 = R.softmax_rows(e.double()), R.softmax_rows(e)
    flat, buf = _lead(rows * P + 8)
    ed, ad, gd = e.cuda(), a32.cuda(), dA.cuda()
    check(lib.dvc_gan_softmax_rows(ptr(ed), rows, P, ptr(buf), None), "softmax")
    torch.cuda.synchronize()
    assert torch.isnan(buf[rows * P:]).all() and torch.isnan(flat[:LEAD]).all()
    a = buf[:rows * P].view(rows, P)
    _assert_close(f"softmax P={P}", a, a64, a32)
    flat2, buf2 = _lead(rows * P + 8)
    check(lib.dvc_gan_softmax_rows_bwd(ptr(ad), ptr(gd), rows, P, ptr(buf2), None), "softmax_bwd")
    torch.cuda.synchronize()
    assert torch.isnan(buf2[rows * P:]).all() and torch.isnan(flat2[:LEAD]).all()
    d64, d32 = R.softmax_rows_bwd(a32.double(), dA.double()), R.softmax_rows_bwd(a32, dA)
    if P == 1:
        assert torch.equal(buf2[:rows].cpu(), torch.zeros(rows))
    else:
        _assert_close(f"softmax_bwd P={P}", buf2[:rows * P].view(rows, P), d64, d32)


def test_scale_add_and_lrelu_bwd(ops):
    g = torch.Generator().manual_seed(2)
    o, x, d = (torch.randn(3, 5, 7, generator=g) for _ in range(3))
    gm = torch.tensor([0.3])
    assert _rel(ops.gan_scale_add(o.cuda(), gm.cuda(), x.cuda()), gm.double() * o.double() + x.double()) <= 1e-6     # one fma or two roundings
    assert torch.equal(ops.gan_scale_add(o.cuda(), torch.zeros(1).cuda(), x.cuda()).cpu(), x)      # gamma = 0: y == x exactly
    assert torch.equal(ops.gan_scale_add(o.cuda(), gm.cuda()).cpu(), gm * o)
    m = R.lrelu_grad(x)
    assert torch.equal(ops.gan_lrelu_bwd(o.cuda(), d.cuda(), x.cuda()).cpu(), (o + d) * m)
    assert torch.equal(ops.gan_lrelu_bwd(o.cuda(), None, x.cuda()).cpu(), o * m)
    assert torch.equal(ops.gan_lrelu_bwd(None, d.cuda(), x.cuda()).cpu(), d * m)


# ================================================================================================ last
@pytest.mark.parametrize("H,W", [(3, 6), (4, 9)])
def test_last_and_its_backward_alone(lib, ops, H, W):
    N, C = 3, 40
    g = torch.Generator().manual_seed(H * W)
    x, w, b, gr = torch.randn(N, C, H, W, generator=g), torch.randn(1, C, 3, 6, generator=g) * 0.1, torch.randn(1, generator=g), \
        torch.randn(N, 1, generator=g)
    ref = {dt: (R.last_fwd(x.to(dt), w.to(dt), b.to(dt), SIGMA), R.last_bwd(gr.to(dt), w.to(dt), SIGMA, x.shape),
                R.last_bwd(gr.to(dt), w.to(dt), SIGMA, x.shape) * R.lrelu_grad(x.to(dt))) for dt in (torch.float64, torch.float32)}
    xbuf, xbs = _padded(x, 4)
    oflat, out = _lead(N + 2)
    wd, bd, inv = w.cuda(), b.cuda(), _inv(SIGMA)
    check(lib.dvc_gan_last(ptr(xbuf), ptr(wd), ptr(bd), ptr(inv), N, C, H, W, xbs, ptr(out), None), "last")
    torch.cuda.synchronize()
    assert torch.isnan(out[N:]).all() and torch.isnan(oflat[:LEAD]).all()
    _assert_close(f"last {H}x{W}", out[:N].view(N, 1), ref[torch.float64][0], ref[torch.float32][0])
    assert torch.equal(ops.gan_last(x.cuda(), w.cuda(), b.cuda(), _inv(SIGMA)), out[:N].view(N, 1))
    for masked in (False, True):
        dx = ops.gan_last_bwd(gr.cuda(), w.cuda(), _inv(SIGMA), x.cuda(), mask=masked)
        i = 2 if masked else 1
        _assert_close(f"last_bwd {H}x{W} masked={masked}", dx, ref[torch.float64][i], ref[torch.float32][i])


# ================================================================================================ the whole network
NET_CASES = {"ndf8_192": (8, 192, 384, 2), "ndf8_216": (8, 216, 384, 2), "ndf64_216": (64, 216, 384, 1)}


@functools.lru_cache(maxsize=None)
def _net_case(name):
    """Inputs and, in float64 and float32, (output, feature4, dx through output, dx through feature4, dx through both, cache)."""
    from dvc_amd import synth
    ndf, H, W, N = NET_CASES[name]
    g = torch.Generator().manual_seed(ndf + H)
    sd = synth.discriminator_state_dict(0, ndf=ndf)
    x = torch.randn(N, 6, H, W, generator=g)
    g_out, g_f4 = torch.randn(N, 1, generator=g), torch.randn(N, 4 * ndf, H // 16, W // 16, generator=g)
    ref = {}
    for dt in (torch.float64, torch.float32):
        out, f4, c = R.forward(sd, x, dt)
        ref[dt] = (out, f4, R.backward(c, g_out, None), R.backward(c, None, g_f4), R.backward(c, g_out, g_f4), c)
    return sd, x, g_out, g_f4, ref


def _net(sd, ndf):
    from dvc_amd.gan import Discriminator_x64
    net = Discriminator_x64(ndf=ndf)
    net.load_state_dict(sd)
    return net.cuda().requires_grad_(False)


@pytest.mark.parametrize("name", list(NET_CASES))
def test_network_outputs_and_input_gradient(name):
    sd, x, g_out, g_f4, ref = _net_case(name)
    r64, r32 = ref[torch.float64], ref[torch.float32]
    ndf = NET_CASES[name][0]
    with torch.no_grad():
        out_ng, f4_ng = _net(sd, ndf)(x.cuda())
    seeds = {"output": (g_out, None, 2), "feature4": (None, g_f4, 3), "both": (g_out, g_f4, 4)}
    grads = {}
    for which, (go, gf, i) in seeds.items():
        net = _net(sd, ndf)                                             # a fresh module: the same u / v state every time
        xd = x.cuda().requires_grad_(True)
        out, f4 = net(xd)
        assert out.requires_grad and f4.requires_grad and out.shape == (x.shape[0], 1)
        assert torch.equal(out, out_ng) and torch.equal(f4, f4_ng)      # the grad-mode forward is the no-grad forward
        torch.autograd.backward([t for t, s in ((out, go), (f4, gf)) if s is not None], [s.cuda() for s in (go, gf) if s is not None])
        torch.cuda.synchronize()
        assert all(p.grad is None for p in net.parameters())            # the input gradient only
        grads[which] = xd.grad
        _assert_close(f"{name} dx through {which}", xd.grad, r64[i], r32[i])
    _assert_close(f"{name} output", out_ng, r64[0], r32[0])
    _assert_close(f"{name} feature4", f4_ng, r64[1], r32[1])
    # two runs from the same u / v: the same bits
    net = _net(sd, ndf)
    xd = x.cuda().requires_grad_(True)
    out, f4 = net(xd)
    torch.autograd.backward([out, f4], [g_out.cuda(), g_f4.cuda()])
    assert torch.equal(out, out_ng) and torch.equal(xd.grad, grads["both"])


def test_u_v_after_one_and_two_forwards_and_gamma_zero():
    sd, x, _, _, ref = _net_case("ndf8_216")
    net = _net(sd, 8).eval()                                            # eval() updates u / v too, as the reference does
    xd = x.cuda()
    with torch.no_grad():
        net(xd)
    got1 = {k: v.detach().cpu().clone() for k, v in net.state_dict().items()}
    c64, c32 = ref[torch.float64][5], ref[torch.float32][5]
    for prefix, (u64, v64) in c64["uv"].items():
        u32, v32 = c32["uv"][prefix]
        _assert_close(f"{prefix}.weight_u after one forward", got1[prefix + ".weight_u"], u64, u32)
        _assert_close(f"{prefix}.weight_v after one forward", got1[prefix + ".weight_v"], v64, v32)
        assert torch.equal(got1[prefix + ".weight_bar"], sd[prefix + ".weight_bar"])     # W_bar is never rewritten
    # the second forward starts from the first one's vectors: the restatement from the DEVICE's state after one forward
    with torch.no_grad():
        net(xd)
    got2 = net.state_dict()
    c64b, c32b = R.forward(got1, x, torch.float64)[2], R.forward(got1, x, torch.float32)[2]
    for prefix, (u64, v64) in c64b["uv"].items():
        assert not torch.equal(got2[prefix + ".weight_u"].cpu(), got1[prefix + ".weight_u"]) or u64.numel() == 1
        _assert_close(f"{prefix}.weight_u after two forwards", got2[prefix + ".weight_u"], u64, c32b["uv"][prefix][0])
        _assert_close(f"{prefix}.weight_v after two forwards", got2[prefix + ".weight_v"], v64, c32b["uv"][prefix][1])
    # gamma = 0: the attention block is the identity, exactly
    net0 = _net(sd, 8)
    with torch.no_grad():
        net0.attention.gamma.zero_()
        f4 = net0._forward(xd)[1]
        assert torch.equal(net0._attention_forward(f4, None), f4)


def test_module_refusals_on_the_device():
    sd, x, _, _, _ = _net_case("ndf8_192")
    net = _net(sd, 8)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        net(x)
    net.layer3[0].module.bias.requires_grad_(True)
    with pytest.raises(NotImplementedError, match="parameter gradients are not built yet"):
        net(x.cuda())
    with torch.no_grad():
        out, _ = net(x.cuda())                                          # under no_grad nothing is refused
    assert out.shape == (2, 1) and not out.requires_grad
    with pytest.raises(RuntimeError, match=r"160 x 384 input leaves a 2 x 6 map"):
        net(torch.zeros(1, 6, 160, 384, device="cuda"))
    # the filters are saved with the graph: a parameter rewritten between forward and backward is refused by autograd, not mixed in
    net = _net(sd, 8)
    out, _ = net(x.cuda().requires_grad_(True))
    net.load_state_dict(sd)
    with pytest.raises(RuntimeError, match="modified by an inplace operation"):
        out.sum().backward()
