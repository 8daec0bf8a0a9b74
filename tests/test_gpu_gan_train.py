"""GPU: Discriminator_x64's own parameter gradients (dvc_amd/gan.py behind set_parameter_training, csrc/gan_wgrad.hip) — every
new kernel alone through the C ABI against its float64 restatement (tests/gan_train_reference.py) on the same float32 inputs,
then the whole network: all 21 `.grad` and dx seeded through `output`, through `feature4` and through both; bit-identity with the
no-grad forward and with the frozen-critic path; the discriminator step as train.py writes it (two forwards, one backward);
partial freezing; the flag off; gamma = 0.

Bound, per tensor (the yardstick of tests/test_gpu_gan.py): error = max-abs difference / max-abs of the float64 restatement;
error <= max(1e-6, 4 x the error of the float32 CPU restatement on the same inputs).  Two gradients are sums with cancellation and
are measured against the sum of the absolute terms instead (gan_train_reference.param_grads, `scale`): d gamma against
sum |dy o|, and the bias gradient of key_conv — zero in exact arithmetic — against max_c sum |dk[c]|."""
import ctypes
import functools
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gan_reference as R  # noqa: E402
import gan_train_reference as T  # noqa: E402
from cabi_helpers import check, lib, nan_tensor, ops, ptr  # noqa: E402,F401

pytestmark = pytest.mark.gpu
F64, F32 = torch.float64, torch.float32
LEAD = 64      # floats of NaN guard


def _err(got, ref, scale=None):
    d = (got.detach().cpu().double() - ref.double()).abs().max().item()
    return d / (scale if scale is not None else max(ref.double().abs().max().item(), 1e-300))


def _assert_close(tag, got, r64, r32, scale=None):
    err, yard = _err(got, r64, scale), _err(r32, r64, scale)
    bound = max(1e-6, 4 * yard)
    print(f"{tag}: hip {err:.3e}  float32 CPU restatement {yard:.3e}  bound {bound:.3e}")
    assert torch.isfinite(got).all(), tag
    assert err <= bound, (tag, err, bound)


def _padded(t, pad):
    """t in the first `dense` floats of every row of a NaN-filled buffer [N, dense + pad] behind a NaN guard; (body, batch stride)."""
    N, dense = t.shape[0], t[0].numel()
    body = nan_tensor(LEAD + N * (dense + pad))[LEAD:].view(N, dense + pad)
    body[:, :dense] = t.reshape(N, dense).cuda()
    return body, dense + pad


# ================================================================================================ the 4x4 stride-2 weight gradient
CONV_SHAPES = [(3, 5, 4, 4), (6, 8, 9, 14), (16, 40, 27, 48), (64, 64, 13, 24), (6, 8, 9, 13),
               (9, 70, 6, 8)]      # Cin * 16 = 144 and Cout = 70 both cross a tile edge


@functools.lru_cache(maxsize=None)
def _conv_case(shape, N):
    Cin, Cout, H, W = shape
    g = torch.Generator().manual_seed(Cin * 1000 + Cout + N)
    x = torch.randn(N, Cin, H, W, generator=g)
    dz = torch.randn(N, Cout, H // 2, W // 2, generator=g)
    return x, dz, {dt: T.conv4s2_wgrad(dz.to(dt), x.to(dt)) for dt in (F64, F32)}


@pytest.mark.parametrize("S", [1, None, 5])
@pytest.mark.parametrize("N", [1, 3])
@pytest.mark.parametrize("shape", CONV_SHAPES)
def test_conv4s2_wgrad_alone(lib, ops, shape, N, S):
    Cin, Cout, H, W = shape
    x, dz, ref = _conv_case(shape, N)
    xbuf, xbs = _padded(x, 5)
    zbuf, zbs = _padded(dz, 3)
    d = ops._conv_desc(N, Cin, H, W, Cout, ksize=4, stride=2, pad=1, act=ops.ACT_LEAKY, act_slope=0.2, x_batch_stride=xbs,
                       y_batch_stride=zbs)
    default = lib.dvc_gan_conv4s2_wgrad_splits(ctypes.byref(d))
    assert default == ops.gan_conv4s2_wgrad_splits(N, Cin, H, W, Cout) >= 1
    S = default if S is None else S
    nw = Cout * Cin * 16
    ld = nw + Cout
    # one NaN buffer: guard | S slots | guard | out | guard
    flat = nan_tensor(LEAD + S * ld + LEAD + ld + LEAD)
    part, out = flat[LEAD:LEAD + S * ld], flat[2 * LEAD + S * ld:2 * LEAD + S * ld + ld]
    check(lib.dvc_gan_conv4s2_wgrad(ctypes.byref(d), ptr(zbuf), ptr(xbuf), S, ptr(part), S * ld, ptr(out), None), "wgrad")
    torch.cuda.synchronize()
    for lo in (0, LEAD + S * ld, 2 * LEAD + S * ld + ld):
        assert torch.isnan(flat[lo:lo + LEAD]).all(), lo                # in front of, between and behind the destinations
    assert torch.isfinite(part).all()                                   # every float of every slot is written
    G, db = out[:nw].view(Cout, Cin, 4, 4), out[nw:]
    _assert_close(f"wgrad {shape} N={N} S={S} G", G, ref[F64][0], ref[F32][0])
    _assert_close(f"wgrad {shape} N={N} S={S} db", db, ref[F64][1], ref[F32][1])
    # the wrapper, dense, is the same launch: the same bits, twice
    xd, zd = x.cuda(), dz.cuda()
    for _ in range(2):
        G2, db2 = ops.gan_conv4s2_wgrad(zd, xd, splits=S)
        assert torch.equal(G2, G) and torch.equal(db2, db)
    # all of dz on ONE output pixel: the gradient is that pixel's gathered input patch times the value, exactly, with zeros at
    # the taps that fall off the map — the top-left corner of the first image, the bottom-right corner of the last
    OH, OW = H // 2, W // 2
    val = torch.randn(Cout, generator=torch.Generator().manual_seed(7))
    xp = torch.nn.functional.pad(x, (1, 2, 1, 2))
    for n, oy, ox in ((0, 0, 0), (N - 1, OH - 1, OW - 1)):
        one = torch.zeros_like(dz)
        one[n, :, oy, ox] = val
        patch = xp[n, :, 2 * oy:2 * oy + 4, 2 * ox:2 * ox + 4]         # (row j of it is input row 2 oy + j - 1; off the map: 0)
        G1, db1 = ops.gan_conv4s2_wgrad(one.cuda(), xd, splits=S)
        assert torch.equal(G1.cpu(), val.view(Cout, 1, 1, 1) * patch[None]), (n, oy, ox)
        assert torch.equal(db1.cpu(), val)
        if (oy, ox) == (0, 0):
            assert (G1[:, :, 0, :] == 0).all() and (G1[:, :, :, 0] == 0).all() and (G1[:, :, 1:, 1:] != 0).any()


# ================================================================================================ the spectral-norm backward
@pytest.mark.parametrize("Cout,K,same", [(1, 18, False), (8, 96, False), (70, 144, False), (70, 144, True), (128, 2048, False)])
def test_sn_wgrad_alone(lib, ops, Cout, K, same):
    g = torch.Generator().manual_seed(Cout + K)
    W = torch.randn(Cout, K, generator=g) * (2.0 / K) ** 0.5
    G = W.clone() if same else torch.randn(Cout, K, generator=g)       # G = W_bar: c u v^T is as large as the first term
    u, v = R.l2n(torch.randn(Cout, generator=g)), R.l2n(torch.randn(K, generator=g))
    sigma = 1.7
    r64, r32 = (T.sn_wgrad(G.to(dt), W.to(dt), u.to(dt), v.to(dt), sigma) for dt in (F64, F32))
    flat = nan_tensor(LEAD + Cout * K + LEAD)
    out = flat[LEAD:LEAD + Cout * K]
    Gd, Wd, ud, vd, inv = G.cuda(), W.cuda(), u.cuda(), v.cuda(), torch.tensor([1.0 / sigma], device="cuda")
    nb = lib.dvc_gan_dot_workspace_bytes(Cout * K)
    ws = torch.empty(nb, dtype=torch.uint8, device="cuda")
    check(lib.dvc_gan_sn_wgrad(ptr(Gd), ptr(Wd), ptr(ud), ptr(vd), ptr(inv), Cout, K, ptr(out), ptr(ws), nb, None), "sn_wgrad")
    torch.cuda.synchronize()
    assert torch.isnan(flat[:LEAD]).all() and torch.isnan(flat[LEAD + Cout * K:]).all()
    _assert_close(f"sn_wgrad {Cout}x{K} same={same}", out.view(Cout, K), r64, r32)
    # the wrapper: the same bits; an existing buffer is REPLACED, not added to
    grad = torch.full((Cout, K), 3.0, device="cuda")
    assert ops.gan_sn_wgrad(Gd, Wd, ud, vd, inv, out=grad) is grad and torch.equal(grad.view(-1), out)
    assert torch.equal(ops.gan_sn_wgrad(Gd, Wd.view(Cout, K, 1, 1), ud, vd, inv).view(-1), out)


# ================================================================================================ last, and the inner product
@pytest.mark.parametrize("N", [1, 3])
@pytest.mark.parametrize("H,W", [(3, 6), (3, 7), (5, 9)])
def test_last_wgrad_alone(lib, ops, H, W, N):
    C = 16
    g = torch.Generator().manual_seed(H * W + N)
    x, gr = torch.randn(N, C, H, W, generator=g), torch.randn(N, 1, generator=g)
    (G64, b64), (G32, b32) = (T.last_wgrad(gr.to(dt), x.to(dt)) for dt in (F64, F32))
    xbuf, xbs = _padded(x, 4)
    flat = nan_tensor(LEAD + C * 18 + 1 + LEAD)
    out = flat[LEAD:LEAD + C * 18 + 1]
    gd = gr.cuda()
    check(lib.dvc_gan_last_wgrad(ptr(gd), ptr(xbuf), N, C, H, W, xbs, ptr(out), None), "last_wgrad")
    torch.cuda.synchronize()
    assert torch.isnan(flat[:LEAD]).all() and torch.isnan(flat[LEAD + C * 18 + 1:]).all()
    _assert_close(f"last_wgrad {H}x{W} N={N} G", out[:C * 18].view(1, C, 3, 6), G64, G32)
    _assert_close(f"last_wgrad {H}x{W} N={N} db", out[C * 18:], b64, b32)
    G2, db2 = ops.gan_last_wgrad(gd, x.cuda())
    assert torch.equal(G2.reshape(-1), out[:C * 18]) and torch.equal(db2, out[C * 18:])


@pytest.mark.parametrize("count", [1, 255, 100003])
def test_dot_alone(lib, ops, count):
    g = torch.Generator().manual_seed(count)
    a, b = torch.randn(count, generator=g), torch.randn(count, generator=g)
    r64, r32 = (a.double() * b.double()).sum().view(1), (a * b).sum().view(1)
    scale = (a.double() * b.double()).abs().sum().item()
    flat = nan_tensor(LEAD + 1 + LEAD)
    ad, bd = a.cuda(), b.cuda()
    nb = lib.dvc_gan_dot_workspace_bytes(count)
    ws = torch.empty(nb, dtype=torch.uint8, device="cuda")
    check(lib.dvc_gan_dot(ptr(ad), ptr(bd), count, ptr(flat[LEAD:]), ptr(ws), nb, None), "dot")
    torch.cuda.synchronize()
    assert torch.isnan(flat[:LEAD]).all() and torch.isnan(flat[LEAD + 1:]).all()
    _assert_close(f"dot {count}", flat[LEAD:LEAD + 1], r64, r32, scale)
    assert abs(flat[LEAD].item() - r64.item()) <= 2.0 ** -23 * abs(r64.item())         # rounded once
    assert torch.equal(ops.gan_dot(ad, bd), flat[LEAD:LEAD + 1]) and torch.equal(ops.gan_dot(ad.view(1, -1), bd), flat[LEAD:LEAD + 1])


# ================================================================================================ the whole network
NET_CASES = {"ndf8_192": (8, 192, 384, 2), "ndf8_216": (8, 216, 384, 2), "ndf64_216": (64, 216, 384, 1)}
SEEDS = {"output": (True, False), "feature4": (False, True), "both": (True, True)}


def _add(a, b):
    """The sum of two param_grads results (the gradients are linear in the seeds)."""
    return a[0] + b[0], {n: a[1][n] + b[1][n] for n in a[1]}, {n: a[2].get(n, 0.0) + b[2].get(n, 0.0) for n in set(a[2]) | set(b[2])}


@functools.lru_cache(maxsize=None)
def _net_case(name, gamma=None):
    """Inputs and, per dtype, (output, feature4, {seed: param_grads result})."""
    from dvc_amd import synth
    ndf, H, W, N = NET_CASES[name]
    g = torch.Generator().manual_seed(ndf + H + 1)
    sd = synth.discriminator_state_dict(0, ndf=ndf)
    if gamma is not None:
        sd["attention.gamma"] = torch.full((1,), gamma)
    x = torch.randn(N, 6, H, W, generator=g)
    g_out, g_f4 = torch.randn(N, 1, generator=g), torch.randn(N, 4 * ndf, H // 16, W // 16, generator=g)
    ref = {}
    for dt in (F64, F32):
        out, f4, c = R.forward(sd, x, dt)
        by = {"output": T.param_grads(sd, c, x, g_out, None), "feature4": T.param_grads(sd, c, x, None, g_f4)}
        by["both"] = _add(by["output"], by["feature4"])
        ref[dt] = (out, f4, by)
    return sd, x, g_out, g_f4, ref


def _net(sd, ndf, train=True):
    from dvc_amd.gan import Discriminator_x64
    net = Discriminator_x64(ndf=ndf)
    net.load_state_dict(sd)
    net = net.cuda()
    return net.set_parameter_training() if train else net.requires_grad_(False)


def _run(net, xd, go, gf, **kw):
    out, f4 = net(xd)
    torch.autograd.backward([t for t, s in ((out, go), (f4, gf)) if s is not None], [s.cuda() for s in (go, gf) if s is not None], **kw)
    torch.cuda.synchronize()
    return out, f4


def _check_grads(tag, net, r64, r32, dx=None):
    """Every parameter gradient (and dx) against the restatements (dx, grads, scale); a parameter no seeded output reaches has
    no gradient at all."""
    (dx64, g64, scale), (dx32, g32, _) = r64, r32
    params = dict(net.named_parameters())
    assert sorted(n for n in params if not n.endswith(("weight_u", "weight_v"))) == sorted(T.PARAM_NAMES)
    for n in T.PARAM_NAMES:
        got = params[n].grad
        if g64[n].abs().max() == 0:
            assert got is None or got.abs().max().item() == 0, n
            continue
        assert got is not None and got.shape == params[n].shape, n
        _assert_close(f"{tag} {n}", got, g64[n], g32[n], scale.get(n))
    for n, p in params.items():
        assert n in T.PARAM_NAMES or p.grad is None, n                 # weight_u / weight_v
    if dx is not None:
        _assert_close(f"{tag} dx", dx, dx64, dx32)


def _grad_bits(net):
    return {n: None if p.grad is None else p.grad.clone() for n, p in net.named_parameters()}


def _same_bits(a, b):
    return a.keys() == b.keys() and all((a[n] is None and b[n] is None) or torch.equal(a[n], b[n]) for n in a)


@pytest.mark.parametrize("name", list(NET_CASES))
def test_network_parameter_gradients(name):
    sd, x, g_out, g_f4, ref = _net_case(name)
    ndf = NET_CASES[name][0]
    with torch.no_grad():
        out_ng, f4_ng = _net(sd, ndf)(x.cuda())
    frozen = _net(sd, ndf, train=False)
    x_fr = x.cuda().requires_grad_(True)
    out_fr, f4_fr = _run(frozen, x_fr, g_out, g_f4)
    assert torch.equal(out_fr, out_ng) and torch.equal(f4_fr, f4_ng)
    for which, (so, sf) in SEEDS.items():
        go, gf = g_out if so else None, g_f4 if sf else None
        net = _net(sd, ndf)                                             # a fresh module: the same u / v state every time
        assert all(p.requires_grad for n, p in net.named_parameters() if n in T.PARAM_NAMES)
        xd = x.cuda().requires_grad_(True)
        out, f4 = _run(net, xd, go, gf)
        assert out.requires_grad and f4.requires_grad
        assert torch.equal(out, out_ng) and torch.equal(f4, f4_ng)      # the training forward is the no-grad forward, bit for bit
        _check_grads(f"{name} through {which}:", net, ref[F64][2][which], ref[F32][2][which], xd.grad)
    assert torch.equal(xd.grad, x_fr.grad)                              # dx (through both): the frozen path's, bit for bit
    # a second run from the same state: the same bits for every gradient
    again = _net(sd, ndf)
    xd2 = x.cuda().requires_grad_(True)
    _run(again, xd2, g_out, g_f4)
    assert _same_bits(_grad_bits(net), _grad_bits(again)) and torch.equal(xd2.grad, xd.grad)


def test_discriminator_step_as_train_py_writes_it(monkeypatch):
    """One module, forward on a "real" batch, forward on a "fake" batch, the relativistic least-squares loss, one backward.  The
    restatement runs the two forwards in sequence, the second from the DEVICE's u / v after the first, and differentiates each
    through its own sigma."""
    from dvc_amd import ops as O
    sd, real, _, _, _ = _net_case("ndf8_216")
    ndf, H, W, N = NET_CASES["ndf8_216"]
    fake = torch.randn(N, 6, H, W, generator=torch.Generator().manual_seed(77))
    dgrad_maps = []
    orig = O.gan_conv4s2_dgrad
    monkeypatch.setattr(O, "gan_conv4s2_dgrad", lambda dz, w, inv, in_hw, **kw: (dgrad_maps.append(tuple(in_hw)), orig(dz, w, inv, in_hw, **kw))[1])
    net = _net(sd, ndf)
    rd, fd = real.cuda(), fake.cuda()
    r, _ = net(rd)
    sd1 = {k: v.detach().cpu().clone() for k, v in net.state_dict().items()}      # u / v as the first forward left them
    f, _ = net(fd)
    loss = T.relativistic_ls_loss(r, f)
    loss.backward(retain_graph=True)
    torch.cuda.synchronize()
    assert rd.grad is None and fd.grad is None
    assert len(dgrad_maps) == 2 * 5 and (H, W) not in dgrad_maps        # per forward: layers 6 .. 2; layer1's dgrad is not launched

    res, stale = {}, None
    for dt in (F64, F32):
        r_ref, _, c1 = R.forward(sd, real, dt)
        f_ref, _, c2 = R.forward(sd1, fake, dt)
        g_r, g_f = T.relativistic_ls_seeds(r_ref, f_ref)
        res[dt] = _add(T.param_grads(sd, c1, real, g_r), T.param_grads(sd1, c2, fake, g_f))
        if dt == F64:
            # the mistake this test exists for: the backward of forward #1 reading the vectors forward #2 left in the module
            stale = _add(T.param_grads(sd, dict(c1, uv=c2["uv"]), real, g_r), T.param_grads(sd1, c2, fake, g_f))
    _check_grads("discriminator step:", net, res[F64], res[F32])
    # ... and it could not pass: under it some W_bar gradient is off by far more than any bound above
    worst = max(_err(stale[1][n], res[F64][1][n]) for n in T.PARAM_NAMES if n.endswith("weight_bar"))
    bounds = [max(1e-6, 4 * _err(res[F32][1][n], res[F64][1][n])) for n in T.PARAM_NAMES if n.endswith("weight_bar")]
    print(f"stale u / v would be off by {worst:.3e}; the largest bound is {max(bounds):.3e}")
    assert worst > 100 * max(bounds)

    # a second backward accumulates: .grad doubles, exactly
    first = _grad_bits(net)
    loss.backward()
    torch.cuda.synchronize()
    for n, p in net.named_parameters():
        if n in T.PARAM_NAMES:
            assert torch.equal(p.grad, first[n] * 2), n


def test_partial_freezing_and_flag_off():
    sd, x, g_out, g_f4, _ = _net_case("ndf8_192")
    hot = ("layer3.0.module.bias", "attention.gamma")
    full = _net(sd, 8)
    _run(full, x.cuda(), g_out, g_f4)
    net = _net(sd, 8).requires_grad_(False)
    for n, p in net.named_parameters():
        p.requires_grad_(n in hot)
    _run(net, x.cuda(), g_out, g_f4)
    want = dict(full.named_parameters())
    for n, p in net.named_parameters():
        if n in hot:
            assert torch.equal(p.grad, want[n].grad), n                 # the same bits as in the all-hot run
        else:
            assert p.grad is None, n
    # flag off: the refusal test_module_refusals_on_the_device pins, unchanged
    net.set_parameter_training(False)
    with pytest.raises(NotImplementedError, match="parameter gradients are not built yet"):
        net(x.cuda())


def test_gamma_zero():
    """gamma = 0, the module's initial value: d gamma is still right (o is recomputed, not divided out of y), and nothing flows
    into the three projections — their gradients are exactly zero."""
    sd, x, g_out, g_f4, ref = _net_case("ndf8_192", 0.0)
    net = _net(sd, 8)
    assert net.attention.gamma.item() == 0.0
    xd = x.cuda().requires_grad_(True)
    _run(net, xd, g_out, g_f4)
    r64, r32 = ref[F64][2]["both"], ref[F32][2]["both"]
    assert r64[1]["attention.gamma"].abs().item() > 1e-6 * r64[2]["attention.gamma"]
    params = dict(net.named_parameters())
    _assert_close("gamma = 0: d gamma", params["attention.gamma"].grad, r64[1]["attention.gamma"], r32[1]["attention.gamma"],
                  r64[2]["attention.gamma"])
    for conv in R.ATT:
        for k in ("weight_bar", "bias"):
            grad = params[f"attention.{conv}.module.{k}"].grad
            assert grad is not None and grad.abs().max().item() == 0, (conv, k)
    for n in T.PARAM_NAMES:
        if not n.startswith("attention."):
            _assert_close(f"gamma = 0: {n}", params[n].grad, r64[1][n], r32[1][n])
    _assert_close("gamma = 0: dx", xd.grad, r64[0], r32[0])
