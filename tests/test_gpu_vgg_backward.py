"""GPU: the input gradient of VGG19_pytorch (frozen weights) and of tensor_lab2rgb — the chain train.py:649-668 trains
through — against float64 CPU autograd through the oracle (tests/vgg_bwd_reference.py), the pool + activation backward bit
for bit against ATen, and the reference's perceptual / contextual chain end to end through the drop-in modules."""
import contextlib
import io
import time

import pytest
import torch
import torch.nn.functional as F

import vgg_bwd_reference as VR
from oracle import dvc_oracle as O

pytestmark = pytest.mark.gpu

KEYS5 = ["r12", "r22", "r32", "r42", "r52"]
R_KEYS = ["r11", "r12", "r21", "r22", "r31", "r32", "r33", "r34", "r41", "r42", "r43", "r44", "r51", "r52", "r53", "r54"]


def _vgg(pool="max"):
    from dvc_amd import synth
    from models.NonlocalNet import VGG19_pytorch
    with contextlib.redirect_stdout(io.StringIO()):
        m = VGG19_pytorch(pool=pool)
    m.load_state_dict(synth.vgg19_state_dict(0))
    for p in m.parameters():
        p.requires_grad = False      # train.py freezes vggnet
    return m.eval().cuda()


def _image(seed, B, H, W):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(B, 3, H, W, generator=g)


CASES = [
    # (id, B, H, W, keys, preprocess, pool, keys whose gradient is None)
    ("216x384", 1, 216, 384, KEYS5, True, "max", ()),
    ("odd45x70", 1, 45, 70, KEYS5, True, "max", ()),
    ("no_preprocess", 2, 64, 112, KEYS5, False, "max", ()),
    ("avg_pool", 1, 45, 70, ["r12", "p1", "r32", "p4", "r52"], True, "avg", ()),
    ("subset_r32", 2, 64, 112, ["r32"], True, "max", ()),
    ("p3_r44", 1, 45, 70, ["p3", "r44"], True, "max", ()),
    ("none_grad", 1, 64, 112, ["r22", "r42", "r51"], True, "max", ("r51",)),
]


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_vgg_input_grad_vs_float64(case):
    name, B, H, W, keys, pre, pool, none_keys = case
    from dvc_amd import synth
    sd = synth.vgg19_state_dict(0)
    m = _vgg(pool)
    x_cpu = _image(11, B, H, W)
    x = x_cpu.cuda().requires_grad_(True)
    outs = m(x, keys, preprocess=pre)
    assert all(o.requires_grad for o in outs)
    G = VR.loss_grads([o.detach().cpu() for o in outs], seed=7)
    G = [None if k in none_keys else g for k, g in zip(keys, G)]
    loss = sum((o * g.float().cuda()).sum() for o, g in zip(outs, G) if g is not None)
    loss.backward()
    got = x.grad.detach().cpu().double()
    # the device's own masks and routes (a no-grad forward returns the bits the grad-mode forward saved)
    with torch.no_grad():
        last = max(VR.O._VGG_SEQ.index(next(s for s in VR.O._VGG_SEQ if s[0] == k)) for k in keys)
        rk = [k for k in R_KEYS if VR.O._VGG_SEQ.index(next(s for s in VR.O._VGG_SEQ if s[0] == k)) < last + 1]
        pins = dict(zip(rk, [r.cpu() for r in m(x.detach(), rk, preprocess=pre)]))
    t0 = time.time()
    ref = VR.vgg_input_grad64(sd, x_cpu, keys, G, preprocess=pre, pool=pool, pins=pins)
    t_ref = time.time() - t0
    l2, mx = VR.rel_errors(got, ref)
    cpu32 = VR.rel_errors(VR.vgg_input_grad_f32(sd, x_cpu, keys, G, preprocess=pre, pool=pool), ref)
    msg = (f"vgg dx {name}: rel L2 {l2:.2e}, max-abs/max {mx:.2e} (CPU fp32 autograd: {cpu32[0]:.2e} / {cpu32[1]:.2e}; "
           f"float64 reference {t_ref:.0f} s)")
    if H * W <= 64 * 112:
        plain = VR.rel_errors(got, VR.vgg_input_grad64(sd, x_cpu, keys, G, preprocess=pre, pool=pool))
        msg += f"; vs float64 with its own masks: {plain[0]:.2e} / {plain[1]:.2e}"
    print(msg)
    assert torch.isfinite(got).all()
    assert l2 <= 1e-4, msg
    assert mx <= 1e-3, msg


def test_grad_mode_forward_is_bit_identical():
    """Every returned key, the pools (fused into the convolution in front of them) included, equals the no-grad forward."""
    keys = ["r11", "p1", "r22", "p2", "r34", "p3", "r44", "p4", "r52", "r12", "r32", "r42"]
    for pool, pre, (H, W) in (("max", True, (64, 112)), ("max", False, (45, 70)), ("avg", True, (64, 112))):
        m = _vgg(pool)
        x = _image(3, 2, H, W).cuda()
        with torch.no_grad():
            ref = m(x, keys, preprocess=pre)
        got = m(x.clone().requires_grad_(True), keys, preprocess=pre)
        for k, a, b in zip(keys, got, ref):
            assert a.requires_grad and a.shape == b.shape, k
            assert torch.equal(a.detach(), b), (pool, pre, k)


def test_backward_is_deterministic():
    m = _vgg()
    x0 = _image(5, 2, 64, 112).cuda()
    grads = []
    for _ in range(2):
        x = x0.clone().requires_grad_(True)
        outs = m(x, KEYS5)
        G = VR.loss_grads([o.detach().cpu() for o in outs], seed=1)
        sum((o * g.float().cuda()).sum() for o, g in zip(outs, G)).backward()
        grads.append(x.grad.clone())
    assert torch.equal(grads[0], grads[1])


def _crafted(seed, N, C, H, W):
    """Pre-activations with many exact ties (a few levels), exact zeros after the ReLU and negative entries."""
    g = torch.Generator().manual_seed(seed)
    z = (torch.randint(-2, 4, (N, C, H, W), generator=g).float() * 0.5)
    return z


@pytest.mark.parametrize("H,W", [(8, 10), (7, 9), (6, 5), (9, 8), (2, 2), (3, 3)])
@pytest.mark.parametrize("pool", ["max", "avg"])
def test_pool_act_bwd_bit_exact_vs_aten(H, W, pool):
    """ops.vgg_pool_act_bwd against ATen CPU relu + max_pool2d / avg_pool2d autograd in float32, bit for bit: exact positive ties
    (the first maximum in scan order takes the gradient), zeros (masked), odd edges (gR only), with and without each term."""
    from dvc_amd import ops
    N, C = 2, 3
    z = _crafted(H * 31 + W, N, C, H, W)
    g = torch.Generator().manual_seed(H + 7 * W)
    dP = torch.randn(N, C, H // 2, W // 2, generator=g)
    gP = torch.randn(N, C, H // 2, W // 2, generator=g)
    gR = torch.randn(N, C, H, W, generator=g)
    for use in ((1, 1, 1), (1, 0, 1), (1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0)):
        zz = z.clone().requires_grad_(True)
        r = F.relu(zz)
        p = F.max_pool2d(r, 2, 2) if pool == "max" else F.avg_pool2d(r, 2, 2)
        terms = []
        if use[0]:
            terms.append((p * dP).sum())
        if use[1]:
            terms.append((p * gP).sum())
        if use[2]:
            terms.append((r * gR).sum())
        sum(terms).backward()
        got = ops.vgg_pool_act_bwd(dP.cuda() if use[0] else None, gP.cuda() if use[1] else None, gR.cuda() if use[2] else None,
                                   r.detach().cuda(), avg=pool == "avg")
        assert torch.equal(got.cpu(), zz.grad), (H, W, pool, use, (got.cpu() - zz.grad).abs().max())


def test_act_bwd_bit_exact_vs_aten():
    """ops.vgg_act_bwd (float4 and scalar paths, in place) against ATen relu autograd: (dX + g) * [R > 0]."""
    from dvc_amd import ops
    for shape in ((2, 8, 6, 10), (1, 3, 5, 7)):
        z = _crafted(1, *shape)
        g = torch.Generator().manual_seed(2)
        dX, gR = torch.randn(shape, generator=g), torch.randn(shape, generator=g)
        zz = z.clone().requires_grad_(True)
        r = F.relu(zz)
        ((r * dX).sum() + (r * gR).sum()).backward()
        R = r.detach().cuda()
        assert torch.equal(ops.vgg_act_bwd(dX.cuda(), gR.cuda(), R).cpu(), zz.grad)
        d = dX.cuda()
        assert torch.equal(ops.vgg_act_bwd(d, gR.cuda(), R, out=d).cpu(), zz.grad)
        zz.grad = None
        (F.relu(zz) * gR).sum().backward()
        assert torch.equal(ops.vgg_act_bwd(None, gR.cuda(), R).cpu(), zz.grad)


def _lab_spread(seed, N, H, W):
    """L over [-10, 110], a and b over [-160, 160]: every branch of the forward, and saturated pixels where a clamp zeroes the
    gradient."""
    g = torch.Generator().manual_seed(seed)
    L = torch.rand(N, 1, H, W, generator=g) * 120 - 10
    ab = torch.rand(N, 2, H, W, generator=g) * 320 - 160
    return torch.cat((L, ab), 1)


def test_tensor_lab2rgb_grad_vs_float64():
    from dvc_amd import ops
    from utils.util import tensor_lab2rgb
    lab = _lab_spread(4, 2, 48, 80)
    x = lab.cuda().requires_grad_(True)
    y = tensor_lab2rgb(x)
    assert y.requires_grad
    assert torch.equal(y.detach(), ops.lab2rgb(lab.cuda()))
    G = torch.randn(y.shape, generator=torch.Generator().manual_seed(9))
    (y * G.cuda()).sum().backward()
    x64 = lab.double().requires_grad_(True)
    (O.tensor_lab2rgb(x64) * G.double()).sum().backward()
    ref, got = x64.grad, x.grad.cpu().double()
    sat = (ref == 0).all(1)
    assert sat.float().mean() > 0.05 and (~sat).float().mean() > 0.3     # both saturated and live pixels are covered
    l2, mx = VR.rel_errors(got, ref)
    print(f"tensor_lab2rgb dlab: rel L2 {l2:.2e}, max-abs/max {mx:.2e}")
    assert l2 <= 1e-5 and mx <= 1e-4, (l2, mx)
    with torch.no_grad():
        assert not tensor_lab2rgb(x).requires_grad


def test_training_chain_ab_grad_vs_float64():
    """train.py:649-668 written with the drop-in modules: leaf ab -> cat(uncenter_l(L), ab) -> tensor_lab2rgb -> VGG19_pytorch
    -> ContextualLoss_forward on r42 / r52 + MSE on r52; ab.grad against float64 autograd through the oracle."""
    from dvc_amd import synth
    from models.ContextualLoss import ContextualLoss_forward
    from oracle import contextual_oracle as CO
    from utils.util import tensor_lab2rgb, uncenter_l
    sd = synth.vgg19_state_dict(0)
    B, H, W = 2, 64, 112
    lab = torch.cat([synth.synth_lab(synth.FRAME_SEED0 + i, H, W) for i in range(B)])      # L centred
    L, ab0 = lab[:, 0:1], lab[:, 1:3] * 0.6
    ref_img = torch.cat([synth.synth_lab(synth.EXEMPLAR_SEED + i, H, W) for i in range(B)])
    ref_rgb = O.tensor_lab2rgb(torch.cat((O.uncenter_l(ref_img[:, 0:1]), ref_img[:, 1:3]), 1))
    m = _vgg()
    with torch.no_grad():
        A_r42, A_r52 = m(ref_rgb.cuda(), ["r42", "r52"])
        tgt_r52 = m(ref_rgb.flip(3).cuda(), ["r52"])[0]
    cx = ContextualLoss_forward()
    ab = ab0.cuda().requires_grad_(True)
    I_rgb = tensor_lab2rgb(torch.cat((uncenter_l(L.cuda()), ab), dim=1))
    pred_r22, pred_r32, pred_r42, pred_r52 = m(I_rgb, ["r22", "r32", "r42", "r52"], preprocess=True)
    loss = (cx(pred_r52, A_r52.detach()) * 8 + cx(pred_r42, A_r42.detach()) * 4).mean() + F.mse_loss(pred_r52, tgt_r52.detach())
    loss.backward()
    got = ab.grad.cpu().double()

    sd64 = {k: v.double() for k, v in sd.items()}
    ab64 = ab0.double().requires_grad_(True)
    rgb64 = O.tensor_lab2rgb(torch.cat((O.uncenter_l(L.double()), ab64), 1))
    p42, p52 = O.vgg19_forward(sd64, rgb64, ["r42", "r52"])
    loss64 = ((CO.contextual_loss_forward(p52, A_r52.cpu().double()) * 8 + CO.contextual_loss_forward(p42, A_r42.cpu().double()) * 4)
              .mean() + F.mse_loss(p52, tgt_r52.cpu().double()))
    loss64.backward()
    ref = ab64.grad
    l2, mx = VR.rel_errors(got, ref)
    print(f"training chain d ab: loss {loss.item():.6f} (float64 {loss64.item():.6f}); rel L2 {l2:.2e}, max-abs/max {mx:.2e}")
    assert abs(loss.item() - loss64.item()) <= 1e-4 * abs(loss64.item())
    assert ref.abs().max() > 0
    assert l2 <= 1e-3 and mx <= 1e-2, (l2, mx)


def test_guards():
    """Trainable VGG parameters with a grad-requiring input raise (no weight gradients); forward_gray keeps raising."""
    from dvc_amd import synth
    from models.NonlocalNet import VGG19_pytorch
    with contextlib.redirect_stdout(io.StringIO()):
        m = VGG19_pytorch()
    m.load_state_dict(synth.vgg19_state_dict(0))
    m.cuda()
    x = torch.rand(1, 3, 32, 48, device="cuda", requires_grad=True)
    with pytest.raises(NotImplementedError, match="freeze"):
        m(x, ["r12"])
    for p in m.parameters():
        p.requires_grad = False
    assert m(x, ["r12"])[0].requires_grad
    with pytest.raises(NotImplementedError):
        m.forward_gray(torch.rand(1, 1, 32, 48, device="cuda", requires_grad=True), ["r12"])
    with torch.no_grad():
        assert not m(x, ["r12"])[0].requires_grad


# ================================================================================================ kernel edges
# Branches of csrc/vgg_bwd.hip that the cases above do not execute, or execute only under an end-to-end bound.
@pytest.mark.parametrize("fold", [True, False], ids=["preprocess_fold", "plain"])
@pytest.mark.parametrize("N", [1, 3])
@pytest.mark.parametrize("H,W", [(216, 384), (45, 70), (16, 16), (1, 1), (17, 15)])
@pytest.mark.parametrize("C", [64, 8, 256])
def test_conv1_bwd_kernel_vs_float64(C, H, W, N, fold):
    """dvc_vgg_conv1_bwd alone against float64 F.conv2d: C = 64 (production) and the limits the entry point accepts, whole
    tiles, ragged tiles, one tile, one pixel; 2e-5 (576 fp32 terms in a fixed order: the direct engine's number), whole map,
    border ring and interior alike."""
    import bwd_audit as BA
    from dvc_amd import nets, ops
    from test_gpu_bwd_audit import report
    g = torch.Generator().manual_seed(C + 7 * H + W)
    w = torch.randn(C, 3, 3, 3, generator=g) / 27 ** 0.5
    dZ = torch.randn(N, C, H, W, generator=g)
    wt = nets.vgg_bwd_weight_conv1(w, preprocess=fold)
    assert tuple(wt.shape) == (3, C, 3, 3)
    if fold:
        assert torch.equal(wt, w.transpose(0, 1).flip(2, 3).flip(0) * 255.0)
    got = ops.vgg_conv1_bwd(dZ.cuda(), wt.cuda())
    rec = BA.audit_conv1_bwd(got.cpu(), dZ, wt, layer=f"edge C{C} N{N}")
    rec["secs"] = 0.0
    report(BA.line(rec, "conv1_bwd " + ("fold" if fold else "plain")))
    assert BA.violations(rec) == [], BA.line(rec)


def _act_inputs(seed, n):
    g = torch.Generator().manual_seed(seed)
    R = torch.relu(torch.randint(-2, 4, (n,), generator=g).float() * 0.5)
    return torch.randn(n, generator=g), torch.randn(n, generator=g), R


def test_act_bwd_grid_wrap_bit_exact_vs_aten():
    """More than 8192 blocks x 256 threads x 4 float4 pieces: the four-in-flight loop runs with every piece in range, then wraps
    the capped grid (one [7, 64, 216, 384] buffer), in place and out of place."""
    import bwd_audit as BA
    from dvc_amd import ops
    shape = (7, 64, 216, 384)
    n = 7 * 64 * 216 * 384
    assert n // 4 > 8192 * 256 * 4
    free, _ = torch.cuda.mem_get_info()
    if free < 5 * 4 * n:
        pytest.skip(f"the card has {free >> 20} MiB free; this case holds four {4 * n >> 20} MiB buffers")
    dX, gR, R = (t.view(shape) for t in _act_inputs(3, n))
    want = BA.ref_act_bwd(dX, gR, R)
    d, gg, r = dX.cuda(), gR.cuda(), R.cuda()
    assert torch.equal(ops.vgg_act_bwd(d, gg, r).cpu(), want)
    assert torch.equal(ops.vgg_act_bwd(d, gg, r, out=d).cpu(), want)
    assert torch.equal(ops.vgg_act_bwd(None, gg, r).cpu(), BA.ref_act_bwd(None, gR, R))


@pytest.mark.parametrize("n", [4096, 1003, 1, 5])
def test_act_bwd_scalar_path_bit_exact_vs_aten(n):
    """n % 4 != 0, and a 4-byte-offset view of each of dX, g, R and out in turn: the scalar kernel, the same bits."""
    import bwd_audit as BA
    from dvc_amd import ops
    dX, gR, R = _act_inputs(4, n)
    want = BA.ref_act_bwd(dX, gR, R)
    assert torch.equal(ops.vgg_act_bwd(dX.cuda(), gR.cuda(), R.cuda()).cpu(), want)

    def off(t):
        buf = torch.zeros(n + 8, device="cuda")
        v = buf[1:1 + n]
        v.copy_(t)
        assert v.data_ptr() % 16 == 4 and v.is_contiguous()
        return buf, v
    for which in range(4):
        args = [dX.cuda(), gR.cuda(), R.cuda(), torch.full((n,), 7.0, device="cuda")]
        buf, args[which] = off(args[which].cpu())
        out = ops.vgg_act_bwd(args[0], args[1], args[2], out=args[3])
        assert out is args[3] and torch.equal(out.cpu(), want), which
        if which == 3:
            assert buf[0] == 0 and bool((buf[1 + n:] == 0).all())       # nothing written around the view
    _, d = off(dX)
    assert torch.equal(ops.vgg_act_bwd(d, gR.cuda(), R.cuda(), out=d).cpu(), want)      # in place on the offset view


NAN, INF = float("nan"), float("inf")


@pytest.mark.parametrize("W", [8, 9])
def test_pool_act_bwd_nan_windows_bit_exact_vs_aten(W):
    """R with NaN in a window (one NaN, two NaNs, NaN beside +inf): ATen's scan `v > max || isnan(v)` gives the window to its LAST
    NaN (tests/test_bwd_audit_host.py shows this ATen doing so on the CPU); float2 (W = 8) and scalar (W = 9) paths."""
    import bwd_audit as BA
    from dvc_amd import ops
    g = torch.Generator().manual_seed(5)
    R = torch.relu(torch.randint(-2, 4, (2, 3, 6, W), generator=g).float() * 0.5)
    wins = [(1.0, NAN, 3.0, 2.0), (NAN, 1.0, NAN, 2.0), (1.0, NAN, 2.0, NAN), (NAN, INF, 0.5, 1.0), (INF, NAN, 0.5, 1.0),
            (NAN, NAN, NAN, NAN)]
    for i, wv in enumerate(wins):
        y, x = 2 * (i // 3), 2 * (i % 3)
        R[i % 2, i % 3, y:y + 2, x:x + 2] = torch.tensor(wv).view(2, 2)
    dP, gP = torch.randn(2, 3, 3, W // 2, generator=g), torch.randn(2, 3, 3, W // 2, generator=g)
    gR = torch.randn(R.shape, generator=g)
    for use in ((1, 1, 1), (1, 0, 0), (0, 1, 1)):
        a, b, c = (t if u else None for t, u in zip((dP, gP, gR), use))
        want = BA.ref_pool_act_bwd(a, b, c, R)
        assert torch.isfinite(want).all()
        cu = lambda t: None if t is None else t.cuda()
        got = ops.vgg_pool_act_bwd(cu(a), cu(b), cu(c), R.cuda())
        assert torch.equal(got.cpu(), want), (W, use, (got.cpu() - want).abs().max())


@pytest.mark.parametrize("pool", ["max", "avg"])
def test_pool_act_bwd_offset_base_takes_the_scalar_path(pool):
    """Even W with R (then gR) at a 4-byte offset from an 8-byte boundary: the scalar kernel, the same bits."""
    import bwd_audit as BA
    from dvc_amd import ops
    N, C, H, W = 2, 3, 6, 10
    z = _crafted(6, N, C, H, W)
    R = torch.relu(z)
    g = torch.Generator().manual_seed(7)
    dP, gR = torch.randn(N, C, H // 2, W // 2, generator=g), torch.randn(N, C, H, W, generator=g)
    want = BA.ref_pool_act_bwd(dP, None, gR, R, avg=pool == "avg")

    def off(t):
        v = torch.zeros(t.numel() + 3, device="cuda")[1:1 + t.numel()].view(t.shape)
        v.copy_(t)
        assert v.data_ptr() % 8 == 4
        return v
    for r, e in ((off(R), gR.cuda()), (R.cuda(), off(gR)), (off(R), off(gR))):
        assert torch.equal(ops.vgg_pool_act_bwd(dP.cuda(), None, e, r, avg=pool == "avg").cpu(), want)


@pytest.mark.parametrize("H,W", [(216, 384), (215, 384), (216, 383)])
def test_pool_act_bwd_grid_wrap_bit_exact_vs_aten(H, W):
    """More than 8192 blocks x 256 cells ([2, 64, 216, 384]): the capped grid wraps; odd H with even W and the reverse."""
    import bwd_audit as BA
    from dvc_amd import ops
    N, C = 2, 64
    assert N * C * ((H + 1) // 2) * ((W + 1) // 2) > 8192 * 256
    z = _crafted(8, N, C, H, W)
    R = torch.relu(z)
    g = torch.Generator().manual_seed(9)
    dP, gR = torch.randn(N, C, H // 2, W // 2, generator=g), torch.randn(N, C, H, W, generator=g)
    for pool in ("max", "avg"):
        want = BA.ref_pool_act_bwd(dP, None, gR, R, avg=pool == "avg")
        got = ops.vgg_pool_act_bwd(dP.cuda(), None, gR.cuda(), R.cuda(), avg=pool == "avg")
        assert torch.equal(got.cpu(), want), (pool, (got.cpu() - want).abs().max())
