"""GPU: ColorVidNet's training path — outputs bit-identical to the no-grad forward, every parameter gradient and d x against
float64 CPU autograd through the oracle, each new kernel (csrc/cvn_bwd.hip) alone against float64, determinism, guards, and
the inference drivers staying on the no-grad path."""
import contextlib
import io

import pytest
import torch
import torch.nn.functional as F

from oracle import dvc_oracle as O

pytestmark = pytest.mark.gpu


def _net(contractive=False, train=True):
    from dvc_amd import synth
    from models.ColorVidNet import ColorVidNet
    with contextlib.redirect_stdout(io.StringIO()):
        m = ColorVidNet(7)
    m.load_state_dict(synth.colorvidnet_state_dict(0, contractive=contractive))
    m = m.cuda()
    return m.train() if train else m.eval()


def _x(seed, B, H, W):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(B, 7, H, W, generator=g) * 2 - 1) * 50


def _g(seed, shape):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(shape, generator=g)


def _rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-300))


def _ref_grads(sd, x, g):
    sd64 = {k: v.double().clone().requires_grad_(True) for k, v in sd.items()}
    x64 = x.double().clone().requires_grad_(True)
    out = O.colorvidnet_forward(sd64, x64)
    out.backward(g.double())
    return out.detach(), x64.grad, {k: v.grad for k, v in sd64.items()}


@pytest.mark.parametrize("algo", ["default", "direct"])
@pytest.mark.parametrize("hw", [(48, 80), (64, 96), (216, 384)])
def test_training_output_bit_identical(hw, algo):
    from dvc_amd import ops
    m = _net()
    x = _x(1, 1, *hw).cuda()
    prev = ops.conv_algo()
    try:
        if algo == "direct":
            ops.set_conv_algo("direct")
        with torch.no_grad():
            ref = m(x)
        y = m(x.clone().requires_grad_(True))
        assert y.requires_grad
        assert torch.equal(y.detach(), ref)
    finally:
        ops.set_conv_algo(prev)


# bounds at about twice the measured worst tensor (MI355X: 2.4e-6 at 48x80, 5.5e-4 at 216x384 — the larger maps of the
# contractive set have more activations near a ReLU's kink, where fp32 and float64 masks part).  The 1e-3 at 216x384 is a
# measure of the CHAIN's conditioning over 31 layers, not of the kernels: tests/test_gpu_bwd_audit.py holds every single launch
# of the same backward, at that size and with both weight sets, to the engines' own 2e-5 / 5e-5 and to float32-CPU yardsticks,
# and this 48x80 case at 1e-5 pins the wiring between the launches (which does not depend on the size).  The plain seed-0
# weights are chaotic over 31 layers (an fp32 rounding of the forward moves the float64 gradient by percent), so they are not
# compared end to end; the audit covers every launch on them.
@pytest.mark.parametrize("B,H,W,contractive,bound", [(2, 48, 80, True, 1e-5), (1, 216, 384, True, 1e-3)])
def test_gradients_vs_float64(B, H, W, contractive, bound):
    from dvc_amd import synth
    sd = synth.colorvidnet_state_dict(0, contractive=contractive)
    m = _net(contractive)
    x = _x(2, B, H, W)
    g = _g(3, (B, 2, H, W))
    xg = x.cuda().requires_grad_(True)
    y = m(xg)
    y.backward(g.cuda())
    _, dx_ref, gref = _ref_grads(sd, x, g)
    worst = []
    named = dict(m.named_parameters())
    assert set(named) == set(sd)
    for k, p in named.items():
        assert p.grad is not None, k
        e = _rel(p.grad, gref[k])
        worst.append((e, k, float((p.grad.double().cpu() - gref[k]).abs().max())))
    worst.append((_rel(xg.grad, dx_ref), "x", float((xg.grad.double().cpu() - dx_ref).abs().max())))
    worst.sort(reverse=True)
    print("worst rel L2 / max abs:", worst[:5])
    assert worst[0][0] <= bound, worst[:5]


@pytest.mark.parametrize("dil,in_up", [(1, 1), (2, 1), (1, 2)])
@pytest.mark.parametrize("Cin,Cout,H,W", [(7, 32, 21, 37), (64, 128, 16, 24), (512, 512, 9, 15), (96, 64, 14, 34)])
@pytest.mark.parametrize("splits", [1, None, 7])
def test_wgrad_kernel_vs_float64(dil, in_up, Cin, Cout, H, W, splits):
    from dvc_amd import ops
    if in_up == 2 and (H % 2 or W % 2):
        H, W = H + H % 2, W + W % 2
    B = 2
    X = _g(4, (B, Cin, H // in_up, W // in_up))
    dZ = _g(5, (B, Cout, H, W))
    dW, db = ops.cvn_wgrad(dZ.cuda(), X.cuda(), dil=dil, in_up=in_up, splits=splits)
    Xf = X.double().repeat_interleave(in_up, 2).repeat_interleave(in_up, 3) if in_up == 2 else X.double()
    ref = torch.nn.grad.conv2d_weight(Xf, (Cout, Cin, 3, 3), dZ.double(), padding=dil, dilation=dil)
    assert _rel(dW, ref) < 1e-6, _rel(dW, ref)
    assert _rel(db, dZ.double().sum((0, 2, 3))) < 1e-5      # (a plain fp32 sum over every position)


def test_head_bwd_kernel_vs_float64():
    from dvc_amd import ops
    B, C, H, W = 2, 128, 19, 45
    R = _g(6, (B, C, H, W))
    R = torch.where(R > 0, R, 0.2 * R)
    w = _g(7, (2, C)) * 0.1
    bias = _g(8, (2,))
    ab = (torch.tanh(torch.einsum("oc,bchw->bohw", w, R) + bias.view(1, 2, 1, 1)) * 128).contiguous()
    g = _g(9, (B, 2, H, W))
    dZ, dW, db = ops.cvn_head_bwd(ab.cuda(), g.cuda(), w.cuda().contiguous(), R.cuda(), slope=0.2)
    dpre = g.double() * 128 * (1 - (ab.double() / 128) ** 2)
    dR = torch.einsum("oc,bohw->bchw", w.double(), dpre)
    dZ_ref = dR * torch.where(R > 0, 1.0, 0.2).double()
    assert _rel(dZ, dZ_ref) < 1e-6
    assert _rel(dW.view(2, C), torch.einsum("bohw,bchw->oc", dpre, R.double())) < 1e-6
    assert _rel(db, dpre.sum((0, 2, 3))) < 1e-6


@pytest.mark.parametrize("kinds", [("full",), ("ss",), ("up",), ("full", "ss"), ("full", "ss", "up")])
@pytest.mark.parametrize("H,W", [(27, 48), (13, 7)])
def test_inorm_bwd_kernel_vs_float64(kinds, H, W):
    from dvc_amd import ops
    B, C = 2, 16
    a = torch.relu(_g(10, (B, C, H, W)) + 0.3).double().requires_grad_(True)
    ssw = _g(11, (C,)).double().requires_grad_(True)
    n = F.instance_norm(a, eps=1e-5)
    gf, gs, gu = _g(12, (B, C, H, W)), _g(13, (B, C, (H + 1) // 2, (W + 1) // 2)), _g(14, (B, C, 2 * H, 2 * W))
    loss = 0
    if "full" in kinds:
        loss = loss + (n * gf.double()).sum()
    if "ss" in kinds:
        loss = loss + (n[:, :, ::2, ::2] * ssw.view(1, C, 1, 1) * gs.double()).sum()
    if "up" in kinds:
        loss = loss + (n.repeat_interleave(2, 2).repeat_interleave(2, 3) * gu.double()).sum()
    loss.backward()
    var = a.detach().var((2, 3), unbiased=False)
    rstd = (1 / torch.sqrt(var + 1e-5)).float().reshape(-1)
    dZ, dss = ops.cvn_inorm_bwd(n.detach().float().cuda(), rstd.cuda(), a.detach().float().cuda(),
                                g_full=gf.cuda() if "full" in kinds else None, g_ss=gs.cuda() if "ss" in kinds else None,
                                ss_w=ssw.detach().float().cuda() if "ss" in kinds else None,
                                g_up=gu.cuda() if "up" in kinds else None)
    ref = a.grad * (a.detach() > 0)
    assert _rel(dZ, ref) < 1e-5, _rel(dZ, ref)
    if "ss" in kinds:
        assert _rel(dss, ssw.grad) < 1e-5
    else:
        assert dss is None


def test_backward_deterministic_and_accumulates():
    m = _net(True)
    x = _x(15, 1, 64, 96).cuda()
    g = _g(16, (1, 2, 64, 96)).cuda()
    grads = []
    for _ in range(2):
        m.zero_grad(set_to_none=True)
        m(x).backward(g)
        grads.append({k: p.grad.clone() for k, p in m.named_parameters()})
    for k in grads[0]:
        assert torch.equal(grads[0][k], grads[1][k]), k
    m(x).backward(g)            # .grad accumulates over a second backward
    for k, p in m.named_parameters():
        assert torch.equal(p.grad, grads[1][k] + grads[1][k]), k


def test_frozen_parameters_get_no_grad():
    m = _net(True)
    frozen = {"conv1_1.0.weight", "conv5_2.bias", "conv2_2norm_ss.weight", "conv10_ab.weight"}
    for k, p in m.named_parameters():
        p.requires_grad = k not in frozen
    m(_x(17, 1, 48, 80).cuda()).sum().backward()
    for k, p in m.named_parameters():
        assert (p.grad is None) == (k in frozen), k


def _three_nets(train_col):
    from dvc_amd import synth
    from models.ColorVidNet import ColorVidNet
    from models.NonlocalNet import VGG19_pytorch, WarpNet
    with contextlib.redirect_stdout(io.StringIO()):
        vgg, warp, col = VGG19_pytorch(), WarpNet(1), ColorVidNet(7)
    for m, sd in zip((vgg, warp, col), (synth.vgg19_state_dict(0), synth.warpnet_state_dict(0),
                                        synth.colorvidnet_state_dict(0, contractive=True))):
        m.load_state_dict(sd)
        m.cuda().eval()
    for p in vgg.parameters():
        p.requires_grad = False
    if train_col:
        col.train()
    return vgg, warp, col


def test_frame_colorization_train_mode_matches_direct_call():
    from dvc_amd import ops, synth
    from dvc_amd.frame import frame_colorization
    H, W = 216, 384
    vgg, warp, col = _three_nets(True)
    IA = synth.synth_lab(3, H, W).cuda()
    IB = synth.synth_lab(4, H, W).cuda()
    last = torch.zeros_like(IA)
    with torch.no_grad():
        fB = vgg(ops.lab2rgb(IB), ["r12", "r22", "r32", "r42", "r52"], preprocess=True)
    ab, nl, _ = frame_colorization(IA, IB, last, fB, vgg, warp, col, feature_noise=0, temperature=0.01)
    assert ab.requires_grad
    g = _g(18, ab.shape).cuda()
    ab.backward(g)
    via_frame = {k: p.grad.clone() for k, p in col.named_parameters()}
    col.zero_grad(set_to_none=True)
    # the same packed input, rebuilt the way frame_colorization builds it, in a no-grad pass
    with torch.no_grad():
        from dvc_amd.frame import warp_color
        fold = ops.fold_merge()
        w_, s_, _ = warp_color(IA[:, 0:1], IB, fB, vgg, warp, col, 0, temperature=0.01, defer_merge=fold)
        cin, _ = ops.pack_color_input(IA, w_, s_, last, want_warped=True)
    y = col(cin)
    assert torch.equal(y.detach(), ab.detach())
    y.backward(g)
    for k, p in col.named_parameters():
        assert torch.equal(p.grad, via_frame[k]), k


def test_sgd_steps_reduce_loss_and_track_float64():
    from dvc_amd import synth
    sd = synth.colorvidnet_state_dict(0, contractive=True)
    m = _net(True)
    x = _x(19, 1, 64, 96)
    target = _g(20, (1, 2, 64, 96)) * 20
    lr = 1e-6
    sd64 = {k: v.double().clone().requires_grad_(True) for k, v in sd.items()}
    named = dict(m.named_parameters())
    losses = []
    for _ in range(20):
        m.zero_grad(set_to_none=True)
        loss = (m(x.cuda()) - target.cuda()).abs().mean()
        loss.backward()
        losses.append(float(loss.detach()))
        with torch.no_grad():
            for p in m.parameters():
                p -= lr * p.grad
        l64 = (O.colorvidnet_forward(sd64, x.double()) - target.double()).abs().mean()
        gr = torch.autograd.grad(l64, list(sd64.values()))
        with torch.no_grad():
            for (k, v), gk in zip(sd64.items(), gr):
                v -= lr * gk
    assert losses[-1] < losses[0], losses
    for k, v in sd64.items():
        e = _rel(named[k].detach(), v.detach())
        assert e < 1e-5, (k, e)


def test_clip_colorizer_stays_inference_with_train_mode_module():
    from dvc_amd import synth
    from dvc_amd.frame import ClipColorizer
    H, W = 216, 384
    frames = [synth.synth_lab(s, H, W).cuda() for s in (5, 6, 7)]
    IB = synth.synth_lab(8, H, W).cuda()
    outs = []
    for train in (False, True):
        vgg, warp, col = _three_nets(train)
        cc = ClipColorizer(vgg, warp, col, temperature=1e-10, graph=True)
        cc.set_exemplar(IB)
        got = cc.clip(frames, lookahead=1)
        torch.cuda.synchronize()
        assert not any(t.requires_grad for t in got)
        outs.append(got)
    for a, b in zip(*outs):
        assert torch.equal(a, b)


def test_eval_mode_grad_input_still_raises():
    m = _net(train=False)
    with pytest.raises(NotImplementedError, match="training mode"):
        m(_x(21, 1, 48, 80).cuda().requires_grad_(True))


def test_double_backward_refused():
    m = _net(True)
    y = m(_x(22, 1, 48, 80).cuda())
    gx = torch.autograd.grad(y.sum(), m.conv10_ab.weight, create_graph=True)[0]
    with pytest.raises(RuntimeError):
        gx.sum().backward()


# ================================================================================================ kernel edges
# Branches of csrc/cvn_bwd.hip that the cases above do not execute, each alone against float64 with the audit's measures
# (tests/bwd_audit.py: whole tensor, per filter tap, worst output channel; bound max(1e-6, 4 x the same sum by float32 CPU
# ATen), the rule test_gpu_bwd_audit.py applies to every launch of a real backward).
def _audit_line(rec, case):
    import bwd_audit as BA
    from test_gpu_bwd_audit import report
    rec["secs"] = 0.0
    report(BA.line(rec, case))
    assert BA.violations(rec) == [], BA.line(rec, case)


WGRAD_EDGES = [
    # N, Cin, Cout, H, W, dil, in_up, splits
    (2, 16, 24, 6, 16, 1, 1, None), (2, 16, 24, 6, 32, 2, 1, 3), (2, 16, 24, 6, 48, 1, 2, None),    # W % 16 == 0: no ragged chunk
    (2, 16, 24, 5, 3, 2, 1, 1), (2, 16, 24, 4, 2, 2, 2, None), (1, 8, 8, 7, 5, 2, 1, 2),              # window wider than the row
    (1, 24, 16, 9, 21, 1, 1, None), (3, 24, 16, 9, 21, 2, 1, None), (3, 24, 16, 8, 22, 1, 2, 5),      # N = 1, N = 3
    (1, 8, 16, 2, 5, 1, 1, 64), (1, 8, 16, 2, 5, 2, 1, 64),                                          # more slots than chunks
    (2, 96, 40, 11, 19, 1, 1, None), (2, 96, 40, 11, 19, 2, 1, 4), (1, 70, 130, 6, 18, 1, 2, None),   # both tiles ragged
]


@pytest.mark.parametrize("N,Cin,Cout,H,W,dil,in_up,splits", WGRAD_EDGES)
def test_wgrad_kernel_edges(N, Cin, Cout, H, W, dil, in_up, splits):
    import bwd_audit as BA
    from dvc_amd import ops
    X = _g(30, (N, Cin, H // in_up, W // in_up))
    dZ = _g(31, (N, Cout, H, W))
    dW, db = ops.cvn_wgrad(dZ.cuda(), X.cuda(), dil=dil, in_up=in_up, splits=splits)
    _audit_line(BA.audit_wgrad(dW.cpu(), db.cpu(), dZ, X, dil, in_up, layer=f"edge {Cin}->{Cout}"), f"wgrad N{N} S={splits}")
    if splits == 64:        # nchunks = 2: every slot but two has an empty range and must contribute exact zeros
        one = ops.cvn_wgrad(dZ.cuda(), X.cuda(), dil=dil, in_up=in_up, splits=2)
        assert torch.equal(one[0], dW) and torch.equal(one[1], db)


@pytest.mark.parametrize("N,Cin,Cout,H,W,dil,in_up", [
    (1, 64, 64, 216, 384, 1, 1),        # wgrad_kernel<1, 1> (conv1_2)
    (1, 512, 512, 27, 48, 2, 1),        # wgrad_kernel<2, 1> (conv5_x, conv6_x)
    (1, 256, 128, 108, 192, 1, 2),      # wgrad_kernel<1, 2> (conv9_1.1)
])
def test_wgrad_kernel_production_shapes(N, Cin, Cout, H, W, dil, in_up):
    """One production shape per template instance the network uses, with the default slot count (512 slots over 5184 chunks
    for 64 -> 64 at 216x384), twice: bit-identical."""
    import bwd_audit as BA
    from dvc_amd import ops
    X = _g(32, (N, Cin, H // in_up, W // in_up))
    dZ = _g(33, (N, Cout, H, W))
    S = ops.cvn_wgrad_splits(N, Cin, Cout, H, W)
    dW, db = ops.cvn_wgrad(dZ.cuda(), X.cuda(), dil=dil, in_up=in_up)
    again = ops.cvn_wgrad(dZ.cuda(), X.cuda(), dil=dil, in_up=in_up)
    assert torch.equal(again[0], dW) and torch.equal(again[1], db)
    _audit_line(BA.audit_wgrad(dW.cpu(), db.cpu(), dZ, X, dil, in_up, layer=f"production {Cin}->{Cout}"), f"wgrad {H}x{W} S={S}")


@pytest.mark.parametrize("B,C,H,W", [
    (2, 16, 16, 16), (1, 16, 32, 48),       # HW an exact multiple of 256: no ragged block
    (2, 16, 5, 7), (1, 8, 1, 1),            # HW < 256: one partial block
    (2, 6, 9, 31), (1, 130, 11, 25),        # C % 4 != 0 (waves take channels w, w + 4, ...)
    (1, 128, 216, 384),                     # the production shape
])
def test_head_bwd_kernel_edges(B, C, H, W):
    import bwd_audit as BA
    from dvc_amd import ops
    R = F.leaky_relu(_g(34, (B, C, H, W)), 0.2)
    w = _g(35, (2, C)) * (0.1 if C > 8 else 0.3)
    bias = _g(36, (2,))
    ab = (torch.tanh(torch.einsum("oc,bchw->bohw", w, R) + bias.view(1, 2, 1, 1)) * 128).contiguous()
    g = _g(37, (B, 2, H, W))
    got = ops.cvn_head_bwd(ab.cuda(), g.cuda(), w.cuda().contiguous(), R.cuda(), slope=0.2)
    _audit_line(BA.audit_head(tuple(t.cpu() for t in got), ab, g, w, R, 0.2), f"head B{B}")


@pytest.mark.parametrize("B,C,H,W,kinds", [
    (2, 5, 3, 5, ("full", "ss", "up")), (1, 3, 3, 5, ("ss",)), (1, 4, 2, 3, ("full", "up")),     # a plane below one pass of 512
    (1, 3, 16, 32, ("up",)),                                                                          # exactly one pass
    (1, 64, 216, 384, ("full", "ss", "up")),                                                          # a production plane
])
def test_inorm_bwd_kernel_edges(B, C, H, W, kinds):
    import bwd_audit as BA
    from dvc_amd import ops
    a = torch.relu(_g(38, (B, C, H, W)) + 0.3)
    n = F.instance_norm(a.double(), eps=1e-5).float()
    rstd = (1 / torch.sqrt(a.double().var((2, 3), unbiased=False) + 1e-5)).float().reshape(-1)
    gf = _g(39, (B, C, H, W)) if "full" in kinds else None
    gs = _g(40, (B, C, (H + 1) // 2, (W + 1) // 2)) if "ss" in kinds else None
    ssw = _g(41, (C,)) if "ss" in kinds else None
    gu = _g(42, (B, C, 2 * H, 2 * W)) if "up" in kinds else None
    cu = lambda t: None if t is None else t.cuda()
    dZ, dss = ops.cvn_inorm_bwd(cu(n), cu(rstd), cu(a), g_full=cu(gf), g_ss=cu(gs), ss_w=cu(ssw), g_up=cu(gu))
    _audit_line(BA.audit_inorm(dZ.cpu(), None if dss is None else dss.cpu(), n, rstd, a, gf, gs, ssw, gu, layer=f"edge C{C}"),
                f"inorm B{B}")


def test_wgrad_bias_sum_at_production_size():
    """db over 2 x 216 x 384 positions and 512 slots with dZ = 1 + noise (every slot's sum positive: no cancellation to hide
    behind).  The kernel keeps the bias sum of a slot and the sum over slots in double and rounds each once to fp32: two
    roundings of at most 2^-24 = 6e-8 relative each, 1.2e-7 in the worst case; the bound is twice that, 2.5e-7.  The fp32 chains this
    replaced (160-term chains per slot, then 512 slots in sequence) give 1e-6 here and put the bias gradients of conv1_1.0 /
    conv1_1.2 over the audit's bound at 216x384 (test_gpu_bwd_audit.py)."""
    import bwd_audit as BA
    from dvc_amd import ops
    N, Cin, Cout, H, W = 2, 8, 64, 216, 384
    assert ops.cvn_wgrad_splits(N, Cin, Cout, H, W) == 512
    dZ = _g(43, (N, Cout, H, W)) + 1.0
    X = _g(44, (N, Cin, H, W))
    dW, db = ops.cvn_wgrad(dZ.cuda(), X.cuda())
    e = BA.relerr(db.cpu(), dZ.double().sum((0, 2, 3)))
    print(f"db at 2x216x384, 512 slots: relerr {e:.2e}")
    assert e <= 2.5e-7, e
    _audit_line(BA.audit_wgrad(dW.cpu(), db.cpu(), dZ, X, 1, 1, layer="bias 8->64"), "wgrad bias sum")
