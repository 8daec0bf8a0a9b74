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
# contractive set have more activations near a ReLU's kink, where fp32 and float64 masks part).  The plain seed-0 weights are
# chaotic over 31 layers (an fp32 rounding of the forward moves the float64 gradient by percent): not a yardstick here.
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
