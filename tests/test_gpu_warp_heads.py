"""GPU: WarpNet's training path through its four heads (WarpNet.set_head_training; dvc_amd/nets.py _WarpHeadsTrain,
csrc/warp_head_bwd.hip) — every new kernel alone against its float64 restatement (tests/warp_head_bwd_reference.py) on the
device's own inputs, all 43 gradients against float64 autograd through the oracle, forward bit-identity, frozen subsets,
reproducibility, frame_colorization, and the default (off).

Bounds.  Weight gradients (sums over positions): max(1e-6, 4 x the error of the float32 CPU restatement against float64) — the
rule of tests/bwd_audit.py.  The data-movement adjoints (dilate-ring, 2x2 block sums, replicated rows) are exact: torch.equal
against the restatement in float32.  End to end: per tensor max(1e-6, 4 x the float32 CPU oracle's error against the float64 oracle
on the same loss), the rule of tests/test_gpu_warp_backward.py, for the 24 head tensors as for the 19 behind the trunk, biases
over max |dW_ref| of their layer as there.  No head needs more than that rule (measured figures: DESIGN.md section 6d)."""
import contextlib
import functools
import io

import pytest
import torch
import torch.nn.functional as F

import warp_head_bwd_reference as RH
from bwd_audit import SUM_FLOOR, YARD_FACTOR, relerr
from test_gpu_warp_backward import (HEADS, _cotangents, _cpu_inputs, _frame_setup, _gpu_inputs, _make_warp, _rnd, _tensor_err,
                                    _threads, report)

pytestmark = pytest.mark.gpu

N, T = 2, 0.01
E2E_SIZES = [(48, 80), (40, 64)]      # 40 x 64: relu5_1 is 2 x 4 and layer5_1 gets one replicated row top and bottom


@pytest.fixture(scope="module")
def vgg():
    from dvc_amd import synth
    from models.NonlocalNet import VGG19_pytorch
    m = VGG19_pytorch()
    m.load_state_dict(synth.vgg19_state_dict(0))
    return m.eval().cuda()


def _make_heads_net(frozen=()):
    """WarpNet in training mode with head training on; `frozen`: top-level names (heads, "layer", "theta", "phi") to freeze."""
    net = _make_warp(freeze_heads=False).set_head_training(True)
    for n, p in net.named_parameters():
        if n.split(".")[0] in frozen:
            p.requires_grad = False
    return net


def _backward(net, ins, gy, gs):
    y, sim = net(*ins, temperature=T)
    assert y.requires_grad and sim.requires_grad
    ((y * gy).sum() + (sim * gs).sum()).backward()
    return {n: (None if p.grad is None else p.grad.clone()) for n, p in net.named_parameters()}, y.detach(), sim.detach()


# ================================================================================================ the kernels, one by one
@pytest.mark.parametrize("stride,Cin,Cout,H,W", [(2, 128, 64, 7, 9), (2, 128, 64, 8, 10), (1, 512, 256, 2, 3)])
def test_step_head_wgrad(stride, Cin, Cout, H, W):
    from dvc_amd import ops
    Ho, Wo = RH.out_hw(H, W, stride)
    dzr = F.pad(_rnd((N, Cout, Ho, Wo), 41), (1, 1, 1, 1)).cuda()
    xp = ops.warp_reflect_pad((_rnd((N, Cin, H, W), 42) + 0.1).cuda())
    dW, db = ops.warp_head_wgrad(dzr, xp, stride=stride)
    rW, rb = RH.head_wgrad(dzr.cpu().double(), xp.cpu().double(), stride)
    torch.set_num_threads(_threads())
    yW, yb = RH.head_wgrad(dzr.cpu(), xp.cpu(), stride)
    bW, bb = max(SUM_FLOOR, YARD_FACTOR * relerr(yW, rW)), max(SUM_FLOOR, YARD_FACTOR * relerr(yb, rb))
    eW, eb = relerr(dW.cpu(), rW), relerr(db.cpu(), rb)
    report(f"step head_wgrad s{stride} {Cin}->{Cout} {H}x{W}: dW {eW:.2e} (bound {bW:.2e}) db {eb:.2e} (bound {bb:.2e})")
    assert eW <= bW and eb <= bb
    # the restatement is the reflect-padded strided layer's gradient (closes the loop on the device result)
    w = torch.zeros(Cout, Cin, 3, 3, dtype=torch.float64, requires_grad=True)
    F.conv2d(xp.cpu().double(), w, stride=stride).backward(dzr.cpu().double()[:, :, 1:-1, 1:-1])
    assert relerr(rW, w.grad) <= 1e-12
    # one slot against the default slots: the same sums, to the same bound; two runs bit-identical
    S = ops.warp_head_wgrad_splits(N, Cin, Cout, H, W, stride)
    dW1, db1 = ops.warp_head_wgrad(dzr, xp, stride=stride, splits=1)
    report(f"  default splits {S}; splits=1 against default: dW {relerr(dW1.cpu(), dW.cpu()):.2e}")
    assert relerr(dW1.cpu(), rW) <= bW and relerr(db1.cpu(), rb) <= bb
    dW2, db2 = ops.warp_head_wgrad(dzr, xp, stride=stride)
    assert torch.equal(dW, dW2) and torch.equal(db, db2)


@pytest.mark.parametrize("stride,H,W", [(2, 7, 9), (2, 6, 35), (1, 5, 18)])
def test_step_head_wgrad_exact_integers_asymmetric(stride, H, W):
    """Small-integer data: every product and sum is exact in fp32, so a wrong tap, stride, tail or channel tile shows as a
    mismatch, not as rounding.  Channels that are no multiple of the 64-wide tile; more than one 16-column chunk per row."""
    from dvc_amd import ops
    g = torch.Generator().manual_seed(43)
    Ho, Wo = RH.out_hw(H, W, stride)
    dzr = F.pad(torch.randint(-3, 4, (N, 96, Ho, Wo), generator=g).float(), (1, 1, 1, 1)).cuda()
    xp = ops.warp_reflect_pad(torch.randint(-3, 4, (N, 130, H, W), generator=g).float().cuda())
    rW, rb = RH.head_wgrad(dzr.cpu().double(), xp.cpu().double(), stride)
    for splits in (None, 1, 3):
        dW, db = ops.warp_head_wgrad(dzr, xp, stride=stride, splits=splits)
        assert torch.equal(dW.cpu().double(), rW) and torch.equal(db.cpu().double(), rb), splits


@pytest.mark.parametrize("H,W", [(7, 9), (8, 10), (2, 3), (3, 2), (54, 95)])
def test_step_dilate_ring_is_exact(H, W):
    from dvc_amd import ops
    Ho, Wo = RH.out_hw(H, W, 2)
    C = 64 if H == 54 else 5
    dzr = F.pad(_rnd((3, C, Ho, Wo), 44), (1, 1, 1, 1))
    got = ops.warp_dilate_ring(dzr.cuda(), H, W).cpu()
    assert torch.equal(got, RH.dilate_ring(dzr, H, W))
    if H % 2 or W % 2:
        assert not torch.equal(got, RH.dilate_ring(dzr, H, W, defect="odd_tail"))


@pytest.mark.parametrize("h,w", [(5, 7), (1, 1), (27, 48)])
def test_step_up2_bwd_is_exact(h, w):
    from dvc_amd import ops
    g = _rnd((3, 64 if h == 27 else 5, 2 * h, 2 * w), 45)
    got = ops.warp_up2_bwd(g.cuda()).cpu()
    assert torch.equal(got, RH.up2_bwd(g))
    assert relerr(got, F.avg_pool2d(g.double(), 2) * 4) <= 1e-6
    if h > 1:
        assert not torch.equal(got, RH.up2_bwd(g, defect="block_index"))


@pytest.mark.parametrize("h,w,rpad", [(8, 16, 1), (1, 3, 1), (2, 5, 1), (3, 4, 2), (52, 96, 1)])
def test_step_rpad_rows_bwd_is_exact(h, w, rpad):
    from dvc_amd import ops
    g = _rnd((3, 64 if h == 52 else 5, h + 2 * rpad, w), 46)
    got = ops.warp_rpad_rows_bwd(g.cuda(), rpad).cpu()
    assert torch.equal(got, RH.rpad_rows_bwd(g, rpad))
    assert not torch.equal(got, RH.rpad_rows_bwd(g, rpad, defect="no_edge"))


# ================================================================================================ end to end vs float64
def _oracle_grads(sd, ins, gy, gs, dtype):
    """All 43 gradients of the loss through oracle.warpnet_forward; also the top-1 / top-2 gap of the affinities."""
    from oracle import dvc_oracle as O
    leaves = {k: v.detach().to(dtype).clone().requires_grad_() for k, v in sd.items()}
    taps = {}
    y, sim = O.warpnet_forward(leaves, *[t.to(dtype) for t in ins], temperature=T, taps=taps)
    ((y * gy.to(dtype)).sum() + (sim * gs.to(dtype)).sum()).backward()
    top2 = taps["top2"].detach()
    return {k: v.grad for k, v in leaves.items()}, (top2[..., 0] - top2[..., 1]).min().item()


@functools.lru_cache(maxsize=None)
def _truth(H, W):
    """Computed once per size and shared: inputs, cotangents, the float64 gradients and the float32 CPU yardstick."""
    from dvc_amd import synth
    torch.set_num_threads(_threads())
    ins = _cpu_inputs(H, W, N, 0)
    sd = synth.warpnet_state_dict(0)
    gy, gs = _cotangents(torch.empty(N, 3, H, W), torch.empty(N, 1, H, W))
    ref, gap = _oracle_grads(sd, ins, gy, gs, torch.float64)
    yard, _ = _oracle_grads(sd, ins, gy, gs, torch.float32)
    return ins, sd, gy, gs, ref, yard, gap


@pytest.mark.parametrize("H,W", E2E_SIZES)
def test_end_to_end_all_43_gradients_against_float64_autograd(H, W):
    """N = 2, T = 0.01, loss = random cotangents on y and on the similarity map.

    Measured on the MI355X (error / bound, worst tensor per size): see DESIGN.md section 6d."""
    ins, sd, gy, gs, ref, yard, gap = _truth(H, W)
    report(f"e2e heads {H}x{W}: smallest top-1 / top-2 gap of the float64 affinities {gap:.3e}")
    assert gap > 1e-5, "pick another seed: an fp32 arg-max may differ from the float64 one"
    net = _make_heads_net()
    got, _, _ = _backward(net, [t.cuda() for t in ins], gy.cuda(), gs.cuda())
    assert len(got) == 43 and all(g is not None for g in got.values())
    bad = []
    for name in got:
        e_y, e = _tensor_err(name, yard[name], ref[name], ref), _tensor_err(name, got[name].cpu(), ref[name], ref)
        bound = max(1e-6, YARD_FACTOR * e_y)
        report(f"e2e heads {H}x{W} {name:24s} hip {e:.3e}  float32 CPU oracle {e_y:.3e}  bound {bound:.3e}")
        if not e <= bound:
            bad.append((name, e, bound))
    assert not bad, bad


# ================================================================================================ forward bit-identity
@pytest.mark.parametrize("algo", ["auto", "direct"])
@pytest.mark.parametrize("group", [True, False])
@pytest.mark.parametrize("H,W", E2E_SIZES)
def test_forward_bit_identical_to_no_grad(vgg, H, W, group, algo):
    from dvc_amd import ops
    prev = ops.conv_algo(), ops.group_heads()
    ops.set_conv_algo(algo)
    ops.set_group_heads(group)
    try:
        net = _make_heads_net()
        ins = _gpu_inputs(vgg, H, W, N)
        y, sim = net(*ins, temperature=T)
        assert y.requires_grad and sim.requires_grad
        with torch.no_grad():
            y0, s0 = net(*ins, temperature=T)
        assert not y0.requires_grad
        assert torch.equal(y, y0) and torch.equal(sim, s0), (H, W, group, algo)
        # one head with history, three without: the same bits
        part = _make_heads_net(frozen=("layer2_1", "layer4_1", "layer5_1", "layer", "theta", "phi"))
        y1, s1 = part(*ins, temperature=T)
        assert y1.requires_grad and torch.equal(y1, y0) and torch.equal(s1, s0)
    finally:
        ops.set_conv_algo(prev[0])
        ops.set_group_heads(prev[1])


# ================================================================================================ subsets, reproducibility
@pytest.fixture(scope="module")
def full_run(vgg):
    """The all-43 run at 48 x 80 the subset and reproducibility tests compare with: (inputs, cotangents, gradients)."""
    ins = _gpu_inputs(vgg, 48, 80, N)
    gy, gs = (t.cuda() for t in _cotangents(torch.empty(N, 3, 48, 80), torch.empty(N, 1, 48, 80)))
    grads, _, _ = _backward(_make_heads_net(), ins, gy, gs)
    return ins, gy, gs, grads


def test_two_identical_calls_give_identical_gradients(full_run):
    ins, gy, gs, grads = full_run
    again, _, _ = _backward(_make_heads_net(), ins, gy, gs)
    for n, g in grads.items():
        assert g is not None and torch.isfinite(g).all() and g.abs().max().item() > 0, n
        assert torch.equal(g, again[n]), n


def test_heads_only_with_the_trunk_frozen(full_run):
    ins, gy, gs, grads = full_run
    net = _make_heads_net(frozen=("layer", "theta", "phi"))
    assert net._takes_training_path()
    got, _, _ = _backward(net, ins, gy, gs)
    for n, g in got.items():
        if n.split(".")[0] in HEADS:
            assert torch.equal(g, grads[n]), n
        else:
            assert g is None, n


def test_one_head_frozen_gets_no_gradient_and_changes_no_other(full_run):
    ins, gy, gs, grads = full_run
    got, _, _ = _backward(_make_heads_net(frozen=("layer3_1",)), ins, gy, gs)
    for n, g in got.items():
        if n.startswith("layer3_1."):
            assert g is None, n
        else:
            assert torch.equal(g, grads[n]), n
    # a single parameter inside a head
    net = _make_heads_net()
    for n, p in net.named_parameters():
        p.requires_grad = n == "layer2_1.3.weight"
    got, _, _ = _backward(net, ins, gy, gs)
    for n, g in got.items():
        assert (g is not None) == (n == "layer2_1.3.weight"), n
    assert torch.equal(got["layer2_1.3.weight"], grads["layer2_1.3.weight"])


# ================================================================================================ guards, default off
def test_default_off_still_refuses_and_inputs_stay_data(vgg):
    ins = _gpu_inputs(vgg, 48, 80, 1)
    with pytest.raises(NotImplementedError, match="freeze"):
        _make_warp(freeze_heads=False)(*ins)
    net = _make_heads_net()
    x = [t.clone() for t in ins]
    x[2].requires_grad_()
    with pytest.raises(NotImplementedError, match="input requires grad"):
        net(*x)
    cache = net.exemplar_side(ins[0], *ins[5:9])
    for kw in (dict(exemplar_cache=cache), dict(return_taps=True), dict(detach_flag=True), dict(defer_merge=True)):
        with pytest.raises(NotImplementedError):
            net(*ins, **kw)
    net.set_head_training(False)
    with pytest.raises(NotImplementedError, match="freeze"):
        net(*ins)


# ================================================================================================ frame_colorization
def test_frame_colorization_fills_all_108_gradients(vgg):
    from dvc_amd.frame import frame_colorization
    from models.ColorVidNet import ColorVidNet
    from oracle import dvc_oracle as O
    H, W = 48, 80
    sds, IA, IB, last, g = _frame_setup(H, W, 1)
    with contextlib.redirect_stdout(io.StringIO()):
        cvn = ColorVidNet(7)
    cvn.load_state_dict(sds[2])
    cvn.train().cuda()
    warp = _make_heads_net()
    for p in vgg.parameters():
        p.requires_grad = False
    dIA, dIB, dlast = IA.cuda(), IB.cuda(), last.cuda()
    with torch.no_grad():
        fB = vgg(O.tensor_lab2rgb(torch.cat((O.uncenter_l(IB[:, 0:1]), IB[:, 1:3]), dim=1)).cuda(), O.VGG_OUT, preprocess=True)
        ab0, warped0, _ = frame_colorization(dIA, dIB, dlast, fB, vgg, warp, cvn, temperature=T)
    ab, warped, _ = frame_colorization(dIA, dIB, dlast, fB, vgg, warp, cvn, temperature=T)
    assert ab.requires_grad and torch.equal(ab, ab0) and torch.equal(warped, warped0)
    (ab * g.cuda()).sum().backward()
    params = list(cvn.named_parameters()) + list(warp.named_parameters())
    assert len(params) == 65 + 43
    for n, p in params:
        assert p.grad is not None and torch.isfinite(p.grad).all(), n
