"""GPU: WarpNet's training path behind the trunk tensor (dvc_amd/nets.py _WarpTrain, csrc/warp_bwd.hip) — forward bit-identity,
every new kernel alone against its float64 restatement (tests/warp_bwd_reference.py), the whole chain against float64 autograd
through the oracle, determinism and the guards.

Bounds.  Elementwise / per-plane steps: 1e-6.  Sums over positions: max(1e-6, 4 x the error of the same step by float32 CPU
ATen against float64) (tests/bwd_audit.py's rule).  3x3 input gradients: the engines' 2e-5 (direct) / 5e-5 (Winograd).  End to
end: per tensor max(1e-6, 4 x the float32 CPU oracle's error against the float64 oracle on the same loss), figure = max-abs error
over max-abs of the reference.  One measure needs a denominator of its own: all eight biases here have a true gradient of
exactly 0 — the six 3x3 biases sit in front of an InstanceNorm, which removes the plane mean, and theta.bias / phi.bias in front of
the centring over positions — so what any implementation returns is the rounding residue of a cancelling sum (the float64 oracle
gives 1e-13 where the weight gradients are 1e+2).  Its scale is that of the sum's terms, i.e. of the same layer's dW (the same dz
summed against inputs of unit order), so a bias error is taken over max |dW_ref| of that layer — for the HIP path and for the
yardstick alike."""
import contextlib
import io
import os

import pytest
import torch
import torch.nn.functional as F

import warp_bwd_reference as R
from bwd_audit import DGRAD_BOUND, SUM_FLOOR, YARD_FACTOR, map_measures, relerr

pytestmark = pytest.mark.gpu

HEADS = ("layer2_1", "layer3_1", "layer4_1", "layer5_1")
ELEM = 1e-6


def report(line):
    """Every measured figure is printed before it is asserted (pytest -s, or the captured output of a failure)."""
    print(line)


def _threads():
    try:
        avail = len(os.sched_getaffinity(0))
    except AttributeError:
        avail = os.cpu_count() or 1
    return max(1, min(16, avail))


def _make_warp(train=True, freeze_heads=True):
    from dvc_amd import synth
    from models.NonlocalNet import WarpNet
    net = WarpNet(1)
    net.load_state_dict(synth.warpnet_state_dict(0))
    if freeze_heads:
        for h in HEADS:
            for p in getattr(net, h).parameters():
                p.requires_grad = False
    return (net.train() if train else net.eval()).cuda()


@pytest.fixture(scope="module")
def vgg():
    from dvc_amd import synth
    from models.NonlocalNet import VGG19_pytorch
    m = VGG19_pytorch()
    m.load_state_dict(synth.vgg19_state_dict(0))
    return m.eval().cuda()


def _gpu_inputs(vgg, H, W, N, seed=0):
    """(B_lab_map, 4 normalised A features, 4 normalised B features) on the device, from this library's VGG19."""
    from dvc_amd import ops, synth
    from oracle import dvc_oracle as O
    with torch.no_grad():
        A = torch.cat([synth.synth_lab(1000 + seed + k, H, W) for k in range(N)])
        B = torch.cat([synth.synth_lab(2 + seed + 7 * k, H, W) for k in range(N)])
        fA = vgg(O.gray2rgb_batch(A[:, 0:1]).cuda(), O.VGG_OUT[1:], preprocess=True)
        fB = vgg(O.gray2rgb_batch(B[:, 0:1]).cuda(), O.VGG_OUT[1:], preprocess=True)
        return [B.cuda()] + [ops.channel_l2norm(t) for t in fA] + [ops.channel_l2norm(t) for t in fB]


def _cpu_inputs(H, W, N, seed=0):
    from dvc_amd import synth
    from oracle import dvc_oracle as O
    sd_v = synth.vgg19_state_dict(0)
    with torch.no_grad():
        A = torch.cat([synth.synth_lab(1000 + seed + k, H, W) for k in range(N)])
        B = torch.cat([synth.synth_lab(2 + seed + 7 * k, H, W) for k in range(N)])
        fA = O.vgg19_forward(sd_v, O.gray2rgb_batch(A[:, 0:1]), O.VGG_OUT)[1:]
        fB = O.vgg19_forward(sd_v, O.gray2rgb_batch(B[:, 0:1]), O.VGG_OUT)[1:]
        return [B] + [O.feature_normalize(t) for t in fA] + [O.feature_normalize(t) for t in fB]


def _trunk_params(net):
    return dict(net._trunk_named_parameters())


def _cotangents(y, sim, seed=11):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(y.shape, generator=g), torch.randn(sim.shape, generator=g)


def _rnd(shape, seed, scale=1.0):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * scale


def _yard_bound(fn32, ref64, floor=SUM_FLOOR, measure=relerr):
    """max(floor, YARD_FACTOR x the float32 CPU restatement's error against float64)."""
    torch.set_num_threads(_threads())
    return max(floor, YARD_FACTOR * measure(fn32(), ref64))


# ================================================================================================ the failing-before test
def test_training_path_returns_history(vgg):
    net = _make_warp()
    ins = _gpu_inputs(vgg, 48, 80, 1)
    y, sim = net(*ins, temperature=0.01)
    assert y.requires_grad and sim.requires_grad
    gy, gs = _cotangents(y, sim)
    ((y * gy.cuda()).sum() + (sim * gs.cuda()).sum()).backward()
    params = _trunk_params(net)
    assert len(params) == 19
    for n, p in params.items():
        assert p.grad is not None, n
        assert torch.isfinite(p.grad).all(), n
        assert p.grad.abs().max().item() > 0, n
    for h in HEADS:
        assert all(p.grad is None for p in getattr(net, h).parameters())


# ================================================================================================ forward bit-identity
@pytest.mark.parametrize("algo", ["auto", "direct"])
@pytest.mark.parametrize("H,W,N", [(48, 80, 1), (48, 80, 2), (64, 96, 1), (64, 96, 2), (216, 384, 1), (216, 384, 2)])
def test_forward_bit_identical_to_no_grad(vgg, algo, H, W, N):
    from dvc_amd import ops
    prev = ops.conv_algo()
    ops.set_conv_algo(algo)
    try:
        net = _make_warp()
        ins = _gpu_inputs(vgg, H, W, N)
        for T in (0.01, 1e-10):
            y, sim = net(*ins, temperature=T)
            assert y.requires_grad and sim.requires_grad
            with torch.no_grad():
                y0, s0 = net(*ins, temperature=T)
            net.eval()
            y1, s1 = net(*ins, temperature=T)
            net.train()
            assert not y0.requires_grad and not y1.requires_grad
            assert torch.equal(y, y0) and torch.equal(sim, s0), (algo, H, W, N, T)
            assert torch.equal(y, y1) and torch.equal(sim, s1), (algo, H, W, N, T)
        # the 2N-image walk of the shared blocks equals the two separate walks
        with torch.no_grad():
            tA, tB = net._heads(*ins[1:5]), net._heads(*ins[5:9])
            both = net._trunk(torch.cat((tA, tB), 0), saved={})
            assert torch.equal(both[:N], net._trunk(tA)) and torch.equal(both[N:], net._trunk(tB))
    finally:
        ops.set_conv_algo(prev)


# ================================================================================================ step-wise
SIZES = [(4, 54, 96), (3, 9, 7)]


@pytest.mark.parametrize("M,H,W", SIZES)
def test_step_up4_bwd(M, H, W):
    from dvc_amd import ops
    g = _rnd((M, 3, 4 * H, 4 * W), 1)
    got = ops.warp_up4_bwd(g.cuda()).cpu()
    e = relerr(got, R.up4_bwd(g.double()))
    report(f"step up4_bwd {M}x{H}x{W}: {e:.2e}")
    assert e <= ELEM
    view = g.cuda()[:, 1:2]                                  # a channel slice is copied by the caller, never read strided
    assert torch.equal(ops.warp_up4_bwd(view.contiguous()).cpu(), got[:, 1:2])
    odd = torch.empty(g.numel() + 1, device="cuda")[1:].view_as(g).copy_(g)       # a 4-byte-aligned base: the scalar loads
    assert torch.equal(ops.warp_up4_bwd(odd).cpu(), got)


@pytest.mark.parametrize("B,C,P", [(4, 256, 54 * 96), (3, 256, 63), (2, 16, 5)])
def test_step_cn_bwd(B, C, P):
    from dvc_amd import ops
    t = _rnd((B, C, P), 2) + 0.3
    g = _rnd((B, C, P), 3)
    out, mean = ops.corr_prepare_with_mean(t.cuda())
    assert torch.equal(out, ops.corr_prepare(t.cuda()))
    got = ops.warp_cn_bwd(t.cuda(), mean, g.cuda()).cpu()
    ref = R.cn_bwd(t.double(), g.double())
    bound = _yard_bound(lambda: R.cn_bwd(t, g), ref)
    e = relerr(got, ref)
    report(f"step cn_bwd {B}x{C}x{P}: {e:.2e} (bound {bound:.2e})")
    assert e <= bound


def test_step_cn_bwd_zero_norm_position():
    """A position whose centred vector is exactly 0 (r == 0): the second term is 0, not NaN."""
    from dvc_amd import ops
    t = torch.zeros(1, 8, 4)
    t[0, :, 1:] = _rnd((8, 3), 4)
    t[0, :, 1:] -= t[0, :, 1:].mean(-1, keepdim=True)        # row means 0 -> position 0 stays exactly 0 after centring
    t[0, :, 0] = 0.0
    g = _rnd((1, 8, 4), 5)
    out, mean = ops.corr_prepare_with_mean(t.cuda())
    got = ops.warp_cn_bwd(t.cuda(), mean, g.cuda())
    assert torch.isfinite(got).all()


@pytest.mark.parametrize("N,Cin,Cout,P", [(2, 256, 256, 54 * 96), (3, 256, 256, 63), (2, 70, 33, 37), (8, 256, 256, 54 * 96)])
def test_step_k1_wgrad(N, Cin, Cout, P):
    from dvc_amd import ops
    dT = _rnd((N, Cout, P), 6)
    Fin = _rnd((N, Cin, P), 7) + 0.2
    dW, db = ops.warp_k1_wgrad(dT.cuda(), Fin.cuda())
    rW, rb = R.k1_wgrad(dT.double(), Fin.double())
    torch.set_num_threads(_threads())
    yW, yb = R.k1_wgrad(dT, Fin)
    bW, bb = max(SUM_FLOOR, YARD_FACTOR * relerr(yW, rW)), max(SUM_FLOOR, YARD_FACTOR * relerr(yb, rb))
    eW, eb = relerr(dW.cpu(), rW), relerr(db.cpu(), rb)
    report(f"step k1_wgrad N{N} {Cin}->{Cout} P{P}: dW {eW:.2e} (bound {bW:.2e}) db {eb:.2e} (bound {bb:.2e})")
    assert eW <= bW and eb <= bb
    # another split, a misaligned view (scalar loads): same sums to the same bound; two runs bit-identical
    dW1, db1 = ops.warp_k1_wgrad(dT.cuda(), Fin.cuda(), splits=1 if P < 100 else 7)
    assert relerr(dW1.cpu(), rW) <= bW and relerr(db1.cpu(), rb) <= bb
    odd = torch.empty(dT.numel() + 1, device="cuda")[1:].view_as(dT).copy_(dT)
    dW2, db2 = ops.warp_k1_wgrad(odd, Fin.cuda())
    assert relerr(dW2.cpu(), rW) <= bW and relerr(db2.cpu(), rb) <= bb
    dW3, db3 = ops.warp_k1_wgrad(dT.cuda(), Fin.cuda())
    assert torch.equal(dW, dW3) and torch.equal(db, db3)


def test_step_k1_wgrad_exact_integers_asymmetric():
    """Exact small-integer data: every product and sum is exact in fp32, so a swapped row / column or a wrong K permutation shows
    as a mismatch, not as rounding."""
    from dvc_amd import ops
    g = torch.Generator().manual_seed(8)
    dT = torch.randint(-3, 4, (2, 96, 70), generator=g).float()
    Fin = torch.randint(-3, 4, (2, 130, 70), generator=g).float()
    dW, db = ops.warp_k1_wgrad(dT.cuda(), Fin.cuda())
    rW, rb = R.k1_wgrad(dT.double(), Fin.double())
    assert torch.equal(dW.cpu().double(), rW) and torch.equal(db.cpu().double(), rb)


@pytest.mark.parametrize("M,H,W", SIZES + [(2, 2, 2), (2, 3, 3), (1, 2, 5)])
@pytest.mark.parametrize("a", [0.25, 0.0, -0.5])
def test_step_norm_prelu_bwd(M, H, W, a):
    from dvc_amd import ops
    C = 256 if H == 54 else 5                   # (4 x 256 = 1024 planes: more workgroups than one round of the chip holds)
    n = _rnd((M, C, H, W), 9)
    n.view(-1)[::7] = 0.0                       # entries with u == 0 at the first site
    skip = _rnd((M, C, H, W), 10)
    skip.view(-1)[::5] = -n.view(-1)[::5]       # ... and n + skip == 0 at the second
    g = _rnd((M, C, H, W), 12)
    g[0, 0] = 1.5                               # a plane whose du is constant where u > 0 ...
    n[0, 0] = n[0, 0].abs() + 0.1               # ... (all of it: dz = rstd (c - c - n mean(c n)))
    rstd = _rnd((M * C,), 13).abs() + 0.5
    at = torch.tensor([a])
    for sk in (None, skip):
        dz, du, part = ops.warp_norm_prelu_bwd(g.cuda(), n.cuda(), rstd.cuda(), at.cuda(), skip=None if sk is None else sk.cuda())
        rz, ru, rp = R.norm_prelu_bwd(g.double(), n.double(), rstd.double(), at.double(), skip=None if sk is None else sk.double())
        ez = relerr(dz.cpu(), rz)
        ring = dz.clone()
        ring[:, :, 1:-1, 1:-1] = 0
        assert not ring.any(), "the ring must be zero"
        ep = relerr(part.cpu(), rp)
        report(f"step norm_prelu_bwd {M}x{C}x{H}x{W} a={a} skip={sk is not None}: dz {ez:.2e} slope partials {ep:.2e}")
        assert ez <= ELEM and ep <= ELEM
        if sk is not None:
            assert relerr(du.cpu(), ru) <= ELEM
        # (the partials are double sums of exact products; their sum in double is rounded once)
        assert relerr(ops.warp_slope_sum(part).cpu(), rp.sum().reshape(1)) <= ELEM


@pytest.mark.parametrize("M,H,W", SIZES + [(2, 2, 2), (2, 3, 3), (1, 2, 5), (1, 6, 3)])
def test_step_reflect_pad_and_fold(M, H, W):
    from dvc_amd import ops
    C = 256 if H == 54 else 5
    x = _rnd((M, C, H, W), 14)
    assert torch.equal(ops.warp_reflect_pad(x.cuda()).cpu(), F.pad(x, (1, 1, 1, 1), mode="reflect"))
    gp = _rnd((M, C, H + 2, W + 2), 15)
    skip = _rnd((M, C, H, W), 16)
    for sk in (None, skip):
        got = ops.warp_fold(gp.cuda(), None if sk is None else sk.cuda()).cpu()
        e = relerr(got, R.fold(gp.double(), None if sk is None else sk.double()))
        assert e <= ELEM, (M, H, W, e)
    assert relerr(ops.warp_fold(gp.cuda()).cpu(), R.fold(gp.double(), defect="no_fold")) > 1e-2


@pytest.mark.parametrize("M,H,W", SIZES)
def test_step_prelu_fwd_is_the_norm_launch_expression(M, H, W):
    from dvc_amd import ops
    x = _rnd((M, 8, H, W), 17).cuda()
    res = _rnd((M, 8, H, W), 18).cuda()
    a = torch.tensor([0.25]).cuda()
    for r in (None, res):
        fused = ops.instnorm_apply(x, residual=r, slope_t=a)
        n = ops.instnorm_apply(x)
        assert torch.equal(ops.warp_prelu_fwd(n, a, skip=r), fused)


@pytest.mark.parametrize("algo", ["direct", "winograd"])
@pytest.mark.parametrize("M,H,W", SIZES)
def test_step_conv_input_gradient_ring_conv_fold(algo, M, H, W):
    """The zero-ringed dz through ops.conv3x3 (zero pad 1, W^T flipped) and the fold, against float64: the engines' bounds, the
    border band (where the fold lands) and the interior reported separately."""
    from dvc_amd import ops
    from dvc_amd.nets import vgg_bwd_weight
    prev = ops.conv_algo()
    ops.set_conv_algo(algo)
    try:
        C = 256
        w = _rnd((C, C, 3, 3), 19, (2.0 / (9 * C)) ** 0.5)
        dz = _rnd((M, C, H, W), 20)
        wt = vgg_bwd_weight(w.cuda())

        def packs(kind):
            return {"winograd": ops.pack_winograd_weight, "ws": ops.pack_ws_weight}.get(kind, ops.pack_conv_weight)(wt)
        dzr = F.pad(dz, (1, 1, 1, 1)).cuda()
        engine = "winograd" if ops.winograd_selected(M, C, H + 2, W + 2, C, layer="warp_bwd.test") else "direct"
        gp = ops.conv3x3(dzr, wt, packs, None, layer="warp_bwd.test")
        got = ops.warp_fold(gp).cpu()
        ref = R.fold(R.padded_input_grad(F.pad(dz.double(), (1, 1, 1, 1)), w.double()))
        m = map_measures(got, ref, 2)
        report(f"step conv input gradient {algo}->{engine} {M}x{C}x{H}x{W}: " + " ".join(f"{k}={v:.2e}" for k, v in m.items() if v is not None))
        for k, v in m.items():
            assert v is None or v <= DGRAD_BOUND[engine], (k, v)
        # the same against autograd through the reflect-padded layer itself (the restatement is checked on the CPU; this closes
        # the loop on the device result)
        x = torch.zeros(M, C, H, W, dtype=torch.float64, requires_grad=True)
        F.conv2d(F.pad(x, (1, 1, 1, 1), mode="reflect"), w.double()).backward(dz.double())
        assert relerr(got, x.grad) <= DGRAD_BOUND[engine]
    finally:
        ops.set_conv_algo(prev)


@pytest.mark.parametrize("M,H,W", SIZES)
def test_step_padded_copy_weight_gradient(M, H, W):
    from dvc_amd import ops
    C = 256 if H == 54 else 40
    dz = _rnd((M, C, H, W), 21)
    x = _rnd((M, C, H, W), 22) + 0.1
    dW, db = ops.cvn_wgrad(F.pad(dz, (1, 1, 1, 1)).cuda(), ops.warp_reflect_pad(x.cuda()))
    w = torch.zeros(C, C, 3, 3, dtype=torch.float64, requires_grad=True)
    b = torch.zeros(C, dtype=torch.float64, requires_grad=True)
    F.conv2d(F.pad(x.double(), (1, 1, 1, 1), mode="reflect"), w, b).backward(dz.double())
    torch.set_num_threads(_threads())
    yW, yb = R.padded_wgrad(F.pad(dz, (1, 1, 1, 1)), R.reflect_pad(x))
    bW, bb = max(SUM_FLOOR, YARD_FACTOR * relerr(yW, w.grad)), max(SUM_FLOOR, YARD_FACTOR * relerr(yb, b.grad))
    eW, eb = relerr(dW.cpu(), w.grad), relerr(db.cpu(), b.grad)
    report(f"step padded-copy wgrad {M}x{C}x{H}x{W}: dW {eW:.2e} (bound {bW:.2e}) db {eb:.2e} (bound {bb:.2e})")
    assert eW <= bW and eb <= bb


# ================================================================================================ end to end vs float64
def _oracle_loss(sd, ins, gy, gs, T, dtype):
    """The loss through the oracle's own functions with the trunk tensor exposed: heads (not differentiated), torch.cat, the
    residual blocks, corr_project, correlate, x4 nearest.  Returns (grads of the 19 parameters, seam gradients (A, B), y, sim,
    taps)."""
    from oracle import dvc_oracle as O
    sd = {k: v.to(dtype) for k, v in sd.items()}
    leaves = {k: v.clone().requires_grad_() for k, v in sd.items() if k.split(".")[0] in ("layer", "theta", "phi")}
    sdl = dict(sd)
    sdl.update(leaves)
    ins = [t.to(dtype) for t in ins]
    seams = []

    def side(r2, r3, r4, r5):
        with torch.no_grad():
            f = [O.warp_head(sd, nm, x) for nm, x in zip(HEADS, (r2, r3, r4, r5))]
            if f[3].shape[2] != f[0].shape[2] or f[3].shape[3] != f[0].shape[3]:
                f[3] = F.pad(f[3], (0, 0, 1, 1), "replicate")
            x = torch.cat(f, 1)
        x.requires_grad_()
        seams.append(x)
        for b in range(3):
            x = O.residual_block(sdl, f"layer.{b}", x)
        return x
    fa, fb = side(*ins[1:5]), side(*ins[5:9])
    theta, phi = O.corr_project(sdl, "theta", fa), O.corr_project(sdl, "phi", fb)
    y, sim, f = O.correlate(theta, phi, ins[0], T)
    taps = dict(top2=torch.topk(f.detach(), 2, dim=-1)[0])
    y = F.interpolate(y, scale_factor=4, mode="nearest")
    sim = F.interpolate(sim, scale_factor=4, mode="nearest")
    ((y * gy.to(dtype)).sum() + (sim * gs.to(dtype)).sum()).backward()
    return {k: v.grad for k, v in leaves.items()}, (seams[0].grad, seams[1].grad), y.detach(), sim.detach(), taps


def _tensor_err(name, got, ref, refs):
    """max-abs error over max-abs of the reference; a bias (true gradient 0) over max |dW_ref| of its layer (module docstring)."""
    if name.endswith(".bias"):
        return ((got.double() - ref.double()).abs().max() / refs[name[:-4] + "weight"].double().abs().max()).item()
    return relerr(got, ref)


@pytest.mark.parametrize("H,W,seed", [(48, 80, 0), (64, 112, 0)])
def test_end_to_end_against_float64_autograd(H, W, seed):
    """All 19 parameter gradients and the seam gradient of both sides, N = 2, T = 0.01, loss on both outputs.

    Measured on the MI355X (error / bound, worst tensor per size): see DESIGN.md section 6d."""
    from dvc_amd import ops, synth
    from oracle import dvc_oracle as O
    N, T = 2, 0.01
    torch.set_num_threads(_threads())
    ins = _cpu_inputs(H, W, N, seed)
    sd = synth.warpnet_state_dict(0)
    gy, gs = _cotangents(torch.empty(N, 3, H, W), torch.empty(N, 1, H, W))
    ref, ref_seam, y64, s64, taps = _oracle_loss(sd, ins, gy, gs, T, torch.float64)
    with torch.no_grad():       # the restatement above is the oracle's forward
        y_o, s_o = O.warpnet_forward(O.to_dtype(sd, torch.float64), *[t.double() for t in ins], temperature=T)
    assert torch.equal(y64, y_o) and torch.equal(s64, s_o)
    gap = taps["top2"][..., 0] - taps["top2"][..., 1]
    report(f"e2e {H}x{W}: smallest top-1 / top-2 gap of the float64 affinities {gap.min().item():.3e}")
    assert gap.min().item() > 1e-5, "pick another seed: an fp32 arg-max may differ from the float64 one"
    yard, yard_seam, _, _, _ = _oracle_loss(sd, ins, gy, gs, T, torch.float32)

    net = _make_warp()
    dev = [t.cuda() for t in ins]
    with torch.no_grad():
        tA, tB = net._heads(*dev[1:5]), net._heads(*dev[5:9])
        blab = ops.avgpool4x4(dev[0])
    tA.requires_grad_()
    tB.requires_grad_()
    y, sim = net._train_from_trunks(tA, tB, blab, T)
    ((y * gy.cuda()).sum() + (sim * gs.cuda()).sum()).backward()
    got = {n: p.grad.cpu() for n, p in _trunk_params(net).items()}
    got["seam.A"], got["seam.B"] = tA.grad.cpu(), tB.grad.cpu()
    ref["seam.A"], ref["seam.B"] = ref_seam
    yard["seam.A"], yard["seam.B"] = yard_seam
    assert len(got) == 21
    bad = []
    for name in got:
        e_y = _tensor_err(name, yard[name], ref[name], ref)
        e = _tensor_err(name, got[name], ref[name], ref)
        bound = max(1e-6, YARD_FACTOR * e_y)
        report(f"e2e {H}x{W} {name:24s} hip {e:.3e}  float32 CPU oracle {e_y:.3e}  bound {bound:.3e}")
        if not e <= bound:
            bad.append((name, e, bound))
    assert not bad, bad


# ================================================================================================ determinism
def test_backward_is_deterministic_and_batch_consistent(vgg):
    """Two backward runs are bit-identical.  Image 0 of a batch of 2 with zero cotangent on image 1 against the batch of 1: the
    seam gradient of image 0 is bit-identical (every step up to it is per image: per-plane norms, per-image convolutions and
    correlation); the parameter gradients are sums over all images taken in position slots whose boundaries move with the batch
    size, so they agree to rounding (the sums' bound), not bit for bit."""
    from dvc_amd import ops
    H, W, T = 64, 96, 0.01
    ins2 = _gpu_inputs(vgg, H, W, 2)

    def run(ins, zero_second):
        net = _make_warp()
        with torch.no_grad():
            tA, tB = net._heads(*ins[1:5]), net._heads(*ins[5:9])
            blab = ops.avgpool4x4(ins[0])
        tA.requires_grad_()
        tB.requires_grad_()
        y, sim = net._train_from_trunks(tA, tB, blab, T)
        gy, gs = _cotangents(y[:1], sim[:1])
        gy, gs = gy.cuda().repeat(y.shape[0], 1, 1, 1), gs.cuda().repeat(y.shape[0], 1, 1, 1)
        if zero_second:
            gy[1:], gs[1:] = 0, 0
        ((y * gy).sum() + (sim * gs).sum()).backward()
        return {n: p.grad.clone() for n, p in _trunk_params(net).items()}, tA.grad.clone(), tB.grad.clone()

    g_a, sA_a, sB_a = run(ins2, True)
    g_b, sA_b, sB_b = run(ins2, True)
    assert torch.equal(sA_a, sA_b) and torch.equal(sB_a, sB_b)
    for n in g_a:
        assert torch.equal(g_a[n], g_b[n]), n
    ins1 = [t[:1].contiguous() for t in ins2]
    g_1, sA_1, sB_1 = run(ins1, False)
    assert torch.equal(sA_a[:1], sA_1) and torch.equal(sB_a[:1], sB_1)
    assert not sA_a[1:].any() and not sB_a[1:].any()
    for n in g_a:
        if n.endswith(".bias"):
            continue                                         # (rounding residue of an exactly-cancelling sum: no common value)
        # (a sanity bound on two fp32 summation orders of the same terms; the precision claim is the end-to-end test's)
        assert relerr(g_a[n], g_1[n].double()) <= 1e-4, n


# ================================================================================================ guards
def test_guards(vgg):
    ins = _gpu_inputs(vgg, 48, 80, 1)
    net = _make_warp(freeze_heads=False)
    with pytest.raises(NotImplementedError, match="freeze"):
        net(*ins)
    net = _make_warp()
    cache = net.exemplar_side(ins[0], *ins[5:9])
    for kw in (dict(exemplar_cache=cache), dict(return_taps=True), dict(detach_flag=True), dict(defer_merge=True)):
        with pytest.raises(NotImplementedError):
            net(*ins, **kw)
    x = [t.clone() for t in ins]
    x[2].requires_grad_()
    with pytest.raises(NotImplementedError, match="input requires grad"):
        net(*x)
    # eval mode with trainable parameters: today's no-history output
    net.eval()
    y, sim = net(*ins)
    assert not y.requires_grad and not sim.requires_grad
    # the exemplar memo is neither hit nor filled by a training call
    memo = getattr(net, "_exemplar_memo", None)
    assert memo is not None
    net.train()
    y2, _ = net(*ins)
    assert y2.requires_grad and getattr(net, "_exemplar_memo", None) is memo
    fresh = _make_warp()
    fresh(*ins)
    assert getattr(fresh, "_exemplar_memo", None) is None
    # only some parameters trainable: the others get no gradient
    part = _make_warp()
    for p in part.parameters():
        p.requires_grad = False
    part.layer[2].conv2.weight.requires_grad = True
    part.phi.bias.requires_grad = True
    y, sim = part(*ins)
    (y.sum() + sim.sum()).backward()
    for n, p in part.named_parameters():
        assert (p.grad is not None) == (n in ("layer.2.conv2.weight", "phi.bias")), n


# ================================================================================================ frame_colorization
def _frame_setup(H, W, N):
    from dvc_amd import synth
    sds = (synth.vgg19_state_dict(0), synth.warpnet_state_dict(0), synth.colorvidnet_state_dict(0, contractive=True))
    IA = torch.cat([synth.synth_lab(1000 + k, H, W) for k in range(N)])
    IB = torch.cat([synth.synth_lab(2 + 7 * k, H, W) for k in range(N)])
    last = torch.cat([synth.synth_lab(500 + k, H, W) for k in range(N)])
    g = _rnd((N, 2, H, W), 31)
    return sds, IA, IB, last, g


def _frame_oracle(sds, IA, IB, last, g, T, dtype):
    from oracle import dvc_oracle as O
    sd_v, sd_w, sd_c = (O.to_dtype(sd, dtype) for sd in sds)
    leaves = {k: v.clone().requires_grad_() for k, v in sd_w.items() if k.split(".")[0] in ("layer", "theta", "phi")}
    sd_w = dict(sd_w)
    sd_w.update(leaves)
    IA, IB, last = IA.to(dtype), IB.to(dtype), last.to(dtype)
    with torch.no_grad():
        fB = O.exemplar_features(IB, sd_v)
    taps = {}
    ab, _, _ = O.frame_colorization(IA, IB, last, fB, sd_v, sd_w, sd_c, temperature=T, taps=taps)
    (ab * g.to(dtype)).sum().backward()
    return {k: v.grad for k, v in leaves.items()}, taps["top2"].detach()


def test_frame_colorization_trains_both_networks(vgg):
    from dvc_amd.frame import frame_colorization
    from models.ColorVidNet import ColorVidNet
    from oracle import dvc_oracle as O
    H, W, N, T = 64, 96, 2, 0.01
    torch.set_num_threads(_threads())
    sds, IA, IB, last, g = _frame_setup(H, W, N)
    ref, top2 = _frame_oracle(sds, IA, IB, last, g, T, torch.float64)
    gap = (top2[..., 0] - top2[..., 1]).min().item()
    report(f"frame {H}x{W}: smallest top-1 / top-2 gap {gap:.3e}")
    assert gap > 1e-5
    yard, _ = _frame_oracle(sds, IA, IB, last, g, T, torch.float32)

    with contextlib.redirect_stdout(io.StringIO()):
        cvn = ColorVidNet(7)
    cvn.load_state_dict(sds[2])
    cvn.train().cuda()
    warp = _make_warp()
    for p in vgg.parameters():
        p.requires_grad = False
    dIA, dIB, dlast = IA.cuda(), IB.cuda(), last.cuda()
    with torch.no_grad():
        fB = vgg(O.tensor_lab2rgb(torch.cat((O.uncenter_l(IB[:, 0:1]), IB[:, 1:3]), dim=1)).cuda(), O.VGG_OUT, preprocess=True)
        ab0, warped0, _ = frame_colorization(dIA, dIB, dlast, fB, vgg, warp, cvn, temperature=T)
    ab, warped, _ = frame_colorization(dIA, dIB, dlast, fB, vgg, warp, cvn, temperature=T)
    assert ab.requires_grad and torch.equal(ab, ab0) and torch.equal(warped, warped0)
    (ab * g.cuda()).sum().backward()
    cp = dict(cvn.named_parameters())
    wp = _trunk_params(warp)
    assert len(cp) == 65 and len(wp) == 19
    for n, p in list(cp.items()) + list(wp.items()):
        assert p.grad is not None and torch.isfinite(p.grad).all() and p.grad.abs().max().item() > 0, n
    bad = []
    for n, p in wp.items():
        e_y, e = _tensor_err(n, yard[n], ref[n], ref), _tensor_err(n, p.grad.cpu(), ref[n], ref)
        bound = max(1e-6, YARD_FACTOR * e_y)
        report(f"frame {H}x{W} {n:24s} hip {e:.3e}  float32 CPU oracle {e_y:.3e}  bound {bound:.3e}")
        if not e <= bound:
            bad.append((n, e, bound))
    assert not bad, bad
    # three optimiser steps on both networks lower a fixed loss
    target = _rnd((N, 2, H, W), 32).cuda() * 20
    params = list(cp.values()) + list(wp.values())
    opt, losses = None, []
    for _ in range(4):
        for p in params:
            p.grad = None
        ab, _, _ = frame_colorization(dIA, dIB, dlast, fB, vgg, warp, cvn, temperature=T)
        loss = ((ab - target) ** 2).mean()
        losses.append(loss.item())
        loss.backward()
        if opt is None:     # step size: a first-order decrease of 0.1 % of the loss per step
            gsq = sum(p.grad.double().pow(2).sum().item() for p in params)
            opt = torch.optim.SGD(params, lr=1e-3 * losses[0] / gsq)
        opt.step()
    report("frame optimiser losses " + " ".join(f"{v:.6f}" for v in losses))
    assert losses[3] < losses[0]
