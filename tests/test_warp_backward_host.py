"""CPU: the host side of WarpNet's backward behind the trunk tensor — header / ctypes table / export agreement and C-ABI validation
of the new entry points (csrc/warp_bwd.hip), the float64 restatements of every new launch kind (tests/warp_bwd_reference.py)
against float64 autograd through oracle.dvc_oracle to 1e-12 relative (the bound of tests/test_bwd_audit_host.py), seeded defects
that must break that bound, the backward filter transform, and the guards that need no device."""
import ctypes
import os
import re
import subprocess

import pytest
import torch
import torch.nn.functional as F

import warp_bwd_reference as R
from bwd_audit import relerr
from cabi_common import _fails, _lib
from oracle import dvc_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ONE = ctypes.c_void_p(256)      # a non-null address that is never dereferenced: every call below fails validation first
TWO, THREE = ctypes.c_void_p(1024), ctypes.c_void_p(4096)
NEW = ["dvc_warp_up4_bwd", "dvc_warp_prelu_fwd", "dvc_warp_cn_bwd", "dvc_warp_k1_wgrad_splits", "dvc_warp_k1_wgrad",
       "dvc_warp_norm_prelu_bwd", "dvc_warp_slope_sum", "dvc_warp_reflect_pad", "dvc_warp_fold"]
BOUND = 1e-12
TRUNK_NAMES = [f"layer.{b}.{k}" for b in range(3) for k in ("conv1.weight", "conv1.bias", "conv2.weight", "conv2.bias",
                                                             "prelu.weight")] + ["theta.weight", "theta.bias", "phi.weight", "phi.bias"]


def _block_sd(seed, ch=6, a=0.25):
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for k in (1, 2):
        sd[f"b.conv{k}.weight"] = torch.randn(ch, ch, 3, 3, generator=g, dtype=torch.float64) * 0.3
        sd[f"b.conv{k}.bias"] = torch.randn(ch, generator=g, dtype=torch.float64)
    sd["b.prelu.weight"] = torch.tensor([a], dtype=torch.float64)
    return sd


# ================================================================================================ C-ABI
def test_new_entry_points_in_header_table_and_exports():
    from dvc_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "dvc_hip.h")).read()
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    for name in NEW:
        assert re.search(r"\b%s\(" % name, hdr), name
        assert name in _lib.SIGNATURES, name
        assert re.search(r"\b%s\b" % name, out), name
    assert _lib.load().dvc_abi_version() == _lib.ABI_VERSION


def test_validation_without_gpu():
    lib = _lib()
    big = 1 << 40
    _fails(lib.dvc_warp_up4_bwd(None, 1, 2, 2, TWO, None), lib, "null pointer")
    _fails(lib.dvc_warp_up4_bwd(ONE, 1, 0, 2, TWO, None), lib, "bad size")
    _fails(lib.dvc_warp_up4_bwd(ONE, 1, 2, 2, ONE, None), lib, "alias")
    _fails(lib.dvc_warp_prelu_fwd(ONE, None, None, 4, TWO, None), lib, "null pointer")
    _fails(lib.dvc_warp_prelu_fwd(ONE, None, ONE, 0, TWO, None), lib, "bad size")
    _fails(lib.dvc_warp_cn_bwd(ONE, ONE, None, 1, 4, 4, 0.0, TWO, None), lib, "null pointer")
    _fails(lib.dvc_warp_cn_bwd(ONE, ONE, ONE, 1, 0, 4, 0.0, TWO, None), lib, "bad size")
    _fails(lib.dvc_warp_cn_bwd(ONE, TWO, THREE, 1, 4, 4, 0.0, ONE, None), lib, "alias")
    f = lib.dvc_warp_k1_wgrad
    _fails(f(None, ONE, 1, 8, 8, 16, 1, TWO, big, THREE, None), lib, "null pointer")
    _fails(f(ONE, ONE, 1, 8, 0, 16, 1, TWO, big, THREE, None), lib, "bad size")
    _fails(f(ONE, ONE, 1, 8, 8, 16, 0, TWO, big, THREE, None), lib, "S must")
    _fails(f(ONE, ONE, 1, 8, 8, 16, 2, TWO, 10, THREE, None), lib, "workspace too small")
    _fails(f(ONE, ONE, 1, 8, 8, 16, 1, TWO, big, ONE, None), lib, "alias")
    assert lib.dvc_warp_k1_wgrad_splits(0, 8, 8, 4) == 0
    assert lib.dvc_warp_k1_wgrad_splits(8, 256, 256, 5184) == 32
    assert lib.dvc_warp_k1_wgrad_splits(1, 256, 256, 4) == 1
    f = lib.dvc_warp_norm_prelu_bwd
    _fails(f(ONE, ONE, None, ONE, None, 1, 4, 4, TWO, None, THREE, None), lib, "null pointer")
    _fails(f(ONE, ONE, None, ONE, ONE, 0, 4, 4, TWO, None, THREE, None), lib, "bad size")
    _fails(f(ONE, ONE, None, ONE, ONE, 1, 4, 4, ONE, None, THREE, None), lib, "alias")
    _fails(lib.dvc_warp_slope_sum(None, 4, TWO, None), lib, "null pointer")
    _fails(lib.dvc_warp_slope_sum(ONE, 0, TWO, None), lib, "bad size")
    _fails(lib.dvc_warp_reflect_pad(ONE, 1, 1, 4, TWO, None), lib, "bad size")
    _fails(lib.dvc_warp_reflect_pad(ONE, 1, 4, 4, ONE, None), lib, "alias")
    _fails(lib.dvc_warp_fold(ONE, None, 1, 4, 1, TWO, None), lib, "bad size")
    _fails(lib.dvc_warp_fold(None, None, 1, 4, 4, TWO, None), lib, "null pointer")
    _fails(lib.dvc_warp_fold(ONE, None, 1, 4, 4, ONE, None), lib, "alias")


# ================================================================================================ float64 restatements vs autograd
def test_up4_bwd_matches_autograd():
    g = torch.Generator().manual_seed(0)
    x = torch.randn(2, 3, 5, 7, generator=g, dtype=torch.float64, requires_grad=True)
    gy = torch.randn(2, 3, 20, 28, generator=g, dtype=torch.float64)
    F.interpolate(x, scale_factor=4, mode="nearest").backward(gy)
    assert relerr(R.up4_bwd(gy), x.grad) <= BOUND


@pytest.mark.parametrize("shape", [(2, 16, 35), (1, 256, 24)])
def test_cn_bwd_matches_autograd_through_corr_project(shape):
    g = torch.Generator().manual_seed(1)
    B, C, P = shape
    t = torch.randn(B, C, P, generator=g, dtype=torch.float64, requires_grad=True)
    gt = torch.randn(B, C, P, generator=g, dtype=torch.float64)
    # corr_project with an identity 1x1 convolution is exactly the centre-and-normalise step
    sd = {"w.weight": torch.eye(C, dtype=torch.float64).reshape(C, C, 1, 1), "w.bias": torch.zeros(C, dtype=torch.float64)}
    if C == 256:
        O.corr_project(sd, "w", t.reshape(B, C, P, 1)).backward(gt)
    else:
        tc = t - t.mean(dim=-1, keepdim=True)
        torch.div(tc, torch.norm(tc, 2, 1, keepdim=True) + O.EPS).backward(gt)
    assert relerr(R.cn_bwd(t.detach(), gt), t.grad) <= BOUND


def test_k1_wgrad_matches_autograd():
    g = torch.Generator().manual_seed(2)
    w = torch.randn(5, 7, 1, 1, generator=g, dtype=torch.float64, requires_grad=True)
    b = torch.randn(5, generator=g, dtype=torch.float64, requires_grad=True)
    x = torch.randn(3, 7, 4, 6, generator=g, dtype=torch.float64)
    gt = torch.randn(3, 5, 4, 6, generator=g, dtype=torch.float64)
    F.conv2d(x, w, b).backward(gt)
    dW, db = R.k1_wgrad(gt, x)
    assert relerr(dW, w.grad) <= BOUND and relerr(db, b.grad) <= BOUND


def test_backward_filter_transform():
    from dvc_amd.nets import vgg_bwd_weight
    w = torch.randn(4, 6, 3, 3, dtype=torch.float64)
    wt = R.bwd_weight(w)
    assert wt.shape == (6, 4, 3, 3) and torch.equal(wt, vgg_bwd_weight(w))
    for ky in range(3):
        for kx in range(3):
            assert torch.equal(wt[:, :, ky, kx], w[:, :, 2 - ky, 2 - kx].t())


@pytest.mark.parametrize("hw", [(9, 7), (2, 2), (3, 3), (2, 5), (6, 3)])
def test_ring_conv_fold_and_padded_wgrad_match_autograd(hw):
    """ring + zero-pad convolution + fold == the input gradient of ReflectionPad2d(1) + Conv2d(3, padding=0); the padded-copy weight
    gradient == its weight / bias gradient."""
    H, W = hw
    g = torch.Generator().manual_seed(3)
    w = torch.randn(5, 4, 3, 3, generator=g, dtype=torch.float64, requires_grad=True)
    b = torch.randn(5, generator=g, dtype=torch.float64, requires_grad=True)
    x = torch.randn(2, 4, H, W, generator=g, dtype=torch.float64, requires_grad=True)
    dz = torch.randn(2, 5, H, W, generator=g, dtype=torch.float64)
    skip = torch.randn(2, 4, H, W, generator=g, dtype=torch.float64)
    O._rconv(x, w, b).backward(dz)
    gp = R.padded_input_grad(R.ring(dz), w.detach())
    assert relerr(R.fold(gp), x.grad) <= BOUND
    assert torch.equal(R.fold(gp, skip=skip), R.fold(gp) + skip)
    dW, db = R.padded_wgrad(R.ring(dz), R.reflect_pad(x.detach()))
    assert relerr(dW, w.grad) <= BOUND and relerr(db, b.grad) <= BOUND
    assert relerr(R.fold(gp, defect="no_fold"), x.grad) > 1e-3        # seeded defect: the ring dropped


@pytest.mark.parametrize("a", [0.25, 0.0, -0.5])
def test_norm_prelu_bwd_both_sites_match_autograd(a):
    g = torch.Generator().manual_seed(4)
    z = torch.randn(2, 3, 6, 5, generator=g, dtype=torch.float64, requires_grad=True)
    skip = torch.randn(2, 3, 6, 5, generator=g, dtype=torch.float64, requires_grad=True)
    gy = torch.randn(2, 3, 6, 5, generator=g, dtype=torch.float64)
    at = torch.tensor([a], dtype=torch.float64, requires_grad=True)
    for with_skip in (False, True):
        for t in (z, skip, at):
            t.grad = None
        n = O._inorm(z)
        F.prelu(n + skip if with_skip else n, at).backward(gy)
        rstd = 1.0 / torch.sqrt(z.detach().var((2, 3), unbiased=False) + 1e-5).reshape(-1)
        dz, du, part = R.norm_prelu_bwd(gy, n.detach(), rstd, at.detach(), skip=skip.detach() if with_skip else None)
        assert torch.equal(dz[:, :, 0], torch.zeros_like(dz[:, :, 0])) and torch.equal(dz[:, :, :, -1], torch.zeros_like(dz[:, :, :, -1]))
        assert relerr(dz[:, :, 1:-1, 1:-1], z.grad) <= BOUND
        assert relerr(part.sum().reshape(1), at.grad) <= BOUND
        if with_skip:
            assert relerr(du, skip.grad) <= BOUND
        bad, _, _ = R.norm_prelu_bwd(gy, n.detach(), rstd, at.detach(), skip=skip.detach() if with_skip else None, defect="no_mean")
        assert relerr(bad[:, :, 1:-1, 1:-1], z.grad) > 1e-3           # seeded defect: the norm's mean term dropped


def test_prelu_backward_at_zero_follows_aten():
    """u == 0: ATen passes a * g to the input and adds 0 to the slope."""
    u = torch.tensor([[[[0.0, 1.0, -1.0, 0.0]]]], dtype=torch.float64, requires_grad=True)
    a = torch.tensor([0.3], dtype=torch.float64, requires_grad=True)
    gy = torch.tensor([[[[2.0, 3.0, 5.0, -7.0]]]], dtype=torch.float64)
    F.prelu(u, a).backward(gy)
    pos = u.detach() > 0
    assert torch.equal(u.grad, torch.where(pos, gy, a.detach() * gy))
    assert torch.equal(a.grad, torch.where(pos, torch.zeros_like(gy), u.detach() * gy).sum().reshape(1))


@pytest.mark.parametrize("hw,a", [((9, 7), 0.25), ((3, 2), -0.4), ((6, 8), 0.0)])
def test_residual_block_walk_matches_autograd_through_oracle(hw, a):
    H, W = hw
    sd = _block_sd(5, a=a)
    g = torch.Generator().manual_seed(6)
    x = torch.randn(2, 6, H, W, generator=g, dtype=torch.float64)
    gy = torch.randn(2, 6, H, W, generator=g, dtype=torch.float64)
    leaves = {k: v.clone().requires_grad_() for k, v in sd.items()}
    xl = x.clone().requires_grad_()
    out = O.residual_block(leaves, "b", xl)
    out.backward(gy)
    s = R.residual_block_forward(sd, "b", x)
    assert relerr(s["out"], out.detach()) <= BOUND
    dx, grads = R.residual_block_bwd(sd, "b", s, gy)
    assert relerr(dx, xl.grad) <= BOUND
    for k, v in leaves.items():
        if k.endswith(".bias"):
            # a bias in front of an InstanceNorm has gradient exactly 0 (the norm removes the plane mean): both sides are the
            # rounding residue of a cancelling sum, which has no scale of its own.  Its scale is that of the sum's terms — the
            # same dz summed against inputs of unit order is the layer's dW — so the error is taken against max |dW|.
            dw = leaves[k[:-4] + "weight"].grad
            assert ((grads[k] - v.grad).abs().max() / dw.abs().max()).item() <= BOUND, k
            assert v.grad.abs().max() <= 1e-12 * dw.abs().max()
        else:
            assert relerr(grads[k], v.grad) <= BOUND, k
    if a != 0.0:
        _, one = R.residual_block_bwd(sd, "b", s, gy, defect="one_site")   # seeded defect: the slope taken at one site only
        assert relerr(one["b.prelu.weight"], leaves["b.prelu.weight"].grad) > 1e-3
    bad_dx, bad = R.residual_block_bwd(sd, "b", s, gy, defect="no_fold")
    assert relerr(bad_dx, xl.grad) > 1e-3 and relerr(bad["b.conv1.weight"], leaves["b.conv1.weight"].grad) > 1e-3
    bad_dx, _ = R.residual_block_bwd(sd, "b", s, gy, defect="no_mean")
    assert relerr(bad_dx, xl.grad) > 1e-3


# ================================================================================================ guards without a device
def _warpnet():
    from dvc_amd import synth
    from models.NonlocalNet import WarpNet
    net = WarpNet(1)
    net.load_state_dict(synth.warpnet_state_dict(0))
    return net


def _inputs(N=1, H=48, W=80):
    lab = torch.zeros(N, 3, H, W)
    f = [torch.zeros(N, c, H // s, W // s) for c, s in ((128, 2), (256, 4), (512, 8), (512, 16))]
    return [lab] + f + [t.clone() for t in f]


def test_trunk_parameter_names_are_the_19_of_the_issue():
    net = _warpnet()
    names = [n for n, _ in net._trunk_named_parameters()]
    assert sorted(names) == sorted(TRUNK_NAMES) and len(names) == 19
    assert len(net.state_dict()) == 43
    heads = {n for n, _ in net._head_named_parameters()}
    assert len(heads) == 24 and not heads & set(names)


def test_training_gate():
    net = _warpnet()
    assert not net.eval()._takes_training_path()
    assert net.train()._takes_training_path()
    with torch.no_grad():
        assert not net._takes_training_path()
    for p in net.parameters():
        p.requires_grad = False
    assert not net._takes_training_path()
    net.layer[1].prelu.weight.requires_grad = True
    assert net._takes_training_path()
    net.layer[1].prelu.weight.requires_grad = False
    net.layer2_1[1].weight.requires_grad = True         # a head parameter alone does not open the training path
    assert not net._takes_training_path()


def test_training_path_refuses_cpu_and_unfrozen_heads_and_extras():
    net = _warpnet().train()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        net(*_inputs())
    # (the remaining guards come before any device work; a meta-free way to reach them is the checker itself)
    with pytest.raises(NotImplementedError, match="freeze"):
        net._check_training_call(exemplar_cache=None, return_taps=False, defer_merge=False, detach_flag=False)
    for head in ("layer2_1", "layer3_1", "layer4_1", "layer5_1"):
        for p in getattr(net, head).parameters():
            p.requires_grad = False
    net._check_training_call(exemplar_cache=None, return_taps=False, defer_merge=False, detach_flag=False)
    for kw in (dict(exemplar_cache=(None, None)), dict(return_taps=True), dict(defer_merge=True), dict(detach_flag=True)):
        args = dict(exemplar_cache=None, return_taps=False, defer_merge=False, detach_flag=False)
        args.update(kw)
        with pytest.raises(NotImplementedError):
            net._check_training_call(**args)
    x = _inputs()
    x[1].requires_grad = True
    with pytest.raises((NotImplementedError, RuntimeError)):
        net(*x)


def test_eval_mode_cpu_message_unchanged():
    net = _warpnet().eval()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        net(*_inputs())
