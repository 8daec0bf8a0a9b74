"""CPU: the host side of WarpNet's backward through its four heads (WarpNet.set_head_training) — header / ctypes table / export
agreement and the pre-launch refusals of the new entry points (csrc/warp_head_bwd.hip), the float64 restatements of every new
launch kind (tests/warp_head_bwd_reference.py) against float64 autograd through oracle.dvc_oracle to 1e-12 relative (the bound
of tests/test_warp_backward_host.py), one seeded defect per restatement that must break that bound, and the opt-in gate."""
import copy
import ctypes
import os
import pickle
import re
import subprocess

import pytest
import torch
import torch.nn.functional as F

import warp_bwd_reference as R
import warp_head_bwd_reference as RH
from bwd_audit import relerr
from cabi_common import _fails, _lib
from oracle import dvc_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ONE, TWO, THREE = ctypes.c_void_p(256), ctypes.c_void_p(1024), ctypes.c_void_p(4096)    # never dereferenced
NEW = ["dvc_warp_head_wgrad_splits", "dvc_warp_head_wgrad", "dvc_warp_dilate_ring", "dvc_warp_up2_bwd", "dvc_warp_rpad_rows_bwd"]
BOUND = 1e-12
HEADS = ("layer2_1", "layer3_1", "layer4_1", "layer5_1")


# ================================================================================================ C-ABI
def test_new_entry_points_in_header_table_and_exports():
    from dvc_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "dvc_hip.h")).read()
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    for name in NEW:
        assert re.search(r"\b%s\(" % name, hdr), name
        assert name in _lib.SIGNATURES, name
        assert re.search(r"\b%s\b" % name, out), name
    assert _lib.load().dvc_abi_version() == _lib.ABI_VERSION == 20


def test_validation_without_gpu():
    lib = _lib()
    big = 1 << 40
    f = lib.dvc_warp_head_wgrad          # (dz_ringed, x_padded, N, Cin, Cout, H, W, stride, S, part, part_floats, out, stream)
    _fails(f(None, ONE, 1, 8, 8, 4, 4, 2, 1, TWO, big, THREE, None), lib, "null pointer")
    _fails(f(ONE, TWO, 1, 8, 8, 4, 4, 2, 1, None, big, THREE, None), lib, "null pointer")
    _fails(f(ONE, TWO, 1, 8, 0, 4, 4, 2, 1, THREE, big, ONE, None), lib, "bad size")
    _fails(f(ONE, TWO, 1, 8, 8, 1, 4, 2, 1, THREE, big, ONE, None), lib, "bad size")
    _fails(f(ONE, TWO, 1, 8, 8, 4, 4, 3, 1, THREE, big, ctypes.c_void_p(8192), None), lib, "stride must")
    _fails(f(ONE, TWO, 1, 8, 8, 4, 4, 2, 0, THREE, big, ctypes.c_void_p(8192), None), lib, "S must")
    _fails(f(ONE, TWO, 1, 8, 8, 4, 4, 2, 2, THREE, 10, ctypes.c_void_p(8192), None), lib, "workspace too small")
    _fails(f(ONE, TWO, 1, 8, 8, 4, 4, 2, 1, THREE, big, ONE, None), lib, "alias")
    _fails(f(ONE, TWO, 1, 8, 8, 4, 4, 2, 1, TWO, big, THREE, None), lib, "alias")
    s = lib.dvc_warp_head_wgrad_splits
    assert s(0, 8, 8, 4, 4, 2) == 0 and s(1, 8, 8, 4, 4, 3) == 0 and s(1, 8, 8, 1, 4, 1) == 0
    assert s(4, 128, 64, 24, 40, 2) == 24          # 2 tiles, 4 * 12 * 2 chunks: at least four chunks per slot
    assert s(4, 128, 64, 24, 40, 1) == 72
    assert s(1, 512, 256, 2, 3, 1) == 1
    f = lib.dvc_warp_dilate_ring         # (dz_ringed, planes, Ho, Wo, H, W, out, stream)
    _fails(f(None, 1, 4, 5, 7, 9, TWO, None), lib, "null pointer")
    _fails(f(ONE, 0, 4, 5, 7, 9, TWO, None), lib, "bad size")
    _fails(f(ONE, 1, 3, 5, 7, 9, TWO, None), lib, "not the stride-2 output size")      # 7 rows give 4, not 3
    _fails(f(ONE, 1, 4, 4, 7, 9, TWO, None), lib, "not the stride-2 output size")
    _fails(f(ONE, 1, 4, 5, 7, 9, ONE, None), lib, "alias")
    f = lib.dvc_warp_up2_bwd             # (g, planes, h, w, out, stream)
    _fails(f(ONE, 1, 2, 2, None, None), lib, "null pointer")
    _fails(f(ONE, 1, 0, 2, TWO, None), lib, "bad size")
    _fails(f(ONE, 1, 2, 2, ONE, None), lib, "alias")
    f = lib.dvc_warp_rpad_rows_bwd       # (g, planes, h, w, rpad, out, stream)
    _fails(f(None, 1, 2, 2, 1, TWO, None), lib, "null pointer")
    _fails(f(ONE, 1, 2, 2, 0, TWO, None), lib, "bad size")
    _fails(f(ONE, 1, 2, 0, 1, TWO, None), lib, "bad size")
    _fails(f(ONE, 1, 2, 2, 1, ONE, None), lib, "alias")


# ================================================================================================ float64 restatements vs autograd
def _rand(shape, g, requires_grad=False):
    return torch.randn(*shape, generator=g, dtype=torch.float64, requires_grad=requires_grad)


@pytest.mark.parametrize("stride,hw", [(2, (7, 9)), (2, (8, 10)), (2, (2, 3)), (2, (3, 2)), (1, (2, 3)), (1, (6, 5))])
def test_strided_wgrad_and_input_gradient_match_autograd(stride, hw):
    """ReflectionPad2d(1) + Conv2d(3, stride): the strided weight gradient on the padded copy, and dilate-ring + zero-pad
    convolution with W^T flipped + fold as its input gradient."""
    H, W = hw
    g = torch.Generator().manual_seed(7)
    w, b, x = _rand((5, 4, 3, 3), g, True), _rand((5,), g, True), _rand((2, 4, H, W), g, True)
    Ho, Wo = RH.out_hw(H, W, stride)
    dz = _rand((2, 5, Ho, Wo), g)
    O._rconv(x, w, b, stride=stride).backward(dz)
    dW, db = RH.head_wgrad(R.ring(dz), R.reflect_pad(x.detach()), stride)
    assert relerr(dW, w.grad) <= BOUND and relerr(db, b.grad) <= BOUND
    spread = RH.dilate_ring(R.ring(dz), H, W) if stride == 2 else R.ring(dz)
    assert tuple(spread.shape[2:]) == (H + 2, W + 2)
    assert relerr(R.fold(R.padded_input_grad(spread, w.detach())), x.grad) <= BOUND
    if stride == 2 and (H % 2 or W % 2):            # seeded defect: the odd-size tail dropped
        bad, _ = RH.head_wgrad(R.ring(dz), R.reflect_pad(x.detach()), stride, defect="odd_tail")
        assert relerr(bad, w.grad) > 1e-3
        bad = RH.dilate_ring(R.ring(dz), H, W, defect="odd_tail")
        assert relerr(R.fold(R.padded_input_grad(bad, w.detach())), x.grad) > 1e-3


def test_up2_bwd_matches_autograd():
    g = torch.Generator().manual_seed(8)
    x, gy = _rand((2, 3, 5, 7), g, True), _rand((2, 3, 10, 14), g)
    F.interpolate(x, scale_factor=2, mode="nearest").backward(gy)
    assert relerr(RH.up2_bwd(gy), x.grad) <= BOUND
    assert relerr(RH.up2_bwd(gy, defect="block_index"), x.grad) > 1e-3          # seeded defect: the wrong block elements


@pytest.mark.parametrize("h,rpad", [(8, 1), (1, 1), (2, 1), (3, 2)])
def test_rpad_rows_bwd_matches_autograd(h, rpad):
    g = torch.Generator().manual_seed(9)
    x, gy = _rand((2, 3, h, 5), g, True), _rand((2, 3, h + 2 * rpad, 5), g)
    F.pad(x, (0, 0, rpad, rpad), "replicate").backward(gy)
    assert relerr(RH.rpad_rows_bwd(gy, rpad), x.grad) <= BOUND
    assert relerr(RH.rpad_rows_bwd(gy, rpad, defect="no_edge"), x.grad) > 1e-3  # seeded defect: the edge rows' share dropped


def _head_sd(name, seed, cin=6, mid=5, cout=4):
    from dvc_amd import arch
    hd = arch.WARP_HEAD_PLAN[arch.WARP_HEAD_ORDER.index(name)]
    g = torch.Generator().manual_seed(seed)
    sd = {f"{name}.{hd.conv_a}.weight": _rand((mid, cin, 3, 3), g) * 0.3, f"{name}.{hd.conv_a}.bias": _rand((mid,), g),
          f"{name}.{hd.conv_b}.weight": _rand((cout, mid, 3, 3), g) * 0.3, f"{name}.{hd.conv_b}.bias": _rand((cout,), g),
          f"{name}.{hd.prelu_a}.weight": torch.tensor([0.25], dtype=torch.float64),
          f"{name}.{hd.prelu_b}.weight": torch.tensor([-0.4], dtype=torch.float64)}
    return hd, sd


@pytest.mark.parametrize("name,hw,rpad,defect", [
    ("layer2_1", (7, 9), 0, "odd_tail"), ("layer2_1", (8, 10), 0, None), ("layer2_1", (2, 3), 0, "odd_tail"),
    ("layer3_1", (5, 4), 0, None), ("layer4_1", (3, 5), 0, "block_index"), ("layer5_1", (2, 3), 1, "no_edge"),
    ("layer5_1", (2, 4), 0, "block_index")])
def test_head_walk_matches_autograd_through_oracle(name, hw, rpad, defect):
    """All six gradients of one head, walked launch by launch as WarpNet._heads_backward does, against autograd through
    oracle.warp_head (+ the replicated rows of layer5_1)."""
    hd, sd = _head_sd(name, 10)
    g = torch.Generator().manual_seed(11)
    x = _rand((2, 6) + hw, g)
    leaves = {k: v.clone().requires_grad_() for k, v in sd.items()}
    out = O.warp_head(leaves, name, x)
    if rpad:
        out = F.pad(out, (0, 0, rpad, rpad), "replicate")
    gy = _rand(tuple(out.shape), g)
    out.backward(gy)
    s = RH.head_forward(sd, hd, x)
    assert relerr(F.pad(s["out"], (0, 0, rpad, rpad), "replicate") if rpad else s["out"], out.detach()) <= BOUND
    grads = RH.head_bwd(sd, hd, s, gy, rpad=rpad)
    assert sorted(grads) == sorted(leaves)
    for k, v in leaves.items():
        if k.endswith(".bias"):     # in front of an InstanceNorm: true gradient 0, taken against its layer's dW (see
            dw = leaves[k[:-4] + "weight"].grad     # tests/test_warp_backward_host.py)
            assert ((grads[k] - v.grad).abs().max() / dw.abs().max()).item() <= BOUND, k
        else:
            assert relerr(grads[k], v.grad) <= BOUND, k
    if defect is not None:
        bad = RH.head_bwd(sd, hd, s, gy, rpad=rpad, defect=defect)
        first = f"{name}.{hd.conv_a}.weight"
        assert relerr(bad[first], leaves[first].grad) > 1e-3, defect


# ================================================================================================ the opt-in gate
def _warpnet():
    from dvc_amd import synth
    from models.NonlocalNet import WarpNet
    net = WarpNet(1)
    net.load_state_dict(synth.warpnet_state_dict(0))
    return net


ARGS = dict(exemplar_cache=None, return_taps=False, defer_merge=False, detach_flag=False)


def test_default_is_off_and_pinned_behaviour_holds():
    net = _warpnet().train()
    assert net.head_training is False
    with pytest.raises(AttributeError):
        net.head_training = True                    # read-only: set_head_training is the switch
    with pytest.raises(NotImplementedError, match="freeze"):
        net._check_training_call(**ARGS)
    for p in net.parameters():
        p.requires_grad = False
    net.layer2_1[1].weight.requires_grad = True     # a head parameter alone does not open the training path
    assert not net._takes_training_path()
    assert net.set_head_training(True).set_head_training(False) is net and not net._takes_training_path()


def test_opt_in_gate():
    net = _warpnet().train()
    assert net.set_head_training() is net and net.head_training is True
    assert len([p for p in net.parameters() if p.requires_grad]) == 43
    net._check_training_call(**ARGS)                # all 43 unfrozen: accepted
    for kw in (dict(exemplar_cache=(None, None)), dict(return_taps=True), dict(defer_merge=True), dict(detach_flag=True)):
        with pytest.raises(NotImplementedError):
            net._check_training_call(**dict(ARGS, **kw))
    for p in net.parameters():
        p.requires_grad = False
    assert not net._takes_training_path()
    net.layer5_1[8].weight.requires_grad = True     # a head parameter alone opens it
    assert net._takes_training_path()
    with torch.no_grad():
        assert not net._takes_training_path()
    assert not net.eval()._takes_training_path()
    net.train()
    net.layer5_1[8].weight.requires_grad = False
    net.theta.bias.requires_grad = True
    assert net._takes_training_path()
    x = [torch.zeros(1, 3, 48, 80)] + [torch.zeros(1, c, 48 // s, 80 // s) for c, s in ((128, 2), (256, 4), (512, 8), (512, 16))] * 2
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        net(*x)


def test_flag_is_not_state_and_survives_copies():
    net = _warpnet()
    keys = list(net.state_dict())
    net.set_head_training(True)
    assert list(net.state_dict()) == keys and len(keys) == 43 and not any("head_training" in k for k in keys)
    assert copy.deepcopy(net).head_training is True
    assert pickle.loads(pickle.dumps(net)).head_training is True
    fresh = _warpnet()
    fresh.load_state_dict(net.state_dict())
    assert fresh.head_training is False
    assert copy.deepcopy(fresh).head_training is False
