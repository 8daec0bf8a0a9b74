"""CPU: the host side of ColorVidNet's backward — C-ABI validation of the new entry points (csrc/cvn_bwd.hip), header / ctypes
table / export agreement, the input-gradient filter transforms and a float64 restatement of the InstanceNorm backward against
autograd, and the gate that decides which calls take the training path."""
import contextlib
import ctypes
import io
import os
import re
import subprocess

import pytest
import torch
import torch.nn.functional as F

from cabi_common import _fails, _lib
from bwd_audit import ref_inorm_bwd as _inorm_bwd64      # (the float64 restatement of dvc_cvn_inorm_bwd; the audit uses it too)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ONE = ctypes.c_void_p(256)      # a non-null address that is never dereferenced: every call below fails validation first
NEW = ["dvc_cvn_wgrad_splits", "dvc_cvn_wgrad", "dvc_cvn_head_bwd_workspace_floats", "dvc_cvn_head_bwd", "dvc_cvn_inorm_bwd"]


def test_new_entry_points_in_header_table_and_exports():
    from dvc_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "dvc_hip.h")).read()
    so = _lib.LIB_PATH
    out = subprocess.run(["nm", "-D", "--defined-only", so], capture_output=True, text=True).stdout
    for name in NEW:
        assert re.search(r"\b%s\(" % name, hdr), name
        assert name in _lib.SIGNATURES, name
        assert re.search(r"\b%s\b" % name, out), name
    _lib.load()


def test_wgrad_validation_without_gpu():
    lib = _lib()
    f = lib.dvc_cvn_wgrad
    P, O_ = ctypes.c_void_p(1024), ctypes.c_void_p(2048)
    big = 1 << 40
    _fails(f(None, ONE, 1, 8, 8, 4, 4, 1, 1, 1, P, big, O_, None), lib, "null pointer")
    _fails(f(ONE, ONE, 1, 8, 8, 4, 4, 1, 1, 1, None, big, O_, None), lib, "null pointer")
    _fails(f(ONE, ONE, 0, 8, 8, 4, 4, 1, 1, 1, P, big, O_, None), lib, "bad size")
    _fails(f(ONE, ONE, 1, 0, 8, 4, 4, 1, 1, 1, P, big, O_, None), lib, "bad size")
    _fails(f(ONE, ONE, 1, 8, -1, 4, 4, 1, 1, 1, P, big, O_, None), lib, "bad size")
    _fails(f(ONE, ONE, 1, 8, 8, 4, 4, 3, 1, 1, P, big, O_, None), lib, "dil")
    _fails(f(ONE, ONE, 1, 8, 8, 4, 4, 1, 4, 1, P, big, O_, None), lib, "in_up")
    _fails(f(ONE, ONE, 1, 8, 8, 5, 4, 1, 2, 1, P, big, O_, None), lib, "even")
    _fails(f(ONE, ONE, 1, 8, 8, 4, 4, 1, 1, 0, P, big, O_, None), lib, "S must")
    _fails(f(ONE, ONE, 1, 8, 8, 4, 4, 1, 1, 2, P, 10, O_, None), lib, "workspace too small")
    _fails(f(ONE, ONE, 1, 8, 8, 4, 4, 1, 1, 1, P, big, ONE, None), lib, "alias")
    assert lib.dvc_cvn_wgrad_splits(0, 8, 8, 4, 4) == 0
    assert lib.dvc_cvn_wgrad_splits(1, 512, 512, 27, 48) >= 1


def test_head_bwd_validation_without_gpu():
    lib = _lib()
    f = lib.dvc_cvn_head_bwd
    Z, P, O_ = ctypes.c_void_p(1024), ctypes.c_void_p(2048), ctypes.c_void_p(4096)
    big = 1 << 40
    _fails(f(None, ONE, ONE, ONE, 1, 128, 64, 0.2, Z, P, big, O_, None), lib, "null pointer")
    _fails(f(ONE, ONE, ONE, ONE, 1, 128, 64, 0.2, None, P, big, O_, None), lib, "null pointer")
    _fails(f(ONE, ONE, ONE, ONE, 0, 128, 64, 0.2, Z, P, big, O_, None), lib, "bad size")
    _fails(f(ONE, ONE, ONE, ONE, 1, 0, 64, 0.2, Z, P, big, O_, None), lib, "bad size")
    _fails(f(ONE, ONE, ONE, ONE, 1, 128, 64, 0.2, Z, P, 3, O_, None), lib, "workspace too small")
    _fails(f(ONE, ONE, ONE, ONE, 1, 128, 64, 0.2, ONE, P, big, O_, None), lib, "alias")
    assert lib.dvc_cvn_head_bwd_workspace_floats(2, 128, 300) == 2 * 2 * 258
    assert lib.dvc_cvn_head_bwd_workspace_floats(0, 128, 300) == 0


def test_inorm_bwd_validation_without_gpu():
    lib = _lib()
    f = lib.dvc_cvn_inorm_bwd
    Z = ctypes.c_void_p(1024)
    _fails(f(None, ONE, ONE, ONE, None, None, None, 1, 4, 8, 8, Z, None, None, None), lib, "null pointer")
    _fails(f(ONE, ONE, ONE, ONE, None, None, None, 1, 4, 8, 8, None, None, None, None), lib, "null pointer")
    _fails(f(ONE, ONE, ONE, ONE, None, None, None, 1, 0, 8, 8, Z, None, None, None), lib, "bad size")
    _fails(f(ONE, ONE, ONE, None, None, None, None, 1, 4, 8, 8, Z, None, None, None), lib, "no incoming gradient")
    _fails(f(ONE, ONE, ONE, None, ONE, None, None, 1, 4, 8, 8, Z, None, None, None), lib, "g_ss needs")
    _fails(f(ONE, ONE, ONE, ONE, None, None, None, 1, 4, 8, 8, ONE, None, None, None), lib, "alias")


@pytest.mark.parametrize("dil,in_up", [(1, 1), (2, 1), (1, 2)])
def test_transposed_filters_give_the_input_gradient(dil, in_up):
    """conv3x3(dZ, cvn_bwd_weight(W), dil) == d/dX conv2d(X, W, pad=dil, dil) in float64; for in_up = 2 the full-resolution
    gradient summed over 2x2 is the gradient of the half-resolution map."""
    from dvc_amd.nets import cvn_bwd_weight
    g = torch.Generator().manual_seed(1)
    Cin, Cout, H, W = 5, 6, 10, 12
    w = torch.randn(Cout, Cin, 3, 3, generator=g, dtype=torch.float64)
    dZ = torch.randn(2, Cout, H, W, generator=g, dtype=torch.float64)
    full = F.conv2d(dZ, cvn_bwd_weight(w), padding=dil, dilation=dil)
    ref = torch.nn.grad.conv2d_input((2, Cin, H, W), w, dZ, padding=dil, dilation=dil)
    assert torch.allclose(full, ref, rtol=1e-12, atol=1e-12)
    if in_up == 2:
        xs = torch.randn(2, Cin, H // 2, W // 2, generator=g, dtype=torch.float64, requires_grad=True)
        y = F.conv2d(F.interpolate(xs, scale_factor=2, mode="nearest"), w, padding=dil, dilation=dil)
        (gx,) = torch.autograd.grad(y, xs, dZ)
        assert torch.allclose(F.avg_pool2d(full, 2) * 4, gx, rtol=1e-12, atol=1e-12)
    padded = cvn_bwd_weight(w, pad_to=8)
    assert padded.shape == (8, Cout, 3, 3) and torch.equal(padded[:Cin], cvn_bwd_weight(w)) and not padded[Cin:].any()


@pytest.mark.parametrize("H,W", [(12, 16), (9, 7)])
def test_inorm_backward_restatement_vs_autograd(H, W):
    g = torch.Generator().manual_seed(2)
    B, C = 2, 3
    pre = torch.randn(B, C, H, W, generator=g, dtype=torch.float64, requires_grad=True)
    ss_w = torch.randn(C, generator=g, dtype=torch.float64, requires_grad=True)
    R = F.relu(pre)
    n = F.instance_norm(R, eps=1e-5)
    gf = torch.randn(B, C, H, W, generator=g, dtype=torch.float64)
    gs = torch.randn(B, C, (H + 1) // 2, (W + 1) // 2, generator=g, dtype=torch.float64)
    gu = torch.randn(B, C, 2 * H, 2 * W, generator=g, dtype=torch.float64)
    loss = (n * gf).sum() + (F.conv2d(n, ss_w.view(C, 1, 1, 1), stride=2, groups=C) * gs).sum() \
        + (F.interpolate(n, scale_factor=2, mode="nearest") * gu).sum()
    loss.backward()
    var = R.detach().var((2, 3), unbiased=False, keepdim=True)
    dx, dss = _inorm_bwd64(n.detach(), 1 / torch.sqrt(var + 1e-5), R.detach(), gf, gs, ss_w.detach(), gu)
    assert torch.allclose(dx, pre.grad, rtol=1e-10, atol=1e-10)
    assert torch.allclose(dss, ss_w.grad, rtol=1e-10, atol=1e-10)


class _CudaLike:
    def __init__(self, x):
        self.is_cuda, self.requires_grad = True, x.requires_grad


@pytest.fixture
def gate(monkeypatch):
    """A ColorVidNet whose two paths are stubs (no GPU needed): which one a call takes is the question.  The input check is the
    real one with the device test passed (the stub input lives on the CPU)."""
    from dvc_amd import nets
    real = nets._check_input
    with contextlib.redirect_stdout(io.StringIO()):
        m = nets.ColorVidNet(7)
    monkeypatch.setattr(nets.ColorVidNet, "_forward", lambda self, x, saved=None, rstd=None: "infer")
    monkeypatch.setattr(nets.ColorVidNet, "_forward_with_grad", lambda self, x: "train")
    monkeypatch.setattr(nets, "_check_input", lambda x, name: real(_CudaLike(x), name))
    return m


@pytest.mark.parametrize("train,grad_mode,x_grad,p_grad,expect", [
    (True, True, False, True, "train"),        # train.py: parameters require grad
    (True, True, True, False, "train"),        # only the input requires grad
    (True, True, False, False, "infer"),       # nothing requires grad
    (True, False, True, True, "infer"),        # torch.no_grad()
    (False, True, False, True, "infer"),       # eval: no history (as before)
    (False, True, True, True, "raise"),        # eval + grad-requiring input: still refused
    (False, False, True, True, "infer"),
])
def test_training_path_gate(gate, train, grad_mode, x_grad, p_grad, expect):
    m = gate
    m.train(train)
    for p in m.parameters():
        p.requires_grad = p_grad
    x = torch.zeros(1, 7, 4, 4, requires_grad=x_grad)
    with torch.set_grad_enabled(grad_mode):
        if expect == "raise":
            with pytest.raises(NotImplementedError, match="training mode"):
                m(x)
        else:
            assert m(x) == expect
