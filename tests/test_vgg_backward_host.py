"""CPU: the host side of VGG19's input gradient and tensor_lab2rgb's gradient — C-ABI validation of the new entry points
(csrc/vgg_bwd.hip), and the weight transforms of the backward packs against F.conv2d's input gradient in float64."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

from cabi_common import _fails, _lib
from oracle import dvc_oracle as O

ONE = ctypes.c_void_p(256)      # a non-null address that is never dereferenced: every call below fails validation first


def test_act_bwd_validation_without_gpu():
    lib = _lib()
    f = lib.dvc_vgg_act_bwd
    _fails(f(ONE, ONE, None, 16, ONE, None), lib, "dvc_vgg_act_bwd")        # no R
    _fails(f(ONE, ONE, ONE, 16, None, None), lib, "dvc_vgg_act_bwd")        # no dZ
    _fails(f(ONE, ONE, ONE, 0, ctypes.c_void_p(512), None), lib, "n > 0")
    _fails(f(ONE, ONE, ONE, -4, ctypes.c_void_p(512), None), lib, "n > 0")
    _fails(f(None, None, ONE, 16, ctypes.c_void_p(512), None), lib, "both null")
    _fails(f(ONE, None, ONE, 16, ONE, None), lib, "alias")                  # dZ == R


def test_pool_act_bwd_validation_without_gpu():
    lib = _lib()
    f = lib.dvc_vgg_pool_act_bwd
    Z = ctypes.c_void_p(1024)
    _fails(f(ONE, None, None, None, 4, 8, 8, 0, Z, None), lib, "bad argument")           # no R
    _fails(f(ONE, None, None, ONE, 4, 8, 8, 0, None, None), lib, "bad argument")         # no dZ
    _fails(f(ONE, None, None, ONE, 0, 8, 8, 0, Z, None), lib, "bad argument")            # no planes
    _fails(f(ONE, None, None, ONE, 4, 1, 8, 0, Z, None), lib, "bad argument")            # H < 2
    _fails(f(ONE, None, None, ONE, 4, 8, 1, 0, Z, None), lib, "bad argument")            # W < 2
    _fails(f(ONE, None, None, ONE, 4, 8, 8, 2, Z, None), lib, "pool_mode")
    _fails(f(None, None, None, ONE, 4, 8, 8, 0, Z, None), lib, "no incoming gradient")
    _fails(f(ONE, None, None, ONE, 4, 8, 8, 1, ONE, None), lib, "alias")


def test_conv1_bwd_validation_without_gpu():
    lib = _lib()
    f = lib.dvc_vgg_conv1_bwd
    X = ctypes.c_void_p(1024)
    _fails(f(None, ONE, 1, 64, 8, 8, X, None), lib, "bad argument")
    _fails(f(ONE, None, 1, 64, 8, 8, X, None), lib, "bad argument")
    _fails(f(ONE, ONE, 1, 64, 8, 8, None, None), lib, "bad argument")
    _fails(f(ONE, ONE, 0, 64, 8, 8, X, None), lib, "bad argument")
    _fails(f(ONE, ONE, 1, 64, 0, 8, X, None), lib, "bad argument")
    _fails(f(ONE, ONE, 1, 60, 8, 8, X, None), lib, "multiple of 8")
    _fails(f(ONE, ONE, 1, 512, 8, 8, X, None), lib, "at most 256")
    _fails(f(ONE, ONE, 70000, 64, 8, 8, X, None), lib, "65535")


def test_lab2rgb_bwd_validation_without_gpu():
    lib = _lib()
    f = lib.dvc_lab2rgb_bwd
    G = ctypes.c_void_p(1024)
    _fails(f(None, 1, 16, 0.0, ONE, G, None), lib, "bad argument")
    _fails(f(ONE, 1, 16, 0.0, None, G, None), lib, "bad argument")
    _fails(f(ONE, 1, 16, 0.0, ONE, None, None), lib, "bad argument")
    _fails(f(ONE, 0, 16, 0.0, ONE, G, None), lib, "bad argument")
    _fails(f(ONE, 1, 0, 0.0, ONE, G, None), lib, "bad argument")
    _fails(f(ONE, 1, 16, 0.0, ONE, ONE, None), lib, "alias")


def test_bwd_weight_gives_conv2d_input_gradient_float64():
    """A 3x3 stride-1 pad-1 layer: conv3x3(dy, vgg_bwd_weight(W)) is F.conv2d's input gradient (odd sizes, Cin != Cout)."""
    from dvc_amd.nets import vgg_bwd_weight
    g = torch.Generator().manual_seed(3)
    w = torch.randn(24, 16, 3, 3, generator=g, dtype=torch.float64)
    b = torch.randn(24, generator=g, dtype=torch.float64)
    x = torch.randn(2, 16, 9, 13, generator=g, dtype=torch.float64, requires_grad=True)
    dy = torch.randn(2, 24, 9, 13, generator=g, dtype=torch.float64)
    (F.conv2d(x, w, b, padding=1) * dy).sum().backward()
    wt = vgg_bwd_weight(w)
    assert wt.shape == (16, 24, 3, 3) and wt.is_contiguous()
    got = F.conv2d(dy, wt, padding=1)
    assert torch.allclose(got, x.grad, rtol=0, atol=1e-12), (got - x.grad).abs().max()


@pytest.mark.parametrize("preprocess", [True, False])
def test_conv1_bwd_weight_folds_vgg_preprocess_float64(preprocess):
    """conv1_1: vgg_bwd_weight_conv1 gives d/d rgb through vgg_preprocess (BGR swap, minus the mean, x255) when preprocess=True,
    d/d x of the plain layer otherwise — the [3][64][3][3] filters ops.vgg_conv1_bwd applies."""
    from dvc_amd import synth
    from dvc_amd.nets import vgg_bwd_weight_conv1
    sd = synth.vgg19_state_dict(0)
    w, b = sd["conv1_1.weight"].double(), sd["conv1_1.bias"].double()
    g = torch.Generator().manual_seed(5)
    x = torch.rand(2, 3, 11, 14, generator=g, dtype=torch.float64, requires_grad=True)
    dy = torch.randn(2, 64, 11, 14, generator=g, dtype=torch.float64)
    xin = O.vgg_preprocess(x) if preprocess else x
    (F.conv2d(xin, w, b, padding=1) * dy).sum().backward()
    wt = vgg_bwd_weight_conv1(w, preprocess)
    assert wt.shape == (3, 64, 3, 3) and wt.is_contiguous()
    got = F.conv2d(dy, wt, padding=1)
    scale = x.grad.abs().max().item()
    assert (got - x.grad).abs().max().item() <= 1e-12 * scale, ((got - x.grad).abs().max(), scale)


def test_vgg_grad_guards_without_gpu():
    """A CPU input is refused before anything else: there is no CPU fallback, with or without grad."""
    import contextlib
    import io
    from models.NonlocalNet import VGG19_pytorch
    with contextlib.redirect_stdout(io.StringIO()):
        m = VGG19_pytorch()
    for p in m.parameters():
        p.requires_grad_(False)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m(torch.rand(1, 3, 8, 8, requires_grad=True), ["r12"])
