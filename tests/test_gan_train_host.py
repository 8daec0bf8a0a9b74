"""CPU: Discriminator_x64's parameter gradients without a device — the hand-written restatement tests/gan_train_reference.py (what
the GPU tests compare against) agrees with an independent float64 autograd composition that spells SpectralNorm literally, to
1e-10 on all 21 gradients and on dx, from the first and from the second of two forwards; it loses that agreement under each of
four seeded defects; the set_parameter_training contract; the refusals of the new C entry points decided before any launch."""
import copy
import ctypes
import functools
import os
import pickle
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gan_reference as R  # noqa: E402
import gan_train_reference as T  # noqa: E402


def _rel(got, ref):
    return (got.double() - ref.double()).abs().max().item() / ref.double().abs().max().item()


@functools.lru_cache(maxsize=None)
def _case(ndf):
    from dvc_amd import synth
    H, W, N = 192, 384, 2
    g = torch.Generator().manual_seed(40 + ndf)
    sd = synth.discriminator_state_dict(1, ndf=ndf)
    x = torch.randn(N, 6, H, W, generator=g)
    g_out, g_f4 = torch.randn(N, 1, generator=g), torch.randn(N, 4 * ndf, H // 16, W // 16, generator=g)
    c1 = R.forward(sd, x)[2]
    sd2 = T.advance(sd, c1)
    return sd, x, g_out, g_f4, c1, sd2, R.forward(sd2, x)[2]


SEEDS = {"output": (True, False), "feature4": (False, True), "both": (True, True)}


def _errors(got, ref):
    """{name: relative error} (against T.param_grads' scale where it gives one); a gradient no seeded output reaches must be
    zero."""
    (dx, grads, scale), (dx_a, grads_a) = got, ref
    err = {"dx": _rel(dx, dx_a)}
    assert set(grads) == set(grads_a) == set(T.PARAM_NAMES) and len(grads) == 21
    for n in T.PARAM_NAMES:
        assert grads[n].shape == grads_a[n].shape, n
        if n in scale:
            err[n] = (grads[n] - grads_a[n]).abs().max().item() / scale[n]
        elif grads_a[n].abs().max() == 0:
            err[n] = grads[n].abs().max().item()
        else:
            err[n] = _rel(grads[n], grads_a[n])
    return err


@pytest.mark.parametrize("which", list(SEEDS))
@pytest.mark.parametrize("ndf", [2, 8])
def test_restatement_matches_float64_autograd(ndf, which):
    sd, x, g_out, g_f4, c1, sd2, c2 = _case(ndf)
    go, gf = (t if on else None for t, on in zip((g_out, g_f4), SEEDS[which]))
    ref = T.autograd_grads(sd, x, go, gf)
    assert all(ref[1][n].abs().max() > 0 for n in T.PARAM_NAMES if SEEDS[which][0] or n.startswith(("layer1", "layer2", "layer3", "layer4")))
    if SEEDS[which][0]:     # the key bias gradient is rounding noise around an exact zero
        assert ref[1]["attention.key_conv.module.bias"].abs().max() <= 1e-12 * ref[1]["attention.query_conv.module.bias"].abs().max()
    err = _errors(T.param_grads(sd, c1, x, go, gf), ref)
    assert max(err.values()) <= 1e-10, err
    # gradients taken from forward #2 of two: sigma of the second forward is made of the vectors the SECOND power step left
    err2 = _errors(T.param_grads(sd2, c2, x, go, gf), T.autograd_grads(sd, x, go, gf, forwards=2))
    assert max(err2.values()) <= 1e-10, err2


@pytest.mark.parametrize("forwards", [1, 2])
@pytest.mark.parametrize("defect,where", [("no_sigma_grad", "weight_bar"), ("stale_uv", "weight_bar"), ("tap", "weight_bar"),
                                          ("gamma_x", "attention.gamma")])
def test_seeded_defects_are_caught(defect, where, forwards):
    """Each defect moves at least one named tensor by more than 1e-3 — with the synthetic state_dict (u, v freshly drawn, as a new
    module has them) the rank-one term is not small and one power step moves u, v far; so also from the second forward, where
    "stale_uv" means the vectors the FIRST forward left (what a module that kept no copies per forward would read)."""
    sd, x, g_out, g_f4, c1, sd2, c2 = _case(2)
    ref = T.autograd_grads(sd, x, g_out, g_f4, forwards=forwards)
    err = _errors(T.param_grads(*((sd, c1) if forwards == 1 else (sd2, c2)), x, g_out, g_f4, defect=defect), ref)
    worst = max(err, key=err.get)
    assert err[worst] > 1e-3 and worst.endswith(where), (defect, worst, err[worst])
    if defect != "stale_uv":
        assert err["dx"] <= 1e-10         # (none of these touches the input gradient)


def test_discriminator_loss_seeds_are_the_gradient_of_the_loss():
    g = torch.Generator().manual_seed(9)
    r, f = (torch.randn(4, 1, generator=g, dtype=torch.float64).requires_grad_(True) for _ in range(2))
    T.relativistic_ls_loss(r, f).backward()
    gr, gf = T.relativistic_ls_seeds(r.detach(), f.detach())
    assert _rel(gr, r.grad) <= 1e-14 and _rel(gf, f.grad) <= 1e-14


def test_set_parameter_training_contract():
    from dvc_amd.gan import Discriminator_x64
    net = Discriminator_x64(ndf=2)
    x = torch.zeros(1, 6, 192, 384)
    assert net.parameter_training is False
    with pytest.raises(NotImplementedError, match="parameter gradients are not built yet"):
        net(x)                                              # flag off: the old refusal
    assert net.set_parameter_training() is net and net.parameter_training is True
    assert not any("training" in k for k in net.state_dict()) and len(net.state_dict()) == 41
    assert copy.deepcopy(net).parameter_training is True and pickle.loads(pickle.dumps(net)).parameter_training is True
    assert len(net._trainable_named_parameters()) == 21 and sorted(n for n, _ in net._trainable_named_parameters()) == sorted(T.PARAM_NAMES)
    assert all(p.requires_grad for _, p in net._trainable_named_parameters())
    with pytest.raises(RuntimeError, match="no CPU fallback") as e:
        net(x)                                              # flag on: nothing left to refuse but the CPU tensor
    assert not isinstance(e.value, NotImplementedError)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        net(x.clone().requires_grad_(True))
    assert net.set_parameter_training(False) is net and net.parameter_training is False
    assert copy.deepcopy(net).parameter_training is False
    with pytest.raises(NotImplementedError, match="parameter gradients are not built yet"):
        net(x)
    fresh = Discriminator_x64(ndf=2)
    fresh.load_state_dict(net.set_parameter_training().state_dict())       # the flag does not travel with the state_dict
    assert fresh.parameter_training is False


def _desc(**kw):
    from dvc_amd import ops
    base = dict(N=1, Cin=6, H=8, W=8, Cout=8, ksize=4, stride=2, pad=1, act=ops.ACT_LEAKY, act_slope=0.2)
    base.update(kw)
    N, Cin, H, W, Cout = (base.pop(k) for k in ("N", "Cin", "H", "W", "Cout"))
    return ops._conv_desc(N, Cin, H, W, Cout, **base)


def test_new_c_entry_points_refuse_before_any_launch():
    from dvc_amd import _lib
    lib = _lib.load()
    a, b, c, d = (ctypes.c_void_p(64 * k) for k in (1, 2, 3, 4))
    ld = 8 * 6 * 16 + 8

    def refused(rc, text):
        assert rc != 0 and text in lib.dvc_last_error().decode(), lib.dvc_last_error()

    wg = lib.dvc_gan_conv4s2_wgrad
    for bad in (dict(ksize=3), dict(stride=1), dict(pad=0)):
        refused(wg(ctypes.byref(_desc(**bad)), a, b, 1, c, ld, d, None), "4x4 stride-2")
        assert lib.dvc_gan_conv4s2_wgrad_splits(ctypes.byref(_desc(**bad))) == 0
    refused(wg(ctypes.byref(_desc(H=1)), a, b, 1, c, ld, d, None), "bad shape")
    refused(wg(ctypes.byref(_desc(Cin=0)), a, b, 1, c, ld, d, None), "bad shape")
    refused(wg(ctypes.byref(_desc(x_batch_stride=6 * 64 - 1)), a, b, 1, c, ld, d, None), "x_batch_stride")
    refused(wg(ctypes.byref(_desc(y_batch_stride=8 * 16 - 1)), a, b, 1, c, ld, d, None), "y_batch_stride")
    refused(wg(None, a, b, 1, c, ld, d, None), "null descriptor")
    for args in ((None, b, 1, c, ld, d), (a, None, 1, c, ld, d), (a, b, 1, None, ld, d), (a, b, 1, c, ld, None)):
        refused(wg(ctypes.byref(_desc()), *args, None), "null argument")
    refused(wg(ctypes.byref(_desc()), ctypes.c_void_p(66), b, 1, c, ld, d, None), "4-byte aligned")
    for S in (0, -1, 65536):
        refused(wg(ctypes.byref(_desc()), a, b, S, c, 65536 * ld, d, None), "S must be in [1, 65535]")
    refused(wg(ctypes.byref(_desc()), a, b, 1, c, ld - 1, d, None), "workspace too small")
    refused(wg(ctypes.byref(_desc()), a, b, 3, c, 3 * ld - 1, d, None), "workspace too small")
    for args in ((a, b, 1, c, ld, a), (a, b, 1, c, ld, b), (a, b, 1, a, ld, d), (a, b, 1, b, ld, d), (a, b, 1, c, ld, c)):
        refused(wg(ctypes.byref(_desc()), *args, None), "must not alias")
    assert lib.dvc_gan_conv4s2_wgrad_splits(ctypes.byref(_desc())) == 1        # one chunk of 16 pixels: nothing to split
    assert lib.dvc_gan_conv4s2_wgrad_splits(ctypes.byref(_desc(N=16, H=216, W=384, Cout=64))) == 512       # layer1: all from S
    assert lib.dvc_gan_conv4s2_wgrad_splits(ctypes.byref(_desc(N=16, Cin=1024, H=6, W=12, Cout=1024))) == 1   # layer6: all from tiles

    nb = lib.dvc_gan_dot_workspace_bytes(8 * 96)
    assert nb == 8 and lib.dvc_gan_dot_workspace_bytes(0) == 0 and lib.dvc_gan_dot_workspace_bytes(1 << 30) == 1024 * 8
    sn = lib.dvc_gan_sn_wgrad
    for i in range(5):
        args = [a, a, a, a, a]
        args[i] = None
        refused(sn(*args, 8, 96, b, c, nb, None), "null argument")
    refused(sn(a, a, a, a, a, 8, 96, None, c, nb, None), "null argument")
    refused(sn(a, a, a, a, a, 0, 96, b, c, nb, None), "bad shape")
    refused(sn(a, a, a, a, a, 8, 0, b, c, nb, None), "bad shape")
    refused(sn(a, a, a, a, a, 8, 96, b, c, nb - 1, None), "workspace too small")
    refused(sn(a, a, a, a, a, 8, 96, b, None, 1 << 20, None), "workspace too small")
    refused(sn(a, a, a, a, a, 8, 96, b, ctypes.c_void_p(68), nb, None), "8-byte aligned")
    refused(sn(a, d, d, d, d, 8, 96, a, c, nb, None), "must not alias")
    refused(sn(d, a, d, d, d, 8, 96, a, c, nb, None), "must not alias")

    lw = lib.dvc_gan_last_wgrad
    refused(lw(a, b, 1, 16, 2, 6, 0, c, None), "smaller than the 3 x 6 filter")
    refused(lw(a, b, 1, 16, 3, 5, 0, c, None), "smaller than the 3 x 6 filter")
    refused(lw(a, b, 0, 16, 3, 6, 0, c, None), "bad shape")
    refused(lw(a, b, 1, 16, 3, 6, 16 * 18 - 1, c, None), "x_batch_stride")
    refused(lw(None, b, 1, 16, 3, 6, 0, c, None), "null argument")
    refused(lw(a, b, 1, 16, 3, 6, 0, b, None), "must not alias")

    dot = lib.dvc_gan_dot
    refused(dot(a, None, 8, c, d, 8, None), "null argument")
    refused(dot(a, b, 0, c, d, 8, None), "bad count")
    refused(dot(a, b, 8, c, d, 7, None), "workspace too small")
    refused(dot(a, b, 8, a, d, 8, None), "must not alias")
