"""CPU: Discriminator_x64 (dvc_amd/gan.py) without a device — the float64 restatement tests/gan_reference.py (what the GPU tests
compare against) agrees with float64 autograd through nn.Conv2d / softmax to 1e-12 on both outputs and the input gradient, and
loses that agreement under each seeded defect; the state_dict contract; the refusals of the module and of the C entry points that
are decided before any launch; the conditioning of the attention inputs the GPU tests use."""
import ctypes
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gan_reference as R  # noqa: E402


def _rel(got, ref):
    return (got.double() - ref.double()).abs().max().item() / ref.double().abs().max().item()


def _case(ndf=4, H=216, W=384, N=1, seed=0):
    from dvc_amd import synth
    g = torch.Generator().manual_seed(seed)
    sd = synth.discriminator_state_dict(seed, ndf=ndf)
    x = torch.randn(N, 6, H, W, generator=g)
    h4, w4 = H // 16, W // 16
    return sd, x, torch.randn(N, 1, generator=g), torch.randn(N, 4 * ndf, h4, w4, generator=g)


@pytest.fixture(scope="module")
def case():
    sd, x, g_out, g_f4 = _case()            # 216 -> 108 -> 54 -> 27 -> 13 -> 6 -> 3: two odd maps
    return sd, x, g_out, g_f4, R.autograd_composition(sd, x, g_out, g_f4)


def test_restatement_matches_float64_autograd(case):
    sd, x, g_out, g_f4, (out_a, f4_a, dx_a) = case
    out, f4, c = R.forward(sd, x)
    dx = R.backward(c, g_out, g_f4)
    assert out.shape == (1, 1) and f4.shape == g_f4.shape and dx.shape == x.shape
    assert dx_a.abs().max() > 0 and sd["attention.gamma"].item() != 0
    for name, got, ref in (("output", out, out_a), ("feature4", f4, f4_a), ("dx", dx, dx_a)):
        assert _rel(got, ref) <= 1e-12, (name, _rel(got, ref))
    # each seed alone
    for go, gf in ((g_out, None), (None, g_f4)):
        assert _rel(R.backward(c, go, gf), R.autograd_composition(sd, x, go, gf)[2]) <= 1e-12


def test_restatement_at_the_smallest_input_and_a_larger_last_map():
    for H, W in ((192, 384), (256, 576)):       # `last` sees 3 x 6 and 4 x 9
        sd, x, g_out, g_f4 = _case(ndf=2, H=H, W=W, N=2, seed=1)
        out_a, f4_a, dx_a = R.autograd_composition(sd, x, g_out, g_f4)
        out, f4, c = R.forward(sd, x)
        assert c["act"][6].shape[2:] == ((3, 6) if H == 192 else (4, 9))
        assert _rel(out, out_a) <= 1e-12 and _rel(f4, f4_a) <= 1e-12 and _rel(R.backward(c, g_out, g_f4), dx_a) <= 1e-12


@pytest.mark.parametrize("defect", ["parity", "sigma_bias", "softmax_sum", "mean"])
def test_seeded_defects_are_caught(case, defect):
    sd, x, g_out, g_f4, (out_a, f4_a, dx_a) = case
    out, f4, c = R.forward(sd, x, defect=defect)
    dx = R.backward(c, g_out, g_f4, defect=defect)
    worst = max(_rel(out, out_a), _rel(f4, f4_a), _rel(dx, dx_a))
    assert worst > 1e-6, (defect, worst)


def test_power_step_is_the_reference_formula():
    g = torch.Generator().manual_seed(3)
    W, u, v = torch.randn(5, 12, generator=g).double(), torch.randn(5, generator=g).double(), torch.randn(12, generator=g).double()
    u2, v2, s = R.sigma_step(W.view(5, 3, 2, 2), u, v)
    v_ref = W.t() @ u / ((W.t() @ u).norm() + 1e-12)
    u_ref = W @ v_ref / ((W @ v_ref).norm() + 1e-12)
    assert torch.equal(v2, v_ref) and torch.equal(u2, u_ref) and s.item() == pytest.approx((u_ref @ W @ v_ref).item(), rel=1e-14)
    assert s.item() <= torch.linalg.matrix_norm(W, 2).item() * (1 + 1e-12)


@pytest.mark.parametrize("C,P,peak", R.ATTENTION_CASES)
def test_attention_inputs_are_well_conditioned(C, P, peak):
    """The GPU tests' attention inputs: energies O(1-10) (or one well-separated maximum near `peak`), and the float32 CPU
    restatement within 1e-4 of float64 on every result."""
    q, k, v, do = R.attention_inputs(C, P, peak=peak)
    e = q.double().transpose(1, 2) @ k.double()
    top2 = e.topk(min(2, P), dim=-1).values
    if peak is None:
        assert e.abs().max().item() <= 30 and (P == 1 or e.std().item() >= 1)
    else:
        assert (top2[..., 0] - peak).abs().max().item() <= 0.05 * peak and (top2[..., 0] - top2[..., 1]).min().item() >= 50
    res = {}
    for dt in (torch.float64, torch.float32):
        qq, kk, vv, dd = (t.to(dt) for t in (q, k, v, do))
        o, a = R.attention_core(qq, kk, vv)
        res[dt] = (o, a) + tuple(R.attention_core_bwd(qq, kk, vv, a, dd))
    for name, r32, r64 in zip(("o", "a", "dq", "dk", "dv"), res[torch.float32], res[torch.float64]):
        assert torch.isfinite(r32).all()
        if r64.abs().max() < 1e-20:      # (the one-hot rows of the peaked case pass no gradient to q and k; P = 1 passes none at all)
            assert r32.abs().max() < 1e-20, name
        else:
            assert _rel(r32, r64) <= 1e-4, (name, _rel(r32, r64))


def test_state_dict_keys_shapes_and_frozen_vectors():
    from dvc_amd import arch, synth
    from dvc_amd.gan import Discriminator_x64
    net = Discriminator_x64(in_size=6, ndf=8)
    sd = net.state_dict()
    shapes = arch.discriminator_param_shapes(6, 8)
    assert {k: tuple(v.shape) for k, v in sd.items()} == shapes
    assert [k for k in sd if k.startswith("layer1.")] == ["layer1.0.module.bias", "layer1.0.module.weight_u",
                                                          "layer1.0.module.weight_v", "layer1.0.module.weight_bar"]
    for k in ("attention.gamma", "attention.query_conv.module.weight_bar", "attention.key_conv.module.weight_u",
              "attention.value_conv.module.bias", "last.module.weight_v", "layer6.0.module.weight_bar"):
        assert k in sd, k
    assert len(sd) == 41 and shapes["last.module.weight_bar"] == (1, 128, 3, 6) and shapes["layer1.0.module.weight_v"] == (96,)
    assert shapes["layer4.0.module.weight_bar"] == (32, 16, 4, 4) and shapes["attention.query_conv.module.weight_bar"] == (32, 32, 1, 1)
    assert net.attention.gamma.item() == 0.0 and net.attention.gamma.requires_grad
    for n, p in net.named_parameters():
        assert p.requires_grad == (not n.endswith(("weight_u", "weight_v"))), n
    for n, p in net.named_parameters():
        if n.endswith("weight_u"):
            assert abs(p.norm().item() - 1) < 1e-5
    net.load_state_dict(synth.discriminator_state_dict(0, ndf=8))      # strict
    assert net.attention.gamma.item() == 0.5
    d64 = Discriminator_x64()
    assert d64.in_size == 6 and d64.ndf == 64 and d64.last.module.weight_bar.shape == (1, 1024, 3, 6)


def test_module_refusals():
    from dvc_amd.gan import Discriminator_x64
    net = Discriminator_x64(ndf=2)
    x = torch.zeros(1, 6, 192, 384)
    with pytest.raises(NotImplementedError, match="parameter gradients are not built yet"):
        net(x)                                              # unfrozen parameters while autograd records
    net.requires_grad_(False)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        net(x)                                              # frozen: nothing left to refuse but the CPU tensor
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        net(x.clone().requires_grad_(True))
    net.requires_grad_(True)
    with torch.no_grad(), pytest.raises(RuntimeError, match="no CPU fallback"):
        net(x)                                              # under no_grad the unfrozen parameters are not refused
    with pytest.raises(RuntimeError, match=r"190 x 384 input leaves a 2 x 6 map"):
        net(torch.zeros(1, 6, 190, 384))
    with pytest.raises(RuntimeError, match=r"192 x 383 input leaves a 3 x 5 map"):
        net(torch.zeros(1, 6, 192, 383))
    with pytest.raises(RuntimeError, match=r"\[N, 6, H, W\]"):
        net(torch.zeros(1, 3, 192, 384))
    from dvc_amd import ops
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.gan_softmax_rows(torch.zeros(2, 3))


def test_abi_version_is_unchanged():
    from dvc_amd import _lib
    assert _lib.ABI_VERSION == 20 and _lib.load().dvc_abi_version() == 20
    assert "#define DVC_ABI_VERSION 20" in open(os.path.join(os.path.dirname(__file__), "..", "include", "dvc_hip.h")).read()


def _desc(**kw):
    from dvc_amd import ops
    base = dict(N=1, Cin=6, H=8, W=8, Cout=8, ksize=4, stride=2, pad=1, act=ops.ACT_LEAKY, act_slope=0.2)
    base.update(kw)
    N, Cin, H, W, Cout = (base.pop(k) for k in ("N", "Cin", "H", "W", "Cout"))
    return ops._conv_desc(N, Cin, H, W, Cout, **base)


def test_c_entry_points_refuse_before_any_launch():
    from dvc_amd import _lib
    lib = _lib.load()
    one, odd = ctypes.c_void_p(64), ctypes.c_void_p(68)

    def refused(rc, text):
        assert rc != 0 and text in lib.dvc_last_error().decode(), lib.dvc_last_error()

    for fn, tail in ((lib.dvc_gan_conv4s2, (one, one, one, one, one, None)), (lib.dvc_gan_conv4s2_dgrad, (one, one, one, None, one, None))):
        refused(fn(ctypes.byref(_desc(ksize=3)), *tail), "4x4 stride-2")
        refused(fn(ctypes.byref(_desc(stride=1)), *tail), "4x4 stride-2")
        refused(fn(ctypes.byref(_desc(pad=0)), *tail), "4x4 stride-2")
        refused(fn(ctypes.byref(_desc(act=1)), *tail), "NONE or LEAKY")
        refused(fn(ctypes.byref(_desc(H=1)), *tail), "bad shape")
        refused(fn(ctypes.byref(_desc(Cout=0)), *tail), "bad shape")
        refused(fn(ctypes.byref(_desc(in_up=2)), *tail), "no input transform")
        refused(fn(ctypes.byref(_desc(x_batch_stride=6 * 64 - 1)), *tail), "x_batch_stride")
        refused(fn(ctypes.byref(_desc(y_batch_stride=8 * 16 - 1)), *tail), "y_batch_stride")
        refused(fn(None, *tail), "null descriptor")
    refused(lib.dvc_gan_conv4s2(ctypes.byref(_desc()), one, one, None, one, one, None), "null argument")
    refused(lib.dvc_gan_conv4s2(ctypes.byref(_desc()), one, odd, one, one, one, None), "16-byte aligned")
    refused(lib.dvc_gan_conv4s2_dgrad(ctypes.byref(_desc()), None, one, one, None, one, None), "null argument")
    refused(lib.dvc_gan_spectral_sigma(one, 8, 96, 1e-12, one, one, one, one, (8 + 96) * 4 - 1, None), "workspace too small")
    refused(lib.dvc_gan_spectral_sigma(one, 8, 96, 1e-12, one, one, one, None, 1 << 20, None), "workspace too small")
    refused(lib.dvc_gan_spectral_sigma(one, 0, 96, 1e-12, one, one, one, one, 1 << 20, None), "bad shape")
    refused(lib.dvc_gan_spectral_sigma(one, 8, 96, 1e-12, None, one, one, one, 1 << 20, None), "null argument")
    refused(lib.dvc_gan_sn_weight(one, one, 8, 8, None, one, 7, None), "ldt")
    refused(lib.dvc_gan_sn_weight(one, one, 8, 8, None, None, 8, None), "null argument")
    refused(lib.dvc_gan_last(one, one, one, one, 1, 16, 2, 6, 0, one, None), "smaller than the 3 x 6 filter")
    refused(lib.dvc_gan_last(one, one, one, one, 1, 16, 3, 5, 0, one, None), "smaller than the 3 x 6 filter")
    refused(lib.dvc_gan_last(one, one, one, one, 1, 16, 3, 6, 16 * 18 - 1, one, None), "x_batch_stride")
    refused(lib.dvc_gan_last_bwd(one, one, one, None, 0.2, 1, 16, 3, 5, one, None), "smaller than the 3 x 6 filter")
    refused(lib.dvc_gan_last_bwd(None, one, one, None, 0.2, 1, 16, 3, 6, one, None), "null argument")
    refused(lib.dvc_gan_softmax_rows(one, 4, 0, one, None), "bad shape")
    refused(lib.dvc_gan_softmax_rows(one, 4, 7, None, None), "null argument")
    refused(lib.dvc_gan_softmax_rows_bwd(one, one, 0, 7, one, None), "bad shape")
    refused(lib.dvc_gan_scale_add(one, None, None, 8, one, None), "null argument")
    refused(lib.dvc_gan_scale_add(one, None, one, 0, one, None), "bad count")
    refused(lib.dvc_gan_lrelu_bwd(None, None, one, 0.2, 8, one, None), "null argument")
