"""GPU: every launch of a real backward against a float64 evaluation of that same launch, fed the device's own inputs
(tests/bwd_audit.py) — at the production size, with both weight sets and both algorithm choices.

The end-to-end comparisons (test_gpu_cvn_backward.py::test_gradients_vs_float64, test_gpu_vgg_backward.py) measure the
conditioning of a 31- / 16-layer chain as much as the kernels; here each step is a short linear map, so the bound is the
engine's own (input gradients: tests/test_gpu_ops.py's 2e-5 / 5e-5) or a float32 CPU evaluation of that very step (sums over
all positions), whatever the weights.  The wiring between the steps does not depend on the size and is pinned by the 48x80
end-to-end test at 1e-5.  One line per launch goes to the suite's test report (test_gpu_ops.report).

Measured on an MI355X with 16 CPU threads for the references: a ColorVidNet case (87 launches) takes 5 s at 1 x 216 x 384 and
13 s at 2 x 216 x 384, 1 s or less at the small sizes; the five VGG19 cases take under 2 s together.
"""
import contextlib
import io
import time

import pytest
import torch

import bwd_audit as BA
import vgg_bwd_reference as VR
from test_gpu_ops import report          # the report file every GPU test of the suite appends to

pytestmark = pytest.mark.gpu

def _assert_records(records, case, expected_kinds):
    for r in records:
        report(BA.line(r, case))
    for kind, r in BA.worst_by_kind(records).items():
        report("bwd_audit worst " + BA.line(r, case)[len("bwd_audit "):])
        print("worst", BA.line(r, case))
    assert [r["kind"] for r in records] == expected_kinds          # coverage: one record per launch the backward must make
    bad = [v for r in records for v in BA.violations(r)]
    assert not bad, "\n".join([case] + bad)


@pytest.mark.parametrize("contractive", [True, False], ids=["contractive", "plain"])
@pytest.mark.parametrize("algo", ["auto", "direct"])
@pytest.mark.parametrize("B,H,W", [(1, 216, 384), (2, 216, 384), (2, 48, 80), (1, 40, 64)])
def test_colorvidnet_backward_every_launch(B, H, W, algo, contractive):
    """Training mode, every parameter and x requiring grad.  The step-wise check does not care about the chaos of the plain
    seed-0 weights (an fp32 rounding of the forward moves their float64 end-to-end gradient by percent): they are what a user
    trains from, and every launch on them is held to the same bounds."""
    from dvc_amd import arch, ops, synth
    from models.ColorVidNet import ColorVidNet
    with contextlib.redirect_stdout(io.StringIO()):
        m = ColorVidNet(7)
    m.load_state_dict(synth.colorvidnet_state_dict(0, contractive=contractive))
    m = m.cuda().train()
    g = torch.Generator().manual_seed(2)
    x = ((torch.rand(B, 7, H, W, generator=g) * 2 - 1) * 50).cuda().requires_grad_(True)
    g_ab = torch.randn(B, 2, H, W, generator=torch.Generator().manual_seed(3)).cuda()
    case = f"cvn B{B} {H}x{W} {algo} {'contractive' if contractive else 'plain'}"
    prev = ops.conv_algo()
    t0 = time.time()
    try:
        ops.set_conv_algo(algo)
        y = m(x)
        with BA.Recorder(ops) as rec:
            y.backward(g_ab)
    finally:
        ops.set_conv_algo(prev)
    assert x.grad is not None and all(p.grad is not None for p in m.parameters())
    wg = [r for r in rec.records if r["kind"] == "wgrad"]
    assert len(wg) == len(arch.CVN_CONVS)
    for r, c in zip(wg, reversed(arch.CVN_CONVS)):          # (the launch does not carry the layer's name)
        r["layer"] = "wgrad." + c["key"]
    report(f"bwd_audit {case}: {len(rec.records)} launches, {time.time() - t0:.0f} s with the references")
    _assert_records(rec.records, case, BA.expected_cvn_kinds(arch.CVN_CONVS, need_dx=True))
    dgrads = [r for r in rec.records if r["kind"] == "dgrad"]
    assert [r["layer"] for r in dgrads] == ["cvn_bwd." + c["key"] for c in reversed(arch.CVN_CONVS)]
    assert dgrads[-1]["pad_zero"] is True              # cvn_bwd.conv1_1.0: all 32 padded channels computed, 25 exactly zero
    engines = {r["engine"] for r in dgrads}
    if algo == "direct":
        assert "winograd" not in engines, engines
    elif (H, W) == (216, 384):
        assert "winograd" in engines and len(engines) >= 2, engines     # the production engine choices are what was audited


AUDITED_VGG_CASES = ("216x384", "odd45x70", "no_preprocess", "avg_pool", "p3_r44")


@pytest.mark.parametrize("name", AUDITED_VGG_CASES)
def test_vgg_input_grad_every_launch(name):
    """VGG19 frozen, input requiring grad; the activation and pool steps bit for bit against ATen float32, from the device's own
    saved R."""
    from dvc_amd import arch, ops
    from test_gpu_vgg_backward import CASES, _image, _vgg
    _, B, H, W, keys, pre, pool, none_keys = next(c for c in CASES if c[0] == name)
    assert not none_keys
    m = _vgg(pool)
    x = _image(11, B, H, W).cuda().requires_grad_(True)
    outs = m(x, keys, preprocess=pre)
    G = VR.loss_grads([o.detach().cpu() for o in outs], seed=7)
    loss = sum((o * g.float().cuda()).sum() for o, g in zip(outs, G))
    with BA.Recorder(ops) as rec:
        loss.backward()
    assert x.grad is not None and torch.isfinite(x.grad).all()
    _assert_records(rec.records, f"vgg {name}", BA.expected_vgg_kinds(arch.VGG_KEYS, keys))
    assert rec.records[-1]["kind"] == "conv1_bwd" and rec.records[-1]["out"] == (B, 3, H, W)
