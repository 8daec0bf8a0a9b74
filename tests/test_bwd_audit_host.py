"""CPU: the backward audit audited (tests/bwd_audit.py) — its float64 step references against float64 autograd through the
pieces of oracle/dvc_oracle.py, the recorder around ColorVidNet._backward / VGG19_pytorch._input_grad driven on CPU tensors with
float32 stand-ins for the launches, and seeded defects, each of which must break the bound the GPU test applies."""
import contextlib
import io

import pytest
import torch
import torch.nn.functional as F

import bwd_audit as BA
from oracle import dvc_oracle as O

D = torch.float64


def _r(seed, *shape):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=D)


def _close(a, b, tol=1e-12):
    e = BA.relerr(a, b)
    assert e <= tol, e


# ================================================================================================ references vs oracle autograd
@pytest.mark.parametrize("dil", [1, 2])
@pytest.mark.parametrize("in_up", [1, 2])
def test_conv_step_references_vs_oracle_autograd(dil, in_up):
    """d/dx, d/dW, d/db of the oracle's convolution (colorvidnet_forward's `conv`, behind O._up2 for the decoder layers)."""
    from dvc_amd.nets import cvn_bwd_weight
    Cin, Cout, H, W = 5, 6, 10, 14
    x = _r(1, 2, Cin, H // in_up, W // in_up).requires_grad_(True)
    w, b = _r(2, Cout, Cin, 3, 3).requires_grad_(True), _r(3, Cout).requires_grad_(True)
    dZ = _r(4, 2, Cout, H, W)
    y = F.conv2d(O._up2(x) if in_up == 2 else x, w, b, padding=dil, dilation=dil)
    gx, gw, gb = torch.autograd.grad(y, (x, w, b), dZ)
    full = BA.ref_dgrad(dZ, cvn_bwd_weight(w.detach()), dil)
    _close(F.avg_pool2d(full, 2) * 4 if in_up == 2 else full, gx)
    dW, db = BA.ref_wgrad(dZ, x.detach(), dil, in_up)
    _close(dW, gw)
    _close(db, gb)
    padded = BA.ref_dgrad(dZ, cvn_bwd_weight(w.detach(), pad_to=8), dil)
    assert torch.equal(padded[:, :Cin], full) and not padded[:, Cin:].any()


@pytest.mark.parametrize("kinds", [("full",), ("ss",), ("up",), ("full", "ss"), ("ss", "up"), ("full", "ss", "up")])
@pytest.mark.parametrize("H,W", [(12, 16), (9, 7)])
def test_inorm_reference_vs_oracle_autograd(kinds, H, W):
    """ReLU -> O._inorm -> one, two or three consumers (plain, `_ss` scale at stride 2, nearest x2)."""
    B, C = 2, 3
    pre = _r(5, B, C, H, W).requires_grad_(True)
    ssw = _r(6, C).requires_grad_(True)
    R = F.relu(pre)
    n = O._inorm(R)
    gf, gs, gu = _r(7, B, C, H, W), _r(8, B, C, (H + 1) // 2, (W + 1) // 2), _r(9, B, C, 2 * H, 2 * W)
    loss = 0
    if "full" in kinds:
        loss = loss + (n * gf).sum()
    if "ss" in kinds:
        loss = loss + (F.conv2d(n, ssw.view(C, 1, 1, 1), None, stride=2, groups=C) * gs).sum()
    if "up" in kinds:
        loss = loss + (O._up2(n) * gu).sum()
    loss.backward()
    rstd = 1 / torch.sqrt(R.detach().var((2, 3), unbiased=False) + 1e-5)
    dZ, dss = BA.ref_inorm_bwd(n.detach(), rstd.reshape(-1), R.detach(), gf if "full" in kinds else None,
                               gs if "ss" in kinds else None, ssw.detach() if "ss" in kinds else None, gu if "up" in kinds else None)
    _close(dZ, pre.grad, 1e-11)         # (the norm's own cancellation: 1e-11 of the gradient's scale in float64)
    if "ss" in kinds:
        _close(dss, ssw.grad)
    else:
        assert dss is None


def test_head_reference_vs_oracle_autograd():
    B, C, H, W = 2, 12, 7, 9
    pre = _r(10, B, C, H, W).requires_grad_(True)
    w, b = (_r(11, 2, C, 1, 1) * 0.1).requires_grad_(True), _r(12, 2).requires_grad_(True)
    c10 = F.leaky_relu(pre, 0.2)
    ab = torch.tanh(F.conv2d(c10, w, b)) * 128
    g = _r(13, B, 2, H, W)
    gp, gw, gb = torch.autograd.grad(ab, (pre, w, b), g)
    dZ, dW, db = BA.ref_head_bwd(ab.detach(), g, w.detach().view(2, C), c10.detach(), 0.2)
    _close(dZ, gp)
    _close(dW, gw.view(2, C))
    _close(db, gb)


def test_act_and_pool_references_are_aten_autograd():
    """Ties, zeros and odd edges: the references are ATen's own relu / max_pool2d / avg_pool2d backward in float32."""
    g = torch.Generator().manual_seed(14)
    R = F.relu(torch.randint(-2, 4, (2, 3, 7, 9), generator=g).float() * 0.5)
    dX, gR = torch.randn(R.shape, generator=g), torch.randn(R.shape, generator=g)
    assert torch.equal(BA.ref_act_bwd(dX, gR, R), torch.ops.aten.threshold_backward(dX + gR, R, 0))
    assert torch.equal(BA.ref_act_bwd(None, gR, R), torch.ops.aten.threshold_backward(gR, R, 0))
    dP = torch.randn(2, 3, 3, 4, generator=g)
    _, idx = F.max_pool2d(R, 2, 2, return_indices=True)
    routed = torch.ops.aten.max_pool2d_with_indices_backward(dP, R, [2, 2], [2, 2], [0, 0], [1, 1], False, idx)
    assert torch.equal(BA.ref_pool_act_bwd(dP, None, gR, R), torch.ops.aten.threshold_backward(routed + gR, R, 0))


# ================================================================================================ the recorder
def _standins(monkeypatch, ops, calls):
    """float32 CPU stand-ins for the launches, built from the audit's own references; `calls` receives (name, layer)."""
    def conv3x3(x, weight, packs, bias, *, dil=1, layer=None, **kw):
        calls.append(("conv3x3", layer))
        if ops.conv_record is not None:
            ops.conv_record.append(dict(algo="winograd") if dil == 2 else dict(Cin=x.shape[1]))     # (conv2d logs no `algo`)
        return F.conv2d(x, weight, bias, padding=dil, dilation=dil)

    def cvn_wgrad(dZ, X, *, dil=1, in_up=1, splits=None):
        calls.append(("cvn_wgrad", None))
        return BA.ref_wgrad(dZ, X, dil, in_up, dtype=torch.float32)

    def cvn_head_bwd(ab, grad_ab, w_ab, R, slope=0.2):
        calls.append(("cvn_head_bwd", None))
        dZ, dW, db = BA.ref_head_bwd(ab, grad_ab, w_ab, R, slope, dtype=torch.float32)
        return dZ, dW.view(2, -1, 1, 1), db

    def cvn_inorm_bwd(n, rstd, R, g_full=None, g_ss=None, ss_w=None, g_up=None):
        calls.append(("cvn_inorm_bwd", None))
        return BA.ref_inorm_bwd(n, rstd, R, g_full, g_ss, ss_w, g_up, dtype=torch.float32)

    def vgg_act_bwd(dX, g, R, out=None):
        calls.append(("vgg_act_bwd", None))
        y = BA.ref_act_bwd(dX, g, R)
        if out is not None:             # in place, as the launch is
            out.copy_(y)
            return out
        return y

    def vgg_pool_act_bwd(dP, gP, gR, R, avg=False):
        calls.append(("vgg_pool_act_bwd", None))
        return BA.ref_pool_act_bwd(dP, gP, gR, R, avg)

    def vgg_conv1_bwd(dZ, w_t):
        calls.append(("vgg_conv1_bwd", None))
        return F.conv2d(dZ, w_t, padding=1)

    fns = dict(conv3x3=conv3x3, cvn_wgrad=cvn_wgrad, cvn_head_bwd=cvn_head_bwd, cvn_inorm_bwd=cvn_inorm_bwd,
               vgg_act_bwd=vgg_act_bwd, vgg_pool_act_bwd=vgg_pool_act_bwd, vgg_conv1_bwd=vgg_conv1_bwd)
    assert set(fns) == set(BA.PATCHED)
    for k, f in fns.items():
        monkeypatch.setattr(ops, k, f)
    return fns


def _cvn_saved(m, x):
    """What ColorVidNet._forward(saved=..., rstd=...) saves, by a float32 CPU walk over arch.CVN_CONVS."""
    from dvc_amd import arch
    acts, t = {"x": x}, {"x": x}
    for c in arch.CVN_CONVS:
        src, pre, inp = c["src"], c["pre"], acts[c["src"]]
        if pre is not None:
            n = F.instance_norm(inp, eps=1e-5)
            t["n:" + src] = n
            t["rstd:" + src] = (1 / torch.sqrt(inp.var((2, 3), unbiased=False) + 1e-5)).reshape(-1)
            inp = n
            if pre == "norm_ss":
                inp = t["nss:" + src] = (n[:, :, ::2, ::2] * m._mod(c["ss"]).weight.detach().view(1, -1, 1, 1)).contiguous()
            elif pre == "up":
                inp = BA.up2(n)
        conv = m._mod(c["key"])
        y = F.conv2d(inp, conv.weight.detach(), conv.bias.detach(), padding=c["dil"], dilation=c["dil"])
        if c["add"] is not None:
            y = y + acts[c["add"]]
        y = F.relu(y) if c["act"] == "relu" else F.leaky_relu(y, 0.2) if c["act"] == "leaky" else y
        acts[c["dst"]] = t[c["dst"]] = y
    out = m._mod(arch.CVN_OUT["key"])
    t["ab"] = torch.tanh(F.conv2d(acts["c10_2"], out.weight.detach(), out.bias.detach())) * 128
    return t


def _cvn_cpu():
    from dvc_amd import nets, synth
    with contextlib.redirect_stdout(io.StringIO()):
        m = nets.ColorVidNet(7)
    m.load_state_dict(synth.colorvidnet_state_dict(0, contractive=True))
    return m


@pytest.mark.parametrize("need_dx", [True, False])
def test_recorder_around_colorvidnet_backward(monkeypatch, need_dx):
    """ColorVidNet._backward itself on CPU tensors (it only reaches the device through `ops`): one record per launch, in the
    order _backward makes them, every clean float32 step inside its bound, attributes restored."""
    from dvc_amd import arch, ops
    calls = []
    fns = _standins(monkeypatch, ops, calls)
    m = _cvn_cpu()
    x = (torch.rand(1, 7, 16, 24, generator=torch.Generator().manual_seed(1)) * 2 - 1) * 50
    t = _cvn_saved(m, x)
    g_ab = torch.randn(t["ab"].shape, generator=torch.Generator().manual_seed(2))
    need = {n for n, _ in m.named_parameters()}
    assert ops.conv_record is None
    with BA.Recorder(ops) as rec:
        assert all(getattr(ops, k) is not fns[k] for k in BA.PATCHED)
        dx, grads = m._backward(t, g_ab, need, need_dx)
        # a forward launch passes straight through: the stand-in sees it, the recorder does not
        n_rec, n_calls = len(rec.records), len(calls)
        ops.conv3x3(x, m._mod("conv1_1.0").weight.detach(), None, None, layer="cvn.conv1_1.0")
        ops.conv3x3(x, m._mod("conv1_1.0").weight.detach(), None, None)
        assert len(rec.records) == n_rec and len(calls) == n_calls + 2
    assert all(getattr(ops, k) is fns[k] for k in BA.PATCHED) and ops.conv_record is None
    kinds = [r["kind"] for r in rec.records]
    assert kinds == BA.expected_cvn_kinds(arch.CVN_CONVS, need_dx)
    assert len(kinds) == n_calls            # exactly one record per launch
    n = len(arch.CVN_CONVS)
    assert kinds.count("wgrad") == n and kinds.count("dgrad") == n - (0 if need_dx else 1) and kinds.count("head") == 1
    assert kinds.count("inorm") + kinds.count("act") == len({c["dst"] for c in arch.CVN_CONVS if c["act"] != "none"}) - 1
    dgrads = [r for r in rec.records if r["kind"] == "dgrad"]
    assert [r["layer"] for r in dgrads] == ["cvn_bwd." + c["key"] for c in reversed(arch.CVN_CONVS)][:len(dgrads)]
    assert {r["engine"] for r in dgrads} == {"direct", "winograd"}      # read from ops.conv_record
    assert (dx is not None) == need_dx and set(grads) == need
    if need_dx:
        assert dgrads[-1]["pad_zero"] is True and dgrads[-1]["out"][1] == 32 and dx.shape[1] == 7
    for r in rec.records:
        assert BA.violations(r) == [], BA.line(r)
        assert BA.line(r, "host").startswith("bwd_audit host " + r["kind"])


def test_recorder_around_vgg_input_grad(monkeypatch):
    from dvc_amd import arch, nets, ops, synth
    calls = []
    fns = _standins(monkeypatch, ops, calls)
    with contextlib.redirect_stdout(io.StringIO()):
        m = nets.VGG19_pytorch()
    sd = synth.vgg19_state_dict(0)
    m.load_state_dict(sd)
    x = torch.rand(1, 3, 32, 48, generator=torch.Generator().manual_seed(3))
    keys = ["r12", "p1", "r32", "r42", "r52"]
    rk = [k for k in arch.VGG_KEYS[:arch.VGG_KEYS.index("r52") + 1] if k[0] == "r"]
    with torch.no_grad():
        saved = dict(zip(rk, O.vgg19_forward(sd, x, rk)))
        outs = O.vgg19_forward(sd, x, keys)
    g_ext = {k: torch.randn(o.shape, generator=torch.Generator().manual_seed(4)) for k, o in zip(keys, outs)}
    with BA.Recorder(ops) as rec:
        dx = m._input_grad(saved, g_ext, True)
    assert all(getattr(ops, k) is fns[k] for k in BA.PATCHED)
    kinds = [r["kind"] for r in rec.records]
    assert kinds == BA.expected_vgg_kinds(arch.VGG_KEYS, keys) and len(kinds) == len(calls)
    assert kinds.count("pool_act") == 4 and kinds.count("dgrad") == 13 and kinds[-1] == "conv1_bwd"
    assert dx.shape == x.shape
    for r in rec.records:
        assert BA.violations(r) == [], BA.line(r)


def test_recorder_restores_on_exception_and_is_inert_outside(monkeypatch):
    from dvc_amd import ops
    calls = []
    fns = _standins(monkeypatch, ops, calls)
    keep = ops.conv_record = []
    try:
        with pytest.raises(ZeroDivisionError):
            with BA.Recorder(ops) as rec:
                assert ops.conv_record is keep
                ops.vgg_act_bwd(None, torch.ones(1, 1, 2, 2), torch.ones(1, 1, 2, 2))
                1 / 0
        assert len(rec.records) == 1
        assert all(getattr(ops, k) is fns[k] for k in BA.PATCHED) and ops.conv_record is keep
        ops.vgg_act_bwd(None, torch.ones(1, 1, 2, 2), torch.ones(1, 1, 2, 2))       # recorder off: untouched
        assert len(rec.records) == 1 and len(calls) == 2
    finally:
        ops.conv_record = None


def test_recorder_sees_the_input_of_an_in_place_activation_step(monkeypatch):
    """vgg_act_bwd(dX, ..., out=dX) overwrites dX: the audit must compare against the reference of the ORIGINAL dX."""
    from dvc_amd import ops
    _standins(monkeypatch, ops, [])
    g = torch.Generator().manual_seed(5)
    R = F.relu(torch.randn(1, 2, 5, 6, generator=g))
    dX, gR = torch.randn(R.shape, generator=g), torch.randn(R.shape, generator=g)
    want = BA.ref_act_bwd(dX, gR, R)
    with BA.Recorder(ops) as rec:
        y = ops.vgg_act_bwd(dX, gR, R, out=dX)
    assert y is dX and torch.equal(dX, want)
    assert BA.violations(rec.records[0]) == []


# ================================================================================================ seeded defects
def _wgrad_case(W=21, dil=1, in_up=1):
    B, Cin, Cout, H = 2, 12, 10, 12
    W += W % in_up
    dZ, X = _r(20, B, Cout, H, W).float(), _r(21, B, Cin, H // in_up, W // in_up).float()
    dW, db = BA.ref_wgrad(dZ, X, dil, in_up)
    return dZ, X, dW.float(), db.float()


def _names(rec):
    return " | ".join(BA.violations(rec))


@pytest.mark.parametrize("tap", range(9))
def test_defect_one_tap_scaled(tap):
    """(a) one of the nine taps of dW off by 1e-3 relative: invisible-ish to a whole-tensor norm (3e-4), plain in its tap."""
    dZ, X, dW, db = _wgrad_case()
    assert BA.violations(BA.audit_wgrad(dW, db, dZ, X)) == []
    bad = dW.clone()
    bad[:, :, tap // 3, tap % 3] *= 1 + 1e-3
    rec = BA.audit_wgrad(bad, db, dZ, X)
    assert "dW.tap%d" % tap in _names(rec)
    others = [k for k in rec["measures"] if k.startswith("dW.tap") and k != "dW.tap%d" % tap]
    assert all(rec["measures"][k] <= rec["bounds"][k] for k in others)
    assert rec["measures"]["dW.tap%d" % tap] > 100 * rec["bounds"]["dW.tap%d" % tap]


@pytest.mark.parametrize("dil,in_up", [(1, 1), (2, 1), (1, 2)])
def test_defect_last_partial_chunk_dropped(dil, in_up):
    """(b) W = 21 or 22: the positions past the last whole 16-chunk of each row missing from the sum."""
    dZ, X, dW, db = _wgrad_case(21, dil, in_up)
    assert BA.violations(BA.audit_wgrad(dW, db, dZ, X, dil, in_up)) == []
    cut = dZ.clone()
    cut[..., 16:] = 0
    bad_dW, bad_db = BA.ref_wgrad(cut, X, dil, in_up)
    rec = BA.audit_wgrad(bad_dW.float(), bad_db.float(), dZ, X, dil, in_up)
    v = _names(rec)
    assert "dW.whole" in v and "dW.chan" in v and "db.whole" in v and all("dW.tap%d" % t in v for t in range(9))


@pytest.mark.parametrize("engine", ["direct", "direct-ws", "winograd"])
@pytest.mark.parametrize("dil", [1, 2])
def test_defect_border_row_padding_one_short(engine, dil):
    """(c) the last output row computed as if the map ended one row earlier (its own input row taken for padding)."""
    B, Ci, Co, H, W = 1, 16, 8, 40, 56
    dZ, wt = _r(22, B, Ci, H, W).float(), (_r(23, Co, Ci, 3, 3) / 12).float()
    good = BA.ref_dgrad(dZ, wt, dil).float()
    assert BA.violations(BA.audit_dgrad(good, dZ, wt, dil, engine, "cvn_bwd.t")) == []
    short = dZ.clone()
    short[:, :, -1] = 0
    bad = good.clone()
    bad[:, :, -1] = BA.ref_dgrad(short, wt, dil).float()[:, :, -1]
    rec = BA.audit_dgrad(bad, dZ, wt, dil, engine, "cvn_bwd.t")
    v = _names(rec)
    assert "ring" in v and "whole" in v and "interior" not in v
    assert rec["measures"]["ring"] > 1000 * max(rec["bounds"].values())
    with pytest.raises(KeyError):
        BA.audit_dgrad(good, dZ, wt, dil, "some-new-engine", "cvn_bwd.t")


def test_dgrad_bound_refinement_uses_the_float32_yardstick():
    """A non-Winograd record over 2e-5 gets max(2e-5, 4 x float32 CPU ATen's error) and no more; Winograd gets no allowance."""
    B, Ci, Co, H, W = 1, 16, 8, 20, 24
    dZ, wt = _r(24, B, Ci, H, W).float(), (_r(25, Co, Ci, 3, 3) / 12).float()
    ref = BA.ref_dgrad(dZ, wt, 1)
    off = (ref + 3e-5 * ref.abs().max()).float()
    rec = BA.audit_dgrad(off, dZ, wt, 1, "direct", "cvn_bwd.t")
    assert rec["yard"] is not None and rec["yard"]["whole"] < 1e-6
    assert rec["bounds"]["whole"] == BA.DGRAD_BOUND["direct"] == 2e-5 and BA.violations(rec)
    rec = BA.audit_dgrad((ref + 3e-5 * ref.abs().max()).float(), dZ, wt, 1, "winograd", "cvn_bwd.t")
    assert rec["yard"] is None and BA.violations(rec) == [] and rec["bounds"]["whole"] == 5e-5
    assert BA.violations(BA.audit_dgrad((ref + 6e-5 * ref.abs().max()).float(), dZ, wt, 1, "winograd", "cvn_bwd.t"))


def test_defect_padded_channels_not_zero():
    from dvc_amd.nets import cvn_bwd_weight
    dZ, w = _r(26, 1, 32, 9, 11).float(), (_r(27, 32, 7, 3, 3) / 8).float()
    wt = cvn_bwd_weight(w, pad_to=32)
    good = BA.ref_dgrad(dZ, wt).float()
    rec = BA.audit_dgrad(good, dZ, wt, 1, "direct", "cvn_bwd.conv1_1.0", keep=7)
    assert rec["pad_zero"] is True and BA.violations(rec) == []
    bad = good.clone()
    bad[0, 31, 4, 5] = 1e-30
    assert "zero-padded" in _names(BA.audit_dgrad(bad, dZ, wt, 1, "direct", "cvn_bwd.conv1_1.0", keep=7))


@pytest.mark.parametrize("kinds", [("up",), ("full", "ss", "up")])
def test_defect_g_up_sum_missing_a_term_on_the_last_row(kinds):
    """(d) the 2x2 sum of g_up without its bottom-right term on the map's last row."""
    B, C, H, W = 2, 4, 24, 32
    R = F.relu(_r(28, B, C, H, W) + 0.3).float()
    n = F.instance_norm(R, eps=1e-5)
    rstd = (1 / torch.sqrt(R.var((2, 3), unbiased=False) + 1e-5)).reshape(-1)
    gf = _r(29, B, C, H, W).float() if "full" in kinds else None
    gs = _r(30, B, C, H // 2, W // 2).float() if "ss" in kinds else None
    ssw = _r(31, C).float() if "ss" in kinds else None
    gu = _r(32, B, C, 2 * H, 2 * W).float()
    dZ, dss = BA.ref_inorm_bwd(n, rstd, R, gf, gs, ssw, gu)
    clean = BA.audit_inorm(dZ.float(), None if dss is None else dss.float(), n, rstd, R, gf, gs, ssw, gu)
    assert BA.violations(clean) == [], _names(clean)
    cut = gu.clone()
    cut[:, :, -1, 1::2] = 0
    bad, _ = BA.ref_inorm_bwd(n, rstd, R, gf, gs, ssw, cut)
    rec = BA.audit_inorm(bad.float(), None if dss is None else dss.float(), n, rstd, R, gf, gs, ssw, gu)
    assert "dZ.whole" in _names(rec) and rec["measures"]["dZ.whole"] > 1000 * rec["bounds"]["dZ.whole"]
    if dss is not None:
        assert "dss.whole" in _names(BA.audit_inorm(dZ.float(), dss.float() * (1 + 1e-4), n, rstd, R, gf, gs, ssw, gu))
        assert "dss.whole" in _names(BA.audit_inorm(dZ.float(), None, n, rstd, R, gf, gs, ssw, gu))


def test_defect_pool_route_to_the_second_tied_maximum():
    """(e) one window with two equal maxima: ATen routes to the first in scan order; a route to the second is not bit-identical."""
    g = torch.Generator().manual_seed(33)
    R = torch.rand(1, 2, 6, 8, generator=g) * 0.5
    R[0, 1, 2, 4] = R[0, 1, 3, 5] = 2.0           # window (1, 2) of plane 1: top-left and bottom-right tie
    dP, gR = torch.randn(1, 2, 3, 4, generator=g), torch.randn(1, 2, 6, 8, generator=g)
    good = BA.ref_pool_act_bwd(dP, None, gR, R)
    assert good[0, 1, 2, 4] == dP[0, 1, 1, 2] + gR[0, 1, 2, 4] and good[0, 1, 3, 5] == gR[0, 1, 3, 5]
    assert BA.violations(BA.audit_pool_act(good, dP, None, gR, R)) == []
    bad = good.clone()
    bad[0, 1, 2, 4], bad[0, 1, 3, 5] = gR[0, 1, 2, 4], dP[0, 1, 1, 2] + gR[0, 1, 3, 5]
    rec = BA.audit_pool_act(bad, dP, None, gR, R)
    assert "not bit-identical" in _names(rec) and rec["differing"] == 2
    one_ulp = good.clone()
    one_ulp[0, 0, 0, 0] = torch.nextafter(good[0, 0, 0, 0], torch.tensor(9.0))
    assert BA.violations(BA.audit_act(one_ulp, None, good, torch.ones_like(good)))      # an activation step one ulp off


def test_defects_in_the_head_and_conv1_steps_and_a_dead_reference():
    B, C, H, W = 2, 16, 10, 12
    R = F.leaky_relu(_r(34, B, C, H, W), 0.2).float()
    w = (_r(35, 2, C) * 0.1).float()
    ab = (torch.tanh(torch.einsum("oc,bchw->bohw", w, R)) * 128).contiguous()
    g = _r(36, B, 2, H, W).float()
    ref = tuple(t.float() for t in BA.ref_head_bwd(ab, g, w, R))
    assert BA.violations(BA.audit_head(ref, ab, g, w, R)) == []
    wrong_slope = tuple(t.float() for t in BA.ref_head_bwd(ab, g, w, R, slope=0.2 * (1 + 1e-3)))
    assert "dZ.whole" in _names(BA.audit_head(wrong_slope, ab, g, w, R))
    assert "dW.whole" in _names(BA.audit_head((ref[0], ref[1] * (1 + 1e-4), ref[2]), ab, g, w, R))
    dZ, wt = _r(37, 1, 8, 17, 15).float(), (_r(38, 3, 8, 3, 3) / 8).float()
    good = BA.ref_conv1_bwd(dZ, wt).float()
    assert BA.violations(BA.audit_conv1_bwd(good, dZ, wt)) == []
    assert "whole" in _names(BA.audit_conv1_bwd(BA.ref_conv1_bwd(dZ, wt.flip(0)).float(), dZ, wt))
    dead = BA.audit_conv1_bwd(torch.zeros_like(good), torch.zeros_like(dZ), wt)
    assert "identically 0" in _names(dead)


@pytest.mark.parametrize("window,takes", [
    ((1.0, float("nan"), 3.0, 2.0), 1),                    # one NaN: it takes the window, whatever follows
    ((float("nan"), 1.0, float("nan"), 2.0), 2),           # two: the last NaN in scan order
    ((1.0, float("nan"), 2.0, float("nan")), 3),
    ((float("nan"), float("inf"), 0.5, 1.0), 0),           # +inf behind a NaN does not take it back (inf > nan is false)
    ((float("inf"), float("nan"), 0.5, 1.0), 1),
])
def test_aten_max_pool_nan_rule_is_the_one_the_kernel_states(window, takes):
    """csrc/vgg_bwd.hip's argmax4 comment: ATen scans with `v > max || isnan(v)`, so the LAST NaN of a window takes its
    gradient.  This machine's ATen agrees (contiguous and channels-last alike); the GPU test holds the kernel to it."""
    for C in (1, 16):
        R = torch.tensor(window).view(1, 1, 2, 2).repeat(1, C, 2, 3)
        for fmt in (torch.contiguous_format, torch.channels_last):
            z = R.clone().requires_grad_(True)
            F.max_pool2d(z.contiguous(memory_format=fmt), 2, 2).sum().backward()
            want = torch.zeros(4)
            want[takes] = 1
            assert torch.equal(z.grad[0, C - 1, 2:4, 4:6].reshape(-1), want), (window, C, fmt)
    dP = torch.full((1, 1, 1, 1), 3.0)
    got = BA.ref_pool_act_bwd(dP, None, None, torch.tensor(window).view(1, 1, 2, 2))
    assert got.reshape(-1)[takes] == 3.0 and got.abs().sum() == 3.0       # (a NaN R is not <= 0: the ReLU mask passes it)
