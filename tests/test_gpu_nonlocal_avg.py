"""GPU: NonlocalWeightedAverage (dvc_nlwa_fwd, csrc/nonlocal_avg.hip) against the float64 restatement
(tests/nlwa_reference.py): accuracy, the prep launch's resize selection, determinism / batch independence, a sharp
alpha, and the drop-in module with its guards."""
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import nlwa_reference as R  # noqa: E402

pytestmark = pytest.mark.gpu

# x_lab shape, feature shape, patch_size, alpha, scale_factor
CASES = {
    "bench_b2": ((2, 3, 216, 384), (2, 128, 108, 192), 3, 0.5, 0.25),        # the benchmark shape (N = 5184, K = 1152)
    "odd_c64": ((1, 3, 37, 53), (1, 64, 37, 53), 3, 0.1, 1),                 # N = 1961, W = 53
    "c3_k5": ((2, 3, 46, 58), (2, 3, 23, 29), 5, 0.01, 0.5),                 # N = 667, C = 3 (29 zero planes)
    "c256_k1": ((1, 3, 29, 31), (1, 256, 29, 31), 1, 1.0, 1),                # N = 899
    "nonint_resize": ((1, 3, 160, 256), (1, 128, 27, 45), 3, 10.0, 0.25),   # feature 27 x 45 -> 40 x 64
    "c64_k5_q": ((1, 3, 66, 102), (1, 64, 33, 51), 5, 0.5, 0.25),           # 16 x 25, N = 400 < one query block x 4
}


def _inputs(case, seed=0, device="cuda"):
    xs, fs, k, alpha, sf = case
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(xs, generator=g) * 220 - 110                # ab drawn from U(-110, 110) (L too)
    K = fs[1] * k * k
    # affinities of a moderate spread at every alpha: |u|^2 / alpha ~ 6 on the diagonal, cross terms ~ 6 / sqrt(K)
    f = torch.randn(fs, generator=g) * (6.0 * alpha / K) ** 0.5
    return x.to(device), f.to(device)


def _run(x, f, k, alpha, sf, **kw):
    from dvc_amd.nonlocal_avg import nonlocal_weighted_average
    with torch.no_grad():
        out = nonlocal_weighted_average(x, f, k, alpha, sf, **kw)
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("name", list(CASES))
def test_matches_float64_restatement(name):
    xs, fs, k, alpha, sf = CASES[name]
    x, f = _inputs(CASES[name])
    got = _run(x, f, k, alpha, sf).cpu().double()
    ref64 = R.nonlocal_weighted_average(x.cpu(), f.cpu(), k, alpha, sf, dtype=torch.float64)
    ref32 = R.nonlocal_weighted_average(x.cpu(), f.cpu(), k, alpha, sf, dtype=torch.float32).double()
    assert got.shape == ref64.shape
    err, err32 = (got - ref64).abs().max().item(), (ref32 - ref64).abs().max().item()
    tol = 4 * err32 + 1e-6 * ref64.abs().max().item()
    print(f"{name}: max-abs err {err:.3e}, fp32 CPU restatement {err32:.3e}, bound {tol:.3e}")
    assert torch.isfinite(got).all()
    assert err <= tol, (name, err, err32)


@pytest.mark.parametrize("name", list(CASES))
def test_prep_resize_is_bit_identical(name):
    """The prep launch's planes, read back out of the workspace: F_pad's interior == F.interpolate(feature, size) and its
    border / padding planes zero; the ab planes == F.interpolate(x_lab, scale_factor)[:, 1:3]."""
    from dvc_amd import _lib
    from dvc_amd.nonlocal_avg import workspace_layout
    xs, fs, k, alpha, sf = CASES[name]
    x, f = _inputs(CASES[name])
    xr = F.interpolate(x, scale_factor=sf)
    B, _, H, W = xr.shape
    fr = F.interpolate(f, size=(H, W))
    C = fs[1]
    ws = torch.empty(_lib.load().dvc_nlwa_workspace_bytes(B, C, k, H, W), device="cuda", dtype=torch.uint8)
    _run(x, f, k, alpha, sf, workspace=ws)
    lay = workspace_layout(B, C, k, H, W)
    (o_f, s_f), (o_a, s_a) = lay["fpad"], lay["ab"]
    n_f = s_f[0] * s_f[1] * s_f[2] * s_f[3]
    fpad = ws[o_f:o_f + 4 * n_f].view(torch.float32).view(s_f)
    ab = ws[o_a:o_a + 4 * B * 2 * H * W].view(torch.float32).view(s_a)
    p = k // 2
    assert torch.equal(fpad[:, :C, p:p + H, p:p + W], fr)
    inner = torch.zeros_like(fpad, dtype=torch.bool)
    inner[:, :C, p:p + H, p:p + W] = True
    assert (fpad[~inner] == 0).all()
    assert torch.equal(ab, xr[:, 1:3])
    # the CPU's nearest selection agrees for these cases too
    assert torch.equal(ab.cpu(), F.interpolate(x.cpu(), scale_factor=sf)[:, 1:3])


def test_batch_independent_and_deterministic():
    case = ((3, 3, 44, 60), (3, 64, 22, 30), 3, 0.1, 0.5)
    xs, fs, k, alpha, sf = case
    x, f = _inputs(case, seed=3)
    full = _run(x, f, k, alpha, sf)
    again = _run(x, f, k, alpha, sf)
    assert torch.equal(full, again)
    for b in range(3):
        one = _run(x[b:b + 1].contiguous(), f[b:b + 1].contiguous(), k, alpha, sf)
        assert torch.equal(one, full[b:b + 1]), b
    # the benchmark map (N = 5184, several key splits per query block)
    x2, f2 = _inputs(CASES["bench_b2"], seed=4)
    full2 = _run(x2, f2, 3, 0.5, 0.25)
    for b in range(2):
        assert torch.equal(_run(x2[b:b + 1].contiguous(), f2[b:b + 1].contiguous(), 3, 0.5, 0.25), full2[b:b + 1]), b


def test_sharp_alpha_gives_convex_rows():
    """alpha = 1e-4 on unit-scale features (affinities / alpha ~ 1e6): every output finite and inside its image's
    per-channel [min, max] of the resized ab."""
    case = ((2, 3, 108, 192), (2, 128, 54, 96), 3, 1e-4, 0.5)
    x, _ = _inputs(case, seed=5)
    f = torch.rand(case[1], generator=torch.Generator().manual_seed(6)).cuda()
    out = _run(x, f, 3, 1e-4, 0.5)
    ab = F.interpolate(x, scale_factor=0.5)[:, 1:3]
    assert torch.isfinite(out).all()
    lo = ab.amin(dim=(2, 3), keepdim=True)
    hi = ab.amax(dim=(2, 3), keepdim=True)
    assert ((out >= lo) & (out <= hi)).all()
    # a row of identical affinities (constant feature) weighs every position equally: the plain mean of ab
    fc = torch.full((1, 4, 6, 10), 0.3, device="cuda")
    xc = x[:1, :, :6, :10].contiguous()
    outc = _run(xc, fc, 1, 1e-4, 1)
    mean = xc[:, 1:3].double().mean(dim=(2, 3), keepdim=True)
    assert (outc.double() - mean).abs().max().item() < 1e-4


def test_module_dropin_and_guards():
    from models.NonlocalNet import NonlocalWeightedAverage
    import dvc_amd.nonlocal_avg
    assert NonlocalWeightedAverage is dvc_amd.nonlocal_avg.NonlocalWeightedAverage
    m = NonlocalWeightedAverage()
    x, f = _inputs(CASES["nonint_resize"], seed=8)
    f.requires_grad_(True)
    with pytest.raises(NotImplementedError, match=r"\.detach\(\)"):
        m(x, f, scale_factor=0.25)
    with torch.no_grad():
        out = m(x, f, scale_factor=0.25)                       # defaults patch_size=3, alpha=0.1
    assert out.shape == (1, 2, 40, 64) and out.dtype == torch.float32 and out.device == x.device
    assert not out.requires_grad
    out2 = m(x, f.detach(), 3, 0.1, 0.25)
    assert torch.equal(out, out2)
    # default scale_factor = 1 and a double-precision input (cast like the contextual losses)
    y = m(x[:, :, :24, :40].double(), f.detach()[:, :, :12, :20].double())
    assert y.shape == (1, 2, 24, 40) and y.dtype == torch.float32
