"""GPU: WeightedAverage_color (dvc_lwa_fwd / dvc_lwa_bwd, csrc/local_avg.hip) against the float64 restatement
(tests/lwa_reference.py): forward and both gradients, determinism / batch / grad-mode independence, sharp and soft alpha,
the drop-in module, train.py's chain and the memory the fused path needs."""
import functools
import inspect
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lwa_reference as R  # noqa: E402

pytestmark = pytest.mark.gpu

# x_lab shape, pred shape, patch_size, alpha, scale_factor
CASES = {
    "train": ((2, 3, 24, 40), (2, 3, 24, 40), 3, 10, 1),        # train.py's call
    "odd": ((1, 3, 37, 53), (1, 3, 37, 53), 3, 1, 1),           # sizes that are no multiple of the 8 x 32 tile
    "k5": ((2, 3, 19, 23), (2, 3, 19, 23), 5, 300, 1),
    "k7": ((1, 3, 11, 70), (1, 3, 11, 70), 7, 50, 1),
    "k1": ((1, 3, 6, 5), (1, 3, 6, 5), 1, 1, 1),                # y == v bit for bit, dv == G, dg == 0
    "tiny": ((1, 3, 2, 3), (1, 3, 2, 3), 5, 10, 1),             # map smaller than the halo
    "half": ((1, 3, 46, 58), (1, 3, 23, 29), 3, 10, 0.5),
    "nonint": ((1, 4, 27, 45), (1, 5, 20, 33), 3, 10, 0.75),    # extra channels on both inputs
    "dark": ((1, 3, 16, 20), (1, 3, 16, 20), 3, 10, 1),         # g ~ 0: out-of-image neighbours weigh like real ones
    "frame": ((2, 3, 216, 384), (2, 3, 216, 384), 3, 10, 1),    # one size-of-workload check
}
DG_CASES = [n for n, c in CASES.items() if c[4] == 1 or n == "half"]


def _inputs(name, seed=0):
    """CPU float32 (x_lab, pred, G).  The guide is noise of std sqrt(alpha / 6) on a per-image constant colour (D / alpha ~ 1:
    spread weights), ab values are U(-110, 110)."""
    xs, ps, k, alpha, sf = CASES[name] if isinstance(name, str) else name
    g = torch.Generator().manual_seed(seed)
    if name == "dark":
        x = torch.cat((-50 + torch.rand((xs[0], 1) + xs[2:], generator=g), torch.rand((xs[0], xs[1] - 1) + xs[2:], generator=g) * 2 - 1), 1)
    else:
        colour = torch.rand(xs[0], xs[1], 1, 1, generator=g) * torch.tensor([100.0] + [160.0] * (xs[1] - 1)).view(1, -1, 1, 1) \
            - torch.tensor([50.0] + [80.0] * (xs[1] - 1)).view(1, -1, 1, 1)
        x = colour + torch.randn(xs, generator=g) * (alpha / 6) ** 0.5
    p = torch.rand(ps, generator=g) * 220 - 110
    G = torch.randn((ps[0], 2) + ps[2:], generator=g)
    return x, p, G


@functools.lru_cache(maxsize=None)
def _reference(name):
    """Computed once per case and shared: inputs, float64 (y, dx, dp) and the float32 CPU composition's own."""
    xs, ps, k, alpha, sf = CASES[name]
    x, p, G = _inputs(name)
    return (x, p, G), R.gradients(x, p, G, k, alpha, sf, torch.float64), R.gradients(x, p, G, k, alpha, sf, torch.float32)


def _module():
    from dvc_amd.local_avg import WeightedAverage_color
    return WeightedAverage_color()


def _fwd_bwd(x, p, G, k, alpha, sf, guide_grad):
    """(y, dx or None, dp) of the module on the device."""
    x = x.cuda().requires_grad_(guide_grad)
    p = p.cuda().requires_grad_(True)
    y = _module()(x, p, k, alpha, sf)
    y.backward(G.cuda())
    torch.cuda.synchronize()
    return y.detach(), x.grad, p.grad


def _rel(got, ref):
    return (got.double() - ref.double()).abs().max().item() / ref.abs().max().item()


@pytest.mark.parametrize("name", list(CASES))
def test_forward_matches_float64_restatement(name):
    xs, ps, k, alpha, sf = CASES[name]
    (x, p, G), (y64, _, _), (y32, _, _) = _reference(name)
    with torch.no_grad():
        got = _module()(x.cuda(), p.cuda(), k, alpha, sf)
    assert got.shape == y64.shape and got.dtype == torch.float32
    got = got.cpu().double()
    err, err32 = (got - y64).abs().max().item(), (y32.double() - y64).abs().max().item()
    tol = 4 * err32 + 1e-6 * y64.abs().max().item()
    print(f"{name}: forward max-abs err {err:.3e}, fp32 CPU restatement {err32:.3e}, bound {tol:.3e}")
    assert torch.isfinite(got).all()
    assert err <= tol, (name, err, err32)
    if name == "k1":
        assert torch.equal(got.float(), p[:, 1:3])


@pytest.mark.parametrize("name", list(CASES))
def test_backward_matches_float64_autograd(name):
    xs, ps, k, alpha, sf = CASES[name]
    (x, p, G), (_, dx64, dp64), (_, dx32, dp32) = _reference(name)
    want_dg = name in DG_CASES
    if name in ("train", "k5", "dark"):
        # the check below must not pass on an all-but-zero tensor
        assert dx64.abs().max().item() > 1e-3 * G.abs().max().item()
    y, dx, dp = _fwd_bwd(x, p, G, k, alpha, sf, want_dg)
    assert dp.shape == p.shape and dp.dtype == p.dtype
    err, err32 = _rel(dp.cpu(), dp64), _rel(dp32, dp64)
    tol = max(1e-6, 4 * err32)
    print(f"{name}: dv rel err {err:.3e}, fp32 CPU autograd {err32:.3e}, bound {tol:.3e}")
    assert torch.isfinite(dp).all() and err <= tol, (name, "dv", err, err32)
    assert (dp[:, 0] == 0).all() and (dp[:, 3:] == 0).all()
    if name == "k1":
        assert torch.equal(dp[:, 1:3].cpu(), G)
    if not want_dg:
        assert dx is None
        return
    assert dx.shape == x.shape and dx.dtype == x.dtype
    assert (dx[:, 3:] == 0).all()
    if name == "k1":
        assert (dx == 0).all() and (dx64 == 0).all()
        return
    err, err32 = _rel(dx.cpu(), dx64), _rel(dx32, dx64)
    tol = max(1e-6, 4 * err32)
    print(f"{name}: dg rel err {err:.3e}, fp32 CPU autograd {err32:.3e}, bound {tol:.3e} (max |dg| {dx64.abs().max().item():.3e})")
    assert torch.isfinite(dx).all() and err <= tol, (name, "dg", err, err32)


def test_deterministic_batch_and_grad_mode_independent():
    case = ((3, 3, 22, 30), (3, 3, 22, 30), 3, 10, 1)
    x, p, G = _inputs(case, seed=3)
    y, dx, dp = _fwd_bwd(x, p, G, 3, 10, 1, True)
    y2, dx2, dp2 = _fwd_bwd(x, p, G, 3, 10, 1, True)
    assert torch.equal(y, y2) and torch.equal(dx, dx2) and torch.equal(dp, dp2)
    with torch.no_grad():
        assert torch.equal(_module()(x.cuda(), p.cuda(), 3, 10, 1), y)
    # dv alone (the guide without a gradient: the launch's other branch) gives the same dv
    _, none, dp3 = _fwd_bwd(x, p, G, 3, 10, 1, False)
    assert none is None and torch.equal(dp3, dp)
    for b in range(3):
        yb, dxb, dpb = _fwd_bwd(x[b:b + 1], p[b:b + 1], G[b:b + 1], 3, 10, 1, True)
        assert torch.equal(yb, y[b:b + 1]) and torch.equal(dxb, dx[b:b + 1]) and torch.equal(dpb, dp[b:b + 1]), b


def test_sharp_and_soft_alpha():
    x, p, _ = _inputs("odd", seed=5)
    m = _module()
    with torch.no_grad():
        y = m(x.cuda(), p.cuda(), 3, 1e-6, 1)
        v = p[:, 1:3].cuda()
        assert torch.isfinite(y).all()
        lo = v.amin(dim=(2, 3), keepdim=True).clamp(max=0)
        hi = v.amax(dim=(2, 3), keepdim=True).clamp(min=0)
        assert ((y >= lo) & (y <= hi)).all()
        y = m(x.cuda(), p.cuda(), 3, 1e12, 1)
        mean = F.avg_pool2d(v.double(), 3, stride=1)                   # interior pixels: the plain 3 x 3 mean
        assert (y[:, :, 1:-1, 1:-1].double() - mean).abs().max().item() <= 1e-4 * v.abs().max().item()


def test_module_dropin_defaults_and_dtypes():
    from models.NonlocalNet import WeightedAverage_color
    import dvc_amd.local_avg
    assert WeightedAverage_color is dvc_amd.local_avg.WeightedAverage_color
    sig = inspect.signature(WeightedAverage_color.forward)
    assert [(n, q.default) for n, q in list(sig.parameters.items())[3:]] == [("patch_size", 3), ("alpha", 1), ("scale_factor", 1)]
    assert [(n, q.default) for n, q in list(inspect.signature(dvc_amd.local_avg.weighted_average_color).parameters.items())[2:]] \
        == [("patch_size", 3), ("alpha", 1), ("scale_factor", 1)]
    m = WeightedAverage_color()
    x, p, G = _inputs("train", seed=8)
    x, p = x.cuda(), p.cuda()
    with torch.no_grad():
        base = m(x, p, 3, 1, 1)
        assert torch.equal(m(x, p), base)                              # the defaults
    assert base.dtype == torch.float32 and base.device == x.device and not base.requires_grad
    # double, non-contiguous inputs (a channels-last copy and a slice of a wider tensor)
    xd = x.double().contiguous(memory_format=torch.channels_last).requires_grad_(True)
    wide = torch.zeros(2, 3, 24, 44, device="cuda", dtype=torch.float64)
    wide[..., 2:42] = p
    wide.requires_grad_(True)
    pd = wide[..., 2:42]
    assert not xd.is_contiguous() and not pd.is_contiguous()
    y = m(xd, pd)
    assert y.dtype == torch.float32 and torch.equal(y, base)
    y.backward(G.cuda())
    assert xd.grad.dtype == torch.float64 and xd.grad.shape == xd.shape
    assert wide.grad.dtype == torch.float64 and wide.grad.shape == wide.shape
    assert (wide.grad[..., :2] == 0).all() and (wide.grad[:, 0] == 0).all() and wide.grad[:, 1:3].abs().max() > 0


def test_train_chain_matches_float64_autograd():
    """train.py's smoothness term: the gradient reaches ab through cat(L, ab) and through the loss's first argument."""
    (x, p, _), _, _ = _reference("train")
    L, ab0 = p[:, 0:1], p[:, 1:3]

    def chain(layer, x_lab, L, ab):
        ab = ab.detach().clone().requires_grad_(True)
        loss = F.mse_loss(ab, layer(x_lab, torch.cat((L, ab), 1), 3, 10, 1))
        loss.backward()
        return loss.detach(), ab.grad

    def cpu_layer(xl, pr, k, alpha, sf):
        return R.compose(F.interpolate(xl, scale_factor=sf), pr, k, alpha)

    l64, g64 = chain(cpu_layer, x.double(), L.double(), ab0.double())
    l32, g32 = chain(cpu_layer, x, L, ab0)
    lg, gg = chain(_module(), x.cuda(), L.cuda(), ab0.cuda())
    torch.cuda.synchronize()
    err, err32 = _rel(gg.cpu(), g64), _rel(g32, g64)
    tol = max(1e-6, 4 * err32)
    print(f"train chain: d ab rel err {err:.3e}, fp32 CPU autograd {err32:.3e}, bound {tol:.3e}; loss {lg.item():.6e} / {l64.item():.6e}")
    assert err <= tol, (err, err32)
    assert abs(lg.item() - l64.item()) <= max(1e-6, 4 * abs(l32.item() - l64.item()) / l64.item()) * l64.item()


def test_memory_is_a_fraction_of_the_compositions():
    """Forward + backward (dv only) at (4, 3, 108, 192), k = 3: the fused path allocates y, the gradient buffers and the two
    sliced inputs — about ten planes — where the composition keeps five 9x unfolded tensors and the k*k-plane softmax chain:
    over 45 planes.  Derived, not measured: at most a third."""
    case = ((4, 3, 108, 192), (4, 3, 108, 192), 3, 10, 1)
    x, p, G = _inputs(case, seed=9)
    x, G = x.cuda(), G.cuda()

    def growth(layer):
        pp = p.cuda().requires_grad_(True)
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        layer(x, pp, 3, 10, 1).backward(G)
        torch.cuda.synchronize()
        return torch.cuda.max_memory_allocated() - base

    fused = growth(_module())
    comp = growth(lambda xl, pr, k, alpha, sf: R.compose(xl, pr, k, alpha))
    plane = 4 * 4 * 108 * 192
    print(f"memory growth: fused {fused / plane:.1f} planes, torch composition {comp / plane:.1f} planes")
    assert fused <= comp / 3, (fused, comp)
