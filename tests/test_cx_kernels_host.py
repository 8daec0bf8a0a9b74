"""No GPU: pins tests/cx_kernels_reference.py, the float64 restatement that tests/test_gpu_cx_kernels.py holds the kernels to,
against oracle/contextual_oracle.py and oracle/dvc_oracle.py (themselves pinned to the reference modules), and its tie rules
and bounds against constructed inputs."""
import pytest
import torch
import torch.nn.functional as F

import cx_kernels_reference as R
from oracle import contextual_oracle as O

SHAPES = [(64, 150, 126), (16, 70, 129)]
FNS = {0: O.contextual_loss_forward, 1: O.contextual_loss}


@pytest.mark.parametrize("h", [0.1, 0.5])
@pytest.mark.parametrize("C,Nx,Ny", SHAPES)
def test_loss_of_S_is_the_oracle_loss(C, Nx, Ny, h):
    """loss(S), S = Xn^T Yn in float64, against both oracle losses on the same features: 1e-12; and its autograd dS pushed
    through the product and the normalise against the oracle's autograd dX: 1e-10 of the largest gradient."""
    B = 2
    X, Y, _, _ = R.features(7 + C, B, C, Nx, Ny)
    gout = torch.tensor([0.5, 1.5], dtype=torch.float64)
    for mode, fn in FNS.items():
        x = X.double().requires_grad_(True)
        lo = fn(x, Y.double(), h=h)
        (lo * gout).sum().backward()
        x2 = X.double().requires_grad_(True)
        y = Y.double()
        mu = y.mean(-1, keepdim=True)
        Xn, Yn = O.feature_normalize(x2 - mu).view(B, C, Nx), O.feature_normalize(y - mu).view(B, C, Ny)
        S = torch.matmul(Xn.transpose(1, 2), Yn)
        lr = R.loss(S, h, mode)
        assert (lr - lo).abs().max().item() <= 1e-12 * max(1.0, lo.abs().max().item())
        S.backward(R.ds(S.detach(), h, mode, gout.view(B)))
        err, scale = (x2.grad - x.grad).abs().max().item(), x.grad.abs().max().item()
        assert err <= 1e-10 * scale, (mode, err, scale)
        # the forward pieces agree with the same loss
        a, jstar, l, r, e = R.rows_stats(S.detach(), h)
        cmax, _ = R.col_max(S.detach(), a, l, h)
        for v, m in ((r, 0), (cmax, 1)):
            if m == mode:
                assert (R.finish(v)[0] - lo.detach()).abs().max().item() <= 1e-12 * max(1.0, lo.abs().max().item())


def _tie_S():
    S = R.scores(3, 1, 16, 6, 9)
    S[0, 2, 7] = S[0, 2, 1] = S[0, 2].max() + 0.125        # row 2: its maximum twice, columns 1 and 7
    return S


def test_row_tie_gradient_goes_to_the_lowest_index():
    """Row maximum at columns 1 and 7: jstar is 1, and dS equals the limit of 'column 7 a hair lower' (column 1 the only
    maximum), not of 'column 1 a hair lower'."""
    S = _tie_S()
    assert R.rows_stats(S, 0.1)[1][0, 2].item() == 1 and R.lowest_argmax(S.double(), -1)[0, 2].item() == 1
    g = R.ds(S, 0.1, 0)
    lo, hi = S.double().clone(), S.double().clone()
    lo[0, 2, 7] -= 1e-12
    hi[0, 2, 1] -= 1e-12
    g_lo, g_hi = R.ds(lo, 0.1, 0), R.ds(hi, 0.1, 0)
    scale = g.abs().max().item()
    assert (g - g_lo).abs().max().item() <= 1e-8 * scale
    assert (g - g_hi).abs().max().item() >= 1e-2 * scale
    assert g[0, 2, 1].item() != g[0, 2, 7].item()


def test_column_tie_gradient_goes_to_the_lowest_row():
    """Rows 1 and 4 identical (A bit-identical): every column they win goes to row 1; row 4 owns nothing, so T = Q = 0 and its
    dS is exactly zero, while row 1 carries the gradient."""
    S = R.scores(4, 1, 16, 6, 9)
    S[0, 4] = S[0, 1] = S[0, 1] + 0.25
    a, jstar, l, r, e = R.rows_stats(S, 0.1)
    cmax, cargi = R.col_max(S, a, l, 0.1)
    assert (cargi == 1).any() and not (cargi == 4).any()
    t, q = R.rows_tq(S, a, l, cargi, 0, 0.1)
    assert t[0, 4].item() == 0.0 and q[0, 4].item() == 0.0 and t[0, 1].item() > 0
    g = R.ds(S, 0.1, 1)
    assert (g[0, 4] == 0).all() and g[0, 1].abs().max().item() > 0


def test_col_max_carried_in_value_wins_ties():
    """Blocks of 4 rows over 10 rows with rows 1 and 6 identical (a tie across two blocks) and rows 2 and 3 identical (inside
    one): the chain of three calls equals the one call, and equals the lowest row of the float64 maximum."""
    S = R.scores(5, 2, 16, 10, 21)
    S[:, 6] = S[:, 1] = S[:, 1] + 0.2
    S[:, 3] = S[:, 2] = S[:, 2] + 0.2
    a, _, l, _, _ = R.rows_stats(S, 0.1)
    whole = R.col_max(S, a, l, 0.1)
    cm, ci = torch.full((2, 21), -1.0, dtype=torch.float64), torch.zeros((2, 21), dtype=torch.long)
    for i0 in (0, 4, 8):
        sl = slice(i0, min(i0 + 4, 10))
        cm, ci = R.col_max(S[:, sl], a[:, sl], l[:, sl], 0.1, i0, cm, ci)
    assert torch.equal(cm, whole[0]) and torch.equal(ci, whole[1])
    assert not torch.isin(ci, torch.tensor([3, 6])).any() and torch.isin(torch.tensor([1, 2]), ci).all()


def test_normalize_bwd_is_the_autograd_of_the_normalise():
    g = torch.Generator().manual_seed(1)
    x = torch.randn(2, 7, 5, generator=g, dtype=torch.float64)
    x[1, :, 3] = 0
    dxn = torch.randn(2, 7, 5, generator=g, dtype=torch.float64)
    eps = 2.0 ** -52
    xl = x.clone().requires_grad_(True)
    O.feature_normalize(xl).backward(dxn)
    n = x.norm(dim=1)
    got = R.normalize_bwd(x / (n.unsqueeze(1) + eps), n, dxn, eps)
    assert (got - xl.grad)[:, :, :3].abs().max().item() <= 1e-12 * xl.grad.abs().max().item()
    assert torch.equal(got[1, :, 3], dxn[1, :, 3] / eps) and torch.isfinite(got).all()


@pytest.mark.parametrize("wta", [1.0, 0.5])
def test_softmax_bwd_is_the_autograd_of_the_reference_ops(wta):
    """Against float64 autograd through oracle.wta_scale, / T, softmax, the colour product and the row maximum.  The restatement
    rounds f' / T to float32 first, as the kernel does: u |z| <= 2^-24 * 20 relative in p at T = 0.05, pinned at 1e-4."""
    from oracle import dvc_oracle as D
    B, rows, P, T = 2, 9, 13, 0.05
    g = torch.Generator().manual_seed(2)
    f = (torch.rand(B, rows, P, generator=g) * 1.6 - 0.8).float()
    f[0, 3, 2] = f[0, 3, 11] = 0.9                                       # a raw-maximum tie
    blab, gy, gsim = torch.randn(B, 3, P, generator=g) * 30, torch.randn(B, 3, rows, generator=g), torch.randn(B, rows, generator=g)
    f64 = f.double().requires_grad_(True)
    fw = f64 if wta == 1.0 else D.wta_scale(f64, wta)
    y64 = torch.matmul(F.softmax(fw / float(torch.tensor(T, dtype=torch.float32)), dim=-1), blab.double().permute(0, 2, 1)).permute(0, 2, 1)
    am = R.lowest_argmax(f.double(), -1)
    ((y64 * gy.double()).sum() + (f64.gather(-1, am.unsqueeze(-1)).squeeze(-1) * gsim.double()).sum()).backward()
    got, bound = R.softmax_bwd(f, blab, gy, y64.detach(), gsim, am, T, wta, with_bound=True)
    assert (got - f64.grad).abs().max().item() <= 1e-4 * f64.grad.abs().max().item()
    assert (bound > 0).all() and torch.isfinite(bound).all()


@pytest.mark.parametrize("C,Nx,Ny,h", [(64, 150, 126, 0.1), (8, 3, 63, 0.1), (16, 70, 129, 0.5), (16, 17, 1025, 0.1)])
def test_float32_evaluation_stays_inside_the_bounds(C, Nx, Ny, h):
    """The same steps in float32 on the CPU (another summation order than the kernel's, the same roundings per element): inside
    the l, r, e and A bounds, which therefore are not tighter than float32 allows."""
    S = R.scores(11 + C, 1, C, Nx, Ny)
    h32 = float(torch.tensor(h, dtype=torch.float32))
    a, jstar, l, r, e = R.rows_stats(S, h32)
    dl, dr, de = R.rows_bounds(S, h32)
    m = S.max(-1)[0]
    a32 = (1 - m) + torch.tensor(1e-5, dtype=torch.float32)
    w32 = torch.exp((1 - (1 - S) / a32.unsqueeze(-1)) / torch.tensor(h, dtype=torch.float32))
    l32 = w32.sum(-1)
    r32 = w32.gather(-1, jstar.unsqueeze(-1)).squeeze(-1) / l32
    e32 = (w32 * (1 - S)).sum(-1) / l32
    assert ((a32.double() - a).abs() <= 2 * R.ulp32(a)).all()
    for got, ref, bound in ((l32, l, dl), (r32, r, dr), (e32, e, de)):
        ratio = ((got.double() - ref).abs() / bound).max().item()
        assert ratio <= 1.0, ratio
    af, lf = a.float(), l.float()
    A32 = torch.exp((1 - (1 - S) / af.unsqueeze(-1)) / torch.tensor(h, dtype=torch.float32)) / lf.unsqueeze(-1)
    assert ((A32.double() - R.affinity(S, af, lf, h32)).abs() / R.A_bound(S, af, lf, h32)).max().item() <= 1.0
