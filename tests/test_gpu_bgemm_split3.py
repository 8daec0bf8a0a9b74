"""GPU: the bf16x3 split GEMM (csrc/bgemm_split3.hip through ops.bgemm(engine="split3")) against torch.matmul in float64 of the
same fp32 inputs, bit for bit against exact integer and one-hot products, and the training-side callers on it
(block_products' "split3" backend) against the float64 oracles and tolerances of tests/test_gpu_corr_backward.py and
tests/test_gpu_contextual.py.

Tolerance: the one the fp32 kernel is held to (tests/test_gpu_bgemm.py), (K + 2) 2^-24 (|A||B| + |C0|) elementwise, |A||B| the
float64 product of the absolute values.  What the split adds to an fp32 sum: the one dropped term product, a3 b3, at most
U / 250 |a||b| per product (tests/test_bgemm_split3_host.py); the eight kept products are exact in
fp32, and the large sum sees K / 16 accumulator additions.  The shapes are the fp32 test's: one element, odd sizes below a
tile, exact tiles, one-past-a-tile in every dimension with K % 16 = 2, a single tile with K = 5184 (split-K: 16 slices), and
2 x 2 tiles with a K tail of 6.

Measured on an MI355X over test_split3_vs_float64's 36 cases: the largest error / bound is 0.337 for split3 ((33, 65, 3),
batch 3, At_B and A_Bt) against 0.439 for the fp32 kernel (the same shape, A_B_acc; split3: 0.298); at K >= 66 split3 stays at 0.005 to 0.029 where the
fp32 kernel has 0.015 to 0.079, and both are below 0.0005 at K = 5184.  The worst ratio is below 1, so the bound is asserted
as it stands, with no constant in front."""
import functools

import numpy as np
import pytest
import torch

import bgemm_split3_reference as R
import test_gpu_contextual as TX
import test_gpu_corr_backward as TC

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
SHAPES = [(1, 1, 1), (33, 65, 3), (128, 128, 256), (130, 257, 66), (66, 64, 5184), (256, 192, 70)]
ORIENTS = ["At_B", "A_B_acc", "A_Bt"]          # scores; grad_cols_accumulate; grad_rows


@functools.lru_cache(maxsize=None)
def _case(M, N, K, batch, scale=1.0):
    """CPU inputs (A scaled by `scale` in fp32) and the float64 truth, computed once per case and never modified."""
    g = torch.Generator().manual_seed(1000 * M + 10 * N + K + batch)
    A = torch.randn(batch, M, K, generator=g) * scale
    B = torch.randn(batch, K, N, generator=g)
    C0 = torch.randn(batch, M, N, generator=g) * (K ** 0.5) * scale
    P64 = torch.matmul(A.double(), B.double())
    Pabs = torch.matmul(A.double().abs(), B.double().abs())
    return A, B, C0, P64, Pabs


def _offset_copy(t, off):
    """A device copy of `t` that starts `off` elements behind a fresh (256-byte aligned) allocation."""
    buf = torch.empty(t.numel() + off, device="cuda", dtype=torch.float32)
    v = buf[off:].view(t.shape)
    v.copy_(t)
    return v


def _operands(A, B, orient, off=0):
    """Device views of A [b, M, K] and B [b, K, N] in the memory orientation block_products uses for that product."""
    if orient == "At_B":
        return _offset_copy(A.transpose(1, 2).contiguous(), off).transpose(1, 2), _offset_copy(B, off)
    if orient == "A_B_acc":
        return _offset_copy(A, off), _offset_copy(B, off)
    return _offset_copy(A, off), _offset_copy(B.transpose(1, 2).contiguous(), off).transpose(1, 2)


def _ratio(got, P64, Pabs, C0, K):
    ref = P64 if C0 is None else P64 + C0.double()
    bound = (K + 2) * U * (Pabs if C0 is None else Pabs + C0.double().abs())
    return ((got.cpu().double() - ref).abs() / bound).max().item()


def _assert_within_bound(got, P64, Pabs, C0, K, what, fp32=None):
    ratio = _ratio(got, P64, Pabs, C0, K)
    beside = "" if fp32 is None else f"   (the fp32 kernel: {_ratio(fp32, P64, Pabs, C0, K):.3f})"
    print(f"bgemm split3 {what}: largest error / bound = {ratio:.3f}{beside}")
    assert torch.isfinite(got).all(), what
    assert ratio <= 1.0, f"{what}: error exceeds (K + 2) 2^-24 (|A||B| + |C0|): largest ratio to the bound {ratio:.3f}"


def _split3(a, b, **kw):
    from dvc_amd import ops
    return ops.bgemm(a, b, engine="split3", **kw)


@pytest.mark.parametrize("orient", ORIENTS)
@pytest.mark.parametrize("batch", [1, 3])
@pytest.mark.parametrize("M,N,K", SHAPES)
def test_split3_vs_float64(M, N, K, batch, orient):
    """Value, twice the same bits, and an `out` with ldc = N + 5 whose margin (NaN) stays untouched; without accumulate the
    interior starts as NaN and must come back finite.  The fp32 kernel's ratio on the same case is printed beside."""
    from dvc_amd import ops
    A, B, C0, P64, Pabs = _case(M, N, K, batch)
    a, b = _operands(A, B, orient)
    acc = orient == "A_B_acc"
    outs = []
    for _ in range(2):
        full = torch.full((batch, M, N + 5), float("nan"), device="cuda")
        out = full[:, :, :N]
        if acc:
            out.copy_(C0)
        r = _split3(a, b, out=out, accumulate=acc)
        assert r is out
        assert torch.isnan(full[:, :, N:]).all(), "the margin between N and ldc was written"
        outs.append(out)
    fp32 = ops.bgemm(a, b, out=C0.cuda(), accumulate=acc)
    _assert_within_bound(outs[0], P64, Pabs, C0 if acc else None, K, f"{orient} {M}x{N}x{K} batch {batch}", fp32)
    assert torch.equal(outs[0], outs[1]), "two runs differ"
    if not acc:
        fresh = _split3(a, b)
        assert fresh.is_contiguous() and torch.equal(fresh, outs[0])


@pytest.mark.parametrize("orient", ORIENTS)
@pytest.mark.parametrize("name", sorted(R.integer_cases()))
def test_split3_exact_cases_bit_for_bit(name, orient):
    """Integer operands whose every term product and partial sum is an integer below 2^24, and one-hot selections of
    full-precision values: any dropped, doubled or mispaired term changes the bits (what each case needs:
    bgemm_split3_reference.integer_cases).  Batch 2: the case and its negation."""
    A, B, C = (torch.from_numpy(np.stack([t, -t])) for t in R.integer_cases()[name])
    a, b = _operands(A, B, orient)
    C0 = torch.zeros_like(C) if orient == "A_B_acc" else None
    got = _split3(a, b, out=None if C0 is None else C0.cuda(), accumulate=C0 is not None)
    want = torch.stack([C[0], C[0]])                                        # (-A)(-B) = A B
    assert torch.equal(got.cpu(), want), f"{name} {orient}: {(got.cpu() != want).sum().item()} elements differ"


@pytest.mark.parametrize("orient", ORIENTS)
@pytest.mark.parametrize("scale", [1e-4, 1e4])
@pytest.mark.parametrize("M,N,K", [(33, 65, 3), (130, 257, 66), (66, 64, 5184)])
def test_split3_scaled_operands(M, N, K, scale, orient):
    A, B, C0, P64, Pabs = _case(M, N, K, 2, scale)
    a, b = _operands(A, B, orient)
    acc = orient == "A_B_acc"
    got = _split3(a, b, out=C0.cuda(), accumulate=acc)
    _assert_within_bound(got, P64, Pabs, C0 if acc else None, K, f"{orient} {M}x{N}x{K} A scaled by {scale:g}")


@pytest.mark.parametrize("orient", ORIENTS)
@pytest.mark.parametrize("M,N,K", [(130, 257, 66), (33, 65, 3), (66, 64, 5184)])
def test_split3_operands_one_element_off_16_bytes(M, N, K, orient):
    """Views that start 4 bytes behind a 16-byte boundary take the dword loads: same bound, and the same bits as the aligned
    call (the loads differ, the arithmetic does not)."""
    A, B, C0, P64, Pabs = _case(M, N, K, 3)
    acc = orient == "A_B_acc"
    res = []
    for off in (0, 1):
        a, b = _operands(A, B, orient, off)
        assert a.data_ptr() % 16 == 4 * off and b.data_ptr() % 16 == 4 * off
        out = _offset_copy(C0, off)
        res.append(_split3(a, b, out=out, accumulate=acc))
    _assert_within_bound(res[1], P64, Pabs, C0 if acc else None, K, f"{orient} {M}x{N}x{K} off by one element")
    assert torch.equal(res[0], res[1])


def test_split3_column_slice_of_the_rows_operand():
    """block_products' views of a ragged block of 70 rows starting at row 64 of L [B, C, 200] against M [B, C, 150]:
    S = L_blk^T M, d M += L_blk dS, d L_blk = M dS^T."""
    g = torch.Generator().manual_seed(7)
    Bn, C, Nl, Nm, rows = 2, 66, 200, 150, 70
    L, Mm = torch.randn(Bn, C, Nl, generator=g), torch.randn(Bn, C, Nm, generator=g)
    dS, dM0 = torch.randn(Bn, rows, Nm, generator=g), torch.randn(Bn, C, Nm, generator=g)
    Ld, Md, dSd = L.cuda(), Mm.cuda(), dS.cuda()
    blk, blk64 = Ld[:, :, 64:64 + rows], L[:, :, 64:64 + rows].double()
    S = _split3(blk.transpose(1, 2), Md)
    _assert_within_bound(S, blk64.transpose(1, 2) @ Mm.double(), blk64.abs().transpose(1, 2) @ Mm.double().abs(), None, C, "slice: scores")
    dM = dM0.cuda()
    _split3(blk, dSd, out=dM, accumulate=True)
    _assert_within_bound(dM, blk64 @ dS.double(), blk64.abs() @ dS.double().abs(), dM0, rows, "slice: grad_cols")
    dL = torch.full((Bn, C, Nl), float("nan"), device="cuda")
    _split3(Md, dSd.transpose(1, 2), out=dL[:, :, 64:64 + rows])
    _assert_within_bound(dL[:, :, 64:64 + rows], Mm.double() @ dS.double().transpose(1, 2),
                         Mm.double().abs() @ dS.double().abs().transpose(1, 2), None, Nm, "slice: grad_rows")
    assert torch.isnan(dL[:, :, :64]).all() and torch.isnan(dL[:, :, 64 + rows:]).all()


@pytest.mark.parametrize("orient", ORIENTS)
@pytest.mark.parametrize("M,N,K", [(66, 64, 5184), (130, 257, 66)])
def test_split3_image_bits_do_not_depend_on_the_batch(M, N, K, orient):
    """Image 1 of a batch of 3 against the same image alone, bit for bit; (66, 64, 5184) takes the split-K path."""
    from dvc_amd import _lib
    assert (_lib.load().dvc_bgemm_split3_workspace_bytes(3, M, N, K) > 0) == (K == 5184)
    A, B, C0, _, _ = _case(M, N, K, 3)
    acc = orient == "A_B_acc"
    a, b = _operands(A, B, orient)
    whole = _split3(a, b, out=C0.cuda(), accumulate=acc)
    a1, b1 = _operands(A[1:2], B[1:2], orient)
    alone = _split3(a1, b1, out=C0[1:2].cuda(), accumulate=acc)
    assert torch.equal(whole[1:2], alone)
    assert torch.equal(_split3(a[1:2], b[1:2], out=C0[1:2].cuda(), accumulate=acc), alone)     # a batch-1 view of the batch


@pytest.mark.parametrize("orient", ORIENTS)
def test_split3_special_values(orient):
    """The contract of the header comment: an Inf or NaN input makes exactly the output elements non-finite that the fp32
    kernel makes non-finite (rows of A's, columns of B's); zero rows and columns give exact zeros; FLT_MAX is selected intact
    (no term of a finite value is infinite); inputs near 2^-110 give finite results."""
    from dvc_amd import ops
    M, N, K = 70, 130, 40
    A, B, _, _, _ = _case(M, N, K, 2)
    A, B = A.clone(), B.clone()
    A[0, 3, 17], A[1, 69, 39], A[0, 40, 0] = float("inf"), float("nan"), float("-inf")
    B[0, 16, 129], B[1, 5, 64] = float("inf"), float("nan")
    A[:, 10], B[:, :, 7] = 0.0, 0.0
    a, b = _operands(A, B, orient)
    acc = orient == "A_B_acc"
    got = _split3(a, b, out=torch.zeros(2, M, N, device="cuda"), accumulate=acc)
    fp32 = ops.bgemm(a, b, out=torch.zeros(2, M, N, device="cuda"), accumulate=acc)
    bad = ~torch.isfinite(fp32)
    assert torch.equal(~torch.isfinite(got), bad)
    assert bad[0, 3].all() and bad[0, 40].all() and bad[0, :, 129].all() and bad[1, 69].all() and bad[1, :, 64].all()
    assert bad.sum() == 3 * N + 2 * M - 3                                 # those three rows and two columns, nothing else
    assert (got[:, 10][~bad[:, 10]] == 0).all() and (got[:, :, 7][~bad[:, :, 7]] == 0).all()
    # FLT_MAX through a one-hot column, and tiny operands
    fmax = torch.finfo(torch.float32).max
    A2 = torch.full((1, M, K), fmax)
    A2[0, 1::2] = -fmax
    B2 = torch.zeros(1, K, N)
    B2[0, torch.arange(N) % K, torch.arange(N)] = 1.0
    a, b = _operands(A2, B2, orient)
    got = _split3(a, b, out=torch.zeros(1, M, N, device="cuda"), accumulate=acc)
    assert torch.equal(got.cpu(), A2[:, :, :1].expand(1, M, N))
    At, Bt = _case(M, N, K, 2)[0] * 2.0 ** -110, _case(M, N, K, 2)[1]
    a, b = _operands(At, Bt, orient)
    assert torch.isfinite(_split3(a, b, out=torch.zeros(2, M, N, device="cuda"), accumulate=acc)).all()


def test_split3_refusals_on_device():
    a, b = torch.zeros(2, 8, 6, device="cuda"), torch.zeros(2, 6, 4, device="cuda")
    with pytest.raises(RuntimeError, match="float32"):
        _split3(a.double(), b)
    with pytest.raises(RuntimeError, match="float32"):
        _split3(a[0], b[0])
    with pytest.raises(RuntimeError, match="inner stride"):
        _split3(torch.zeros(2, 8, 12, device="cuda")[:, :, ::2], b)
    with pytest.raises(RuntimeError, match="do not match"):
        _split3(a, b[:, :5])
    with pytest.raises(RuntimeError, match="accumulate needs"):
        _split3(a, b, accumulate=True)
    with pytest.raises(RuntimeError, match="unit inner stride"):
        _split3(a, b, out=torch.zeros(2, 4, 8, device="cuda").transpose(1, 2))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        _split3(a, b.cpu())
    with pytest.raises(ValueError, match="bogus"):
        from dvc_amd import ops
        ops.bgemm(a, b, engine="bogus")


# ---------------------------------------------------------------------------------------------- through the public callers
@pytest.fixture
def split3():
    from dvc_amd import block_products as bp
    assert bp.backend() is None
    with bp.use_backend("split3"):
        yield bp
    assert bp.backend() is None


def _count_split3_products(monkeypatch):
    from dvc_amd import block_products as bp
    calls = []

    def counted(*a, **kw):
        calls.append(1)
        return _split3(*a, **kw)
    monkeypatch.setattr(bp._Split3, "product", staticmethod(counted))
    return calls


def test_split3_fused_correlation_over_ragged_row_blocks(split3, monkeypatch):
    """tests/test_gpu_corr_backward.py's several-row-blocks check at (h, w, B, T) = (12, 20, 2, 0.01) (ROW_BLOCK = 64: 240 rows
    = 3 x 64 + 48; chunk 1), its oracle and its tolerances, with the three products on the split GEMM."""
    calls = _count_split3_products(monkeypatch)
    TC.test_fused_correlation_backward_over_several_row_blocks(12, 20, 2, 0.01, 4 * 64 * 240, "split3-gemm", monkeypatch)
    assert len(calls) >= 3


@pytest.mark.parametrize("C,H,W,B", [(256, 27, 48, 2), (512, 13, 24, 2)])
def test_split3_contextual_losses(C, H, W, B, split3, monkeypatch):
    """ContextualLoss and ContextualLoss_forward through tests/test_gpu_contextual.py's checker (float64 autograd, its
    tolerances, run-to-run equality)."""
    calls = _count_split3_products(monkeypatch)
    TX._check_vs_float64_autograd(C, H, W, B, 0.1, True)
    assert len(calls) >= 2


def test_the_earlier_backend_is_back_after_the_block():
    from dvc_amd import block_products as bp
    assert bp.backend() is None
    with bp.use_backend("native"):
        with bp.use_backend("split3"):
            assert bp.backend() == "split3"
        assert bp.backend() == "native"
    assert bp.backend() is None
