"""GPU: the library's own batched fp32 GEMM (csrc/bgemm.hip through ops.bgemm) against torch.matmul in float64 of the same fp32
inputs, and the training-side callers on it (block_products' "native" backend) against the float64 oracles and tolerances of
tests/test_gpu_corr_backward.py and tests/test_gpu_contextual.py.

Tolerance (derived, not measured): an fp32 sum of K products in any order, each product rounded once, plus the rounding of
the accumulate, is within (K + 2) 2^-24 (|A| |B| + |C0|) of the exact value, elementwise, |A| |B| the float64 matrix product of
the absolute values.  The split-K path (slices of K / S products, then S - 1 additions of the partial sums) stays inside the
same bound: (K / S + S) <= K + 2 for every K it splits.

Shapes are the smallest at which the tiling can go wrong (128 x 128 tiles, K steps of 16, 32 x 32 MFMA tiles): one element, odd
sizes below a tile, exact tiles, one-past-a-tile in every dimension with K % 16 = 2, a single tile with K = 5184 (the split-K
path: 16 slices), and 2 x 2 tiles with a K tail of 6."""
import functools

import pytest
import torch

import test_gpu_contextual as TX
import test_gpu_corr_backward as TC

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
SHAPES = [(1, 1, 1), (33, 65, 3), (128, 128, 256), (130, 257, 66), (66, 64, 5184), (256, 192, 70)]
ORIENTS = ["At_B", "A_B_acc", "A_Bt"]          # scores; grad_cols_accumulate; grad_rows


@functools.lru_cache(maxsize=None)
def _case(M, N, K, batch):
    """CPU inputs and the float64 truth, computed once per (shape, batch) and never modified."""
    g = torch.Generator().manual_seed(1000 * M + 10 * N + K + batch)
    A = torch.randn(batch, M, K, generator=g)
    B = torch.randn(batch, K, N, generator=g)
    C0 = torch.randn(batch, M, N, generator=g) * (K ** 0.5)
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


def _assert_within_bound(got, P64, Pabs, C0, K, what):
    ref = P64 if C0 is None else P64 + C0.double()
    bound = (K + 2) * U * (Pabs if C0 is None else Pabs + C0.double().abs())
    err = (got.cpu().double() - ref).abs()
    ratio = (err / bound).max().item()
    print(f"bgemm {what}: largest error / bound = {ratio:.3f}")
    assert torch.isfinite(got).all(), what
    assert ratio <= 1.0, f"{what}: error exceeds (K + 2) 2^-24 (|A||B| + |C0|): largest ratio to the bound {ratio:.3f}"


@pytest.mark.parametrize("orient", ORIENTS)
@pytest.mark.parametrize("batch", [1, 3])
@pytest.mark.parametrize("M,N,K", SHAPES)
def test_bgemm_vs_float64(M, N, K, batch, orient):
    """Value, twice the same bits, and an `out` with ldc = N + 5 whose margin (NaN) stays untouched; without accumulate the
    interior starts as NaN and must come back finite."""
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
        r = ops.bgemm(a, b, out=out, accumulate=acc)
        assert r is out
        assert torch.isnan(full[:, :, N:]).all(), "the margin between N and ldc was written"
        outs.append(out)
    torch.cuda.synchronize()
    _assert_within_bound(outs[0], P64, Pabs, C0 if acc else None, K, f"{orient} {M}x{N}x{K} batch {batch}")
    assert torch.equal(outs[0], outs[1]), "two runs differ"
    fresh = ops.bgemm(a, b) if not acc else None
    if fresh is not None:
        assert fresh.is_contiguous() and torch.equal(fresh, outs[0])


@pytest.mark.parametrize("orient", ORIENTS)
@pytest.mark.parametrize("M,N,K", [(130, 257, 66), (33, 65, 3), (66, 64, 5184)])
def test_bgemm_operands_one_element_off_16_bytes(M, N, K, orient):
    """Views that start 4 bytes behind a 16-byte boundary take the dword loads: same bound, and the same bits as the aligned
    call (the loads differ, the arithmetic does not)."""
    from dvc_amd import ops
    A, B, C0, P64, Pabs = _case(M, N, K, 3)
    acc = orient == "A_B_acc"
    res = []
    for off in (0, 1):
        a, b = _operands(A, B, orient, off)
        assert a.data_ptr() % 16 == 4 * off and b.data_ptr() % 16 == 4 * off
        out = _offset_copy(C0, off)
        res.append(ops.bgemm(a, b, out=out, accumulate=acc))
    _assert_within_bound(res[1], P64, Pabs, C0 if acc else None, K, f"{orient} {M}x{N}x{K} off by one element")
    assert torch.equal(res[0], res[1])


def test_bgemm_column_slice_of_the_rows_operand():
    """block_products' views of a ragged block of 70 rows starting at row 64 of L [B, C, 200] against M [B, C, 150]:
    S = L_blk^T M, d M += L_blk dS, d L_blk = M dS^T."""
    from dvc_amd import ops
    g = torch.Generator().manual_seed(7)
    Bn, C, Nl, Nm, rows = 2, 66, 200, 150, 70
    L, Mm = torch.randn(Bn, C, Nl, generator=g), torch.randn(Bn, C, Nm, generator=g)
    dS, dM0 = torch.randn(Bn, rows, Nm, generator=g), torch.randn(Bn, C, Nm, generator=g)
    Ld, Md, dSd = L.cuda(), Mm.cuda(), dS.cuda()
    blk, blk64 = Ld[:, :, 64:64 + rows], L[:, :, 64:64 + rows].double()
    S = ops.bgemm(blk.transpose(1, 2), Md)
    _assert_within_bound(S, blk64.transpose(1, 2) @ Mm.double(), blk64.abs().transpose(1, 2) @ Mm.double().abs(), None, C, "slice: scores")
    dM = dM0.cuda()
    ops.bgemm(blk, dSd, out=dM, accumulate=True)
    _assert_within_bound(dM, blk64 @ dS.double(), blk64.abs() @ dS.double().abs(), dM0, rows, "slice: grad_cols")
    dL = torch.full((Bn, C, Nl), float("nan"), device="cuda")
    ops.bgemm(Md, dSd.transpose(1, 2), out=dL[:, :, 64:64 + rows])
    _assert_within_bound(dL[:, :, 64:64 + rows], Mm.double() @ dS.double().transpose(1, 2),
                         Mm.double().abs() @ dS.double().abs().transpose(1, 2), None, Nm, "slice: grad_rows")
    assert torch.isnan(dL[:, :, :64]).all() and torch.isnan(dL[:, :, 64 + rows:]).all()


@pytest.mark.parametrize("orient", ORIENTS)
@pytest.mark.parametrize("M,N,K", [(66, 64, 5184), (130, 257, 66)])
def test_bgemm_image_bits_do_not_depend_on_the_batch(M, N, K, orient):
    """Image 1 of a batch of 3 against the same image alone, bit for bit; (66, 64, 5184) takes the split-K path."""
    from dvc_amd import _lib, ops
    assert (_lib.load().dvc_bgemm_workspace_bytes(3, M, N, K) > 0) == (K == 5184)
    A, B, C0, _, _ = _case(M, N, K, 3)
    acc = orient == "A_B_acc"
    a, b = _operands(A, B, orient)
    whole = ops.bgemm(a, b, out=C0.cuda(), accumulate=acc)
    a1, b1 = _operands(A[1:2], B[1:2], orient)
    alone = ops.bgemm(a1, b1, out=C0[1:2].cuda(), accumulate=acc)
    assert torch.equal(whole[1:2], alone)
    assert torch.equal(ops.bgemm(a[1:2], b[1:2], out=C0[1:2].cuda(), accumulate=acc), alone)     # a batch-1 view of the batch


@pytest.mark.parametrize("orient", ORIENTS)
def test_dvc_bgemm_unsplit_entry_point_at_a_shape_ops_bgemm_splits(orient):
    """dvc_bgemm itself (no workspace, never split; ops.bgemm calls dvc_bgemm_splitk) at (66, 64, 5184), batch 3: one k-ordered
    chain of 5184 products per element — the same bound, the same bits twice and for image 1 alone."""
    from dvc_amd import _lib, ops
    M, N, K = 66, 64, 5184
    A, B, C0, P64, Pabs = _case(M, N, K, 3)
    acc = orient == "A_B_acc"
    a, b = _operands(A, B, orient)
    lib = _lib.load()

    def run(a, b, c0):
        out = c0.cuda()
        rc = lib.dvc_bgemm(ops._p(a), ops._p(b), ops._p(out), a.shape[0], M, N, K, *a.stride(), *b.stride(), M * N, N, int(acc),
                           ops._stream())
        _lib.check(rc, "dvc_bgemm")
        return out
    whole = run(a, b, C0)
    _assert_within_bound(whole, P64, Pabs, C0 if acc else None, K, f"dvc_bgemm {orient} {M}x{N}x{K} unsplit")
    assert torch.equal(run(a, b, C0), whole)
    a1, b1 = _operands(A[1:2], B[1:2], orient)
    assert torch.equal(run(a1, b1, C0[1:2]), whole[1:2])


def test_bgemm_refusals_on_device():
    from dvc_amd import ops
    a, b = torch.zeros(2, 8, 6, device="cuda"), torch.zeros(2, 6, 4, device="cuda")
    with pytest.raises(RuntimeError, match="float32"):
        ops.bgemm(a.double(), b)
    with pytest.raises(RuntimeError, match="float32"):
        ops.bgemm(a[0], b[0])
    with pytest.raises(RuntimeError, match="inner stride"):
        ops.bgemm(torch.zeros(2, 8, 12, device="cuda")[:, :, ::2], b)
    with pytest.raises(RuntimeError, match="do not match"):
        ops.bgemm(a, b[:, :5])
    with pytest.raises(RuntimeError, match="accumulate needs"):
        ops.bgemm(a, b, accumulate=True)
    with pytest.raises(RuntimeError, match="unit inner stride"):
        ops.bgemm(a, b, out=torch.zeros(2, 4, 8, device="cuda").transpose(1, 2))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.bgemm(a, b.cpu())


# ---------------------------------------------------------------------------------------------- through the public callers
@pytest.fixture
def native():
    from dvc_amd import block_products as bp
    assert bp.backend() is None
    with bp.use_backend("native"):
        yield bp
    assert bp.backend() is None


def _count_native_products(monkeypatch):
    from dvc_amd import block_products as bp, ops
    calls = []

    def counted(*a, **kw):
        calls.append(1)
        return ops.bgemm(*a, **kw)
    monkeypatch.setattr(bp._Native, "product", staticmethod(counted))
    return calls


@pytest.mark.parametrize("h,w,B,T,block_bytes", [(12, 20, 2, 0.01, 4 * 64 * 240), (9, 7, 2, 0.05, None)])
def test_native_fused_correlation_over_ragged_row_blocks(h, w, B, T, block_bytes, native, monkeypatch):
    """tests/test_gpu_corr_backward.py's several-row-blocks check (ROW_BLOCK = 64: 240 rows = 3 x 64 + 48, 63 rows one ragged
    block; chunk 1), its oracle and its tolerances, with the three products on the native GEMM."""
    calls = _count_native_products(monkeypatch)
    TC.test_fused_correlation_backward_over_several_row_blocks(h, w, B, T, block_bytes, "native-gemm", monkeypatch)
    assert len(calls) >= 3


@pytest.mark.parametrize("h,w,B,T,scale", [(10, 16, 1, 0.01, 0.5), (12, 20, 2, 0.01, 1e-4)])
def test_native_fused_correlation_with_wta_scale(h, w, B, T, scale, native, monkeypatch):
    calls = _count_native_products(monkeypatch)
    TC.test_fused_correlation_backward_with_wta_scale(h, w, B, T, scale, "native-gemm")
    assert len(calls) >= 3


def test_native_fused_correlation_single_block(native):
    TC.test_fused_correlation_backward_vs_oracle_autograd(12, 20, 2, 0.01, "native-gemm")


@pytest.mark.parametrize("C,H,W,B,h,centre,row_block", [(512, 13, 24, 2, 0.1, True, None), (256, 27, 48, 2, 0.1, True, None),
                                                        (64, 24, 40, 1, 0.2, False, None), (128, 7, 9, 3, 0.1, True, None),
                                                        (64, 9, 14, 3, 0.1, True, 64), (66, 7, 9, 2, 0.1, True, 64)])
def test_native_contextual_losses(C, H, W, B, h, centre, row_block, native, monkeypatch):
    """ContextualLoss and ContextualLoss_forward at the shapes of tests/test_gpu_contextual.py (its checker: float64 autograd,
    its tolerances, run-to-run equality), several and ragged row blocks with ROW_BLOCK = 64, and C = 66, which the engine
    cannot take."""
    from dvc_amd import contextual
    if row_block:
        monkeypatch.setattr(contextual, "ROW_BLOCK", row_block)
    calls = _count_native_products(monkeypatch)
    TX._check_vs_float64_autograd(C, H, W, B, h, centre)
    assert len(calls) >= 2


def test_engine_refuses_c66_and_native_ignores_torchs_tf32_switch(monkeypatch):
    from dvc_amd import block_products as bp, contextual
    from models.ContextualLoss import ContextualLoss
    monkeypatch.setattr(contextual, "ROW_BLOCK", 64)
    X, Y = TX.O.synth_features(1066, 2, 66, 7, 9)
    with bp.use_backend("engine"):
        x = X.cuda().requires_grad_(True)
        with pytest.raises(RuntimeError, match="multiple of 4"):
            ContextualLoss()(x, Y.cuda()).sum().backward()
    assert bp.backend() is None
    before = torch.backends.cuda.matmul.allow_tf32
    torch.backends.cuda.matmul.allow_tf32 = True
    try:
        with bp.use_backend("vendor"):
            with pytest.raises(RuntimeError, match="TF32"):
                ContextualLoss()(X.cuda(), Y.cuda())
        with bp.use_backend("native"):
            loss_tf = ContextualLoss()(X.cuda(), Y.cuda())
    finally:
        torch.backends.cuda.matmul.allow_tf32 = before
    with bp.use_backend("native"):
        assert torch.equal(ContextualLoss()(X.cuda(), Y.cuda()), loss_tf)


def test_vendor_again_after_the_block():
    """The default path before, the native one inside, the default again after: backend() says so and the bits agree."""
    from dvc_amd import block_products as bp, ops
    from dvc_amd.corr_autograd import fused_correlation
    th, ph, lab, gy, gs = TC._inputs(2, 9, 7, 907)
    blab = ops.avgpool4x4(lab.cuda()).view(2, 3, -1)

    def grads():
        t, p = th.cuda().requires_grad_(True), ph.cuda().requires_grad_(True)
        y, sim, _ = fused_correlation(t, p, blab, 0.05, 9, 7)
        ((y * gy.cuda()).sum() + (sim * gs.cuda()).sum()).backward()
        return t.grad, p.grad
    assert bp.backend() is None
    before = grads()
    with bp.use_backend("native"):
        assert bp.backend() == "native"
        inside = grads()
    assert bp.backend() is None
    after = grads()
    assert torch.equal(before[0], after[0]) and torch.equal(before[1], after[1])
    for i, r in zip(inside, before):       # each is within 2e-3 of the truth's scale (tests/test_gpu_corr_backward.py)
        assert (i - r).abs().max().item() <= 4e-3 * r.abs().max().item()
