"""GPU: every bandwidth-bound kernel between the GEMMs of the contextual losses and of the fused correlation's backward, ALONE,
through the C ABI, against its float64 restatement (tests/cx_kernels_reference.py, pinned by tests/test_cx_kernels_host.py):

    dvc_cx_rows, dvc_cx_colmax, dvc_cx_finish, dvc_cx_rows_tq, dvc_cx_ds      csrc/contextual.hip
    dvc_cx_normalize_bwd                                                      csrc/feature_norm.hip
    dvc_corr_softmax_bwd (row statistics + dS)                                csrc/corr_bwd.hip

The end-to-end tests (test_gpu_contextual.py, test_gpu_corr_backward.py) see these kernels through one scalar loss and through
max |dX - dX64| against the single largest gradient; here every output element has its own bound, derived from the kernel's
arithmetic (formulas: the docstrings of cx_kernels_reference.py and of the tests below; u = 2^-24), integer outputs are compared
exactly, and every output starts as NaN (integers: -1) so that an element the launch left alone shows.

Inputs: S = the float32 rounding of Xn^T Yn for oracle.contextual_oracle.synth_features cut to Nx x Ny positions (CASES), and
constructed blocks for exact ties and degenerate rows.  The row statistics a kernel READS are the float64 reference's rounded to
float32, so that an error of dvc_cx_rows cannot cancel in a later kernel.  CASES covers Nx != Ny; N = 1, 63, 126, 129, 256, 257,
312, 1025; rows = 1, 3 and every tail of cx_colmax_kernel's 64-row unrolled loop (rows mod 64 = 0, 1, 17, 33, 49, and 6, 22, 56);
batches of 1 and 3; dense and padded strides (S_bs = ld * N with ld = rows rounded up to 64, plus 64; row_bs = rows + 7;
tq_bs = rows + 3).

Every test prints its worst error / bound ratio and asserts it is at most 1.  Measured on an MI355X (worst over the cases):
    dvc_cx_rows            a 0.36 (of 2 ulp), l 0.31, r 0.13, e 0.08; ties: jstar exact, l 0.22; max S = 1: l 0.09
    dvc_cx_colmax          cmax 0.43; smallest top-two column gap of the reference 2.0e-4 (N1025); ties 0.34
    dvc_cx_rows_tq         T 0.31, Q 0.28
    dvc_cx_finish          loss 0.24, gscale 0.23 (of 2 ulp)
    dvc_cx_ds              mode 0: 0.58 (arg-max columns 0.38), mode 1: 0.59 (arg-max columns 0.54)
    dvc_cx_normalize_bwd   0.46
    dvc_corr_softmax_bwd   0.77 at T = 0.01, 0.53 at T = 0.05, 0.04 at T = 1e-7; row sums 0.28
The same steps in float32 on the CPU give the same ratios to two digits (0.77 for the correlation at T = 0.01): the bounds are
first-order worst cases and the arithmetic uses about half of them.
"""
import functools
from types import SimpleNamespace

import pytest
import torch

import cx_kernels_reference as R
from cabi_helpers import check, lib, nan_tensor, ops, ptr  # noqa: F401  (ops, lib: fixtures)
from test_gpu_contextual import gemm_mode  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu

# name: (C, Nx, Ny, h, B, padded strides, centre)
CASES = {
    "c64_150x126_h01": (64, 150, 126, 0.1, 3, False, True),
    "c64_150x126_h02": (64, 150, 126, 0.2, 1, True, True),
    "c8_3x63": (8, 3, 63, 0.1, 3, True, True),
    "c128_65x256": (128, 65, 256, 0.1, 1, False, True),
    "c512_312x312": (512, 312, 312, 0.1, 1, True, True),
    "c16_70x129_h05": (16, 70, 129, 0.5, 3, False, True),
    "N1": (8, 5, 1, 0.1, 3, True, False),            # (one exemplar position: centring would zero it)
    "N257": (16, 33, 257, 0.1, 1, False, True),
    "N1025": (16, 17, 1025, 0.1, 3, True, True),
    "rows1": (16, 1, 70, 0.1, 3, False, True),
    "rows49": (16, 49, 70, 0.1, 1, True, True),
    "rows64": (16, 64, 40, 0.1, 3, True, True),
}
SEED = 2                # of seeds 1 .. 8 the one whose smallest top-two column gap (the float64 reference's) is largest: 2.0e-4
GOUT = 0.75
FAKE_ROW0 = 192         # a block that is the whole of S, placed at this global row (the column arg-max shifted with it)


def _h32(h):
    return float(torch.tensor(h, dtype=torch.float32))


def _f32(t):
    return t.float()


def _ints(*shape, fill=-1):
    return torch.full(shape, fill, device="cuda", dtype=torch.int32)


def _ld(rows, padded):
    return (rows + 63) // 64 * 64 + 64 if padded else rows


def _block(S, ld):
    """S [B, rows, N] (CPU float32) in a NaN-filled device buffer [B, ld, N]."""
    buf = nan_tensor(S.shape[0], ld, S.shape[2])
    buf[:, :S.shape[1]] = S.cuda()
    return buf


def _rowbuf(x, row_bs, dtype=torch.float32):
    """x [B, rows] in a device buffer [B, row_bs] (NaN / -1 behind the rows)."""
    buf = nan_tensor(x.shape[0], row_bs) if dtype == torch.float32 else _ints(x.shape[0], row_bs)
    buf[:, :x.shape[1]] = x.to(dtype).cuda()
    return buf


def _worst(got, ref, bound):
    return ((got.double().cpu() - ref).abs() / bound).max().item()


def _stats(S, h32):
    """The float64 reference of every forward piece for S [B, Nx, N], and the float32 roundings the later kernels are fed."""
    c = SimpleNamespace(S=S, h32=h32, B=S.shape[0], Nx=S.shape[1], N=S.shape[2])
    c.a, c.jstar, c.l, c.r, c.e = R.rows_stats(S, h32)
    c.a32, c.l32, c.r32, c.e32 = (_f32(t) for t in (c.a, c.l, c.r, c.e))
    # what dvc_cx_colmax / rows_tq compute from the float32 a and l they are GIVEN
    c.cmax, c.cargi = R.col_max(S, c.a32, c.l32, h32)
    return c


@functools.lru_cache(maxsize=None)
def _case(name):
    C, Nx, Ny, h, B, padded, centre = CASES[name]
    c = _stats(R.scores(SEED, B, C, Nx, Ny, centre), _h32(h))
    c.padded, c.h = padded, h
    return c


@functools.lru_cache(maxsize=None)
def _ds_ref(name, mode):
    c = _case(name)
    return R.ds(c.S, c.h32, mode, GOUT)


# ------------------------------------------------------------------------------------------------ dvc_cx_rows
def _run_rows(lib, ops, S, h, ld, row_bs):
    B, rows, N = S.shape
    Sd = _block(S, ld)
    a, l, r, e = (nan_tensor(B, row_bs) for _ in range(4))
    js = _ints(B, row_bs)
    check(lib.dvc_cx_rows(ptr(Sd), B, ld * N, row_bs, rows, N, h, ptr(a), ptr(js), ptr(l), ptr(r), ptr(e), ops._stream()), "dvc_cx_rows")
    torch.cuda.synchronize()
    for t in (a, l, r, e):
        assert torch.isnan(t[:, rows:]).all() and not torch.isnan(t[:, :rows]).any()
    assert (js[:, rows:] == -1).all()
    return [t[:, :rows].cpu() for t in (a, js, l, r, e)]


def _assert_rows(tag, got, S, h32):
    a, js, l, r, e = got
    ra, rj, rl, rr, re = R.rows_stats(S, h32)
    dl, dr, de = R.rows_bounds(S, h32)
    assert torch.equal(js.long(), rj), f"{tag}: jstar differs in rows {(js.long() != rj).nonzero().tolist()[:8]}"
    ratios = dict(a=_worst(a, ra, 2 * R.ulp32(ra)), l=_worst(l, rl, dl), r=_worst(r, rr, dr), e=_worst(e, re, de))
    print(f"cx_rows {tag}: worst error / bound " + ", ".join(f"{k} {v:.3f}" for k, v in ratios.items()))
    assert max(ratios.values()) <= 1.0, ratios


@pytest.mark.parametrize("name", list(CASES))
def test_cx_rows(lib, ops, name):
    """jstar exactly the lowest index of the float32 row maximum; a within 2 ulp (1 - m, the float32 constant 1e-5f, the sum);
    l, r, e within cx_kernels_reference.rows_bounds:
        dz <= u (3 q + 2 |1 - q| + 1) / h,  dw <= w (dz + 4 u) + 2^-126,  dl <= sum_j dw + (ceil(N / 256) + 10) u l,
        dr <= r (dw* / w* + dl / l + u),  de <= [sum_j d (dw + u w) + (ceil(N / 256) + 10) u sum_j w d] / l + e (dl / l + u)."""
    c = _case(name)
    got = _run_rows(lib, ops, c.S, c.h, _ld(c.Nx, c.padded), c.Nx + 7 if c.padded else c.Nx)
    _assert_rows(name, got, c.S, c.h32)


def _tie_rows():
    """Six rows of 600 columns, background in (-0.5, 0.5), the row maximum 0.75 at several columns.  Thread t of the 256 reads
    columns t, t + 256, t + 512; wave = (column mod 256) / 64."""
    g = torch.Generator().manual_seed(9)
    S = torch.rand(1, 6, 600, generator=g) - 0.5
    sets = [(5, 261),                       # one thread's stride
            (70, 200),                      # waves 1 and 3
            (300, 10),                      # across the 256-column wrap: lanes 44 and 10 of wave 0
            (517, 3, 259, 130, 64),         # five: threads 5, 3, 3 and waves 2, 1
            (40, 33, 50, 63, 35),           # five lanes of one wave: the butterfly alone decides
            (21, 20)]                       # neighbouring lanes
    for i, cols in enumerate(sets):
        S[0, i, list(cols)] = 0.75
    return S, torch.tensor([min(s) for s in sets])


def test_cx_rows_ties(lib, ops):
    """The row maximum at two and at five columns — in one thread's stride, across lanes, across waves and across the 256-column
    wrap: jstar is the lowest column; a, l, r, e within the bounds of test_cx_rows (the values do not depend on the choice)."""
    S, lowest = _tie_rows()
    got = _run_rows(lib, ops, S, 0.1, 6, 6)
    assert torch.equal(got[1][0].long(), lowest), (got[1][0].tolist(), lowest.tolist())
    _assert_rows("ties", got, S, _h32(0.1))


def test_cx_rows_maximum_one(lib, ops):
    """A row whose maximum is exactly 1: a = 1e-5f, every other weight underflows (d >= 0.1: z <= -1e5), so l = w* = exp(1 / h),
    r = 1 and e = 0 exactly (e accumulates w * 0 and zeros)."""
    g = torch.Generator().manual_seed(10)
    S = torch.rand(2, 3, 130, generator=g) * 1.4 - 0.5
    S[:, 1, 77] = 1.0
    got = _run_rows(lib, ops, S, 0.1, 3, 3)
    a, js, l, r, e = got
    assert (a[:, 1] == torch.tensor(1e-5, dtype=torch.float32)).all() and (js[:, 1] == 77).all()
    assert (r[:, 1] == 1.0).all() and (e[:, 1] == 0.0).all()
    _assert_rows("max S = 1", got, S, _h32(0.1))


# ------------------------------------------------------------------------------------------------ dvc_cx_colmax
def _run_colmax(lib, ops, c, Sd, ld, row_bs, a, l, blocks):
    """dvc_cx_colmax over `blocks` = [(row0, rows), ...] of the device block Sd [B, ld, N] on one pair of running buffers that
    starts in the initial state of dvc_amd.contextual (cmax = -1, cargi = 0)."""
    cmax, cargi = torch.full((c.B, c.N), -1.0, device="cuda"), torch.zeros((c.B, c.N), device="cuda", dtype=torch.int32)
    for row0, rows in blocks:
        check(lib.dvc_cx_colmax(ptr(Sd[:, row0:]), c.B, ld * c.N, row_bs, ptr(a[:, row0:]), ptr(l[:, row0:]), rows, c.N, row0, c.h,
                                ptr(cmax), ptr(cargi), ops._stream()), "dvc_cx_colmax")
    torch.cuda.synchronize()
    return cmax.cpu(), cargi.cpu()


def _blocks64(Nx):
    return [(i0, min(64, Nx - i0)) for i0 in range(0, Nx, 64)]


def _gap(A):
    """Relative gap between the largest and the second largest value of every column of A [B, rows, N] (inf for one row)."""
    if A.shape[1] == 1:
        return torch.full(A.shape[::2], float("inf"), dtype=torch.float64)
    top = A.topk(2, dim=1)[0]
    return (top[:, 0] - top[:, 1]) / top[:, 0]


def _colmax_both_ways(lib, ops, c):
    ld, row_bs = _ld(c.Nx, c.padded), c.Nx + 7 if c.padded else c.Nx
    Sd, a, l = _block(c.S, ld), _rowbuf(c.a32, row_bs), _rowbuf(c.l32, row_bs)
    one = _run_colmax(lib, ops, c, Sd, ld, row_bs, a, l, [(0, c.Nx)])
    if c.Nx > 64:
        many = _run_colmax(lib, ops, c, Sd, ld, row_bs, a, l, _blocks64(c.Nx))
        assert torch.equal(one[0], many[0]) and torch.equal(one[1], many[1]), "one call and the chain of 64-row blocks differ"
    assert (one[0] > 0).all(), "a column kept the initial state"
    return one


@pytest.mark.parametrize("name", list(CASES))
def test_cx_colmax(lib, ops, name):
    """One call over all rows, and (Nx > 64) the chain of calls over 64-row blocks with a ragged last one on the same running
    buffers: bit-identical.  cargi exactly the reference's — first asserting that the reference's top two values of every column
    are at least 1e-4 apart, relative, against an affinity bound of some 1e-6 — and cmax within
        dA <= A (dz + 6 u) + 2^-126,  dz <= u (3 q + 2 |1 - q| + 1) / h        (A from the float32 a and l the kernel is given)."""
    c = _case(name)
    cmax, cargi = _colmax_both_ways(lib, ops, c)
    if c.N == 1:            # A = w / l is 1 up to rounding in EVERY row: no row is the maximum by more than that; the value is checked
        gap = float("inf")
        assert ((cargi >= 0) & (cargi < c.Nx)).all()
    else:
        gap = _gap(R.affinity(c.S, c.a32, c.l32, c.h32)).min().item()
        assert gap >= 1e-4, gap
        assert torch.equal(cargi.long(), c.cargi)
    dA = R.A_bound(c.S, c.a32, c.l32, c.h32)
    dA = dA.max(1)[0] if c.N == 1 else dA.gather(1, c.cargi.unsqueeze(1)).squeeze(1)
    ratio = _worst(cmax, c.cmax, dA)
    print(f"cx_colmax {name}: smallest top-two gap {gap:.2e}, worst error / bound {ratio:.3f}")
    assert ratio <= 1.0


@pytest.mark.parametrize("where,copies", [("inside", (5, 37, 42)), ("across", (5, 69, 130))])
def test_cx_colmax_ties(lib, ops, where, copies):
    """The row that wins the most columns, copied into three rows of S (their a, l and A are then bit-identical: exact ties in
    every column).  inside: rows 5 and 37 belong to one row group of the kernel, 42 to another — the serial scan and the LDS
    combine; across: rows 5, 69 and 130 sit in three 64-row blocks — the carried-in maximum.  The lowest copy wins every column
    the three win, in one call and in the chain of blocks, and the other columns keep the reference's row."""
    base = _case("c64_150x126_h01")
    S, higher = base.S.clone(), []
    for b in range(base.B):
        wins = torch.bincount(base.cargi[b], minlength=base.Nx)
        wins[:copies[0] + 1] = 0              # (a source above the lowest copy: the source row itself is a fourth, higher copy)
        src = wins.argmax().item()
        row = S[b, src].clone()
        for i in copies:
            S[b, i] = row
        higher.append(sorted({src, *copies})[1:])
    c = _stats(S, base.h32)
    c.padded, c.h = True, base.h
    cmax, cargi = _colmax_both_ways(lib, ops, c)
    A = R.affinity(c.S, c.a32, c.l32, c.h32)
    for b in range(c.B):
        assert not torch.isin(cargi[b], torch.tensor(higher[b], dtype=torch.int32)).any(), "a higher copy of the tied rows won a column"
        assert (cargi[b] == copies[0]).sum().item() >= 2
        keep = torch.ones(c.Nx, dtype=torch.bool)
        keep[higher[b]] = False
        safe = _gap(A[b:b + 1, keep])[0] >= 1e-4
        assert safe.float().mean().item() > 0.9
        assert torch.equal(cargi[b].long()[safe], c.cargi[b][safe])
    dA = R.A_bound(c.S, c.a32, c.l32, c.h32).gather(1, c.cargi.unsqueeze(1)).squeeze(1)
    ratio = _worst(cmax, c.cmax, dA)
    print(f"cx_colmax ties {where}: worst error / bound {ratio:.3f}")
    assert ratio <= 1.0


# ------------------------------------------------------------------------------------------------ dvc_cx_rows_tq
def _run_tq(lib, ops, c, cargi, row0):
    ld, row_bs, tq_bs = _ld(c.Nx, c.padded), c.Nx + 7 if c.padded else c.Nx, c.Nx + 3 if c.padded else c.Nx
    Sd, a, l = _block(c.S, ld), _rowbuf(c.a32, row_bs), _rowbuf(c.l32, row_bs)
    t, q = nan_tensor(c.B, tq_bs), nan_tensor(c.B, tq_bs)
    cg = cargi.to(torch.int32).cuda().contiguous()
    check(lib.dvc_cx_rows_tq(ptr(Sd), c.B, ld * c.N, row_bs, tq_bs, ptr(a), ptr(l), ptr(cg), c.Nx, c.N, row0, c.h, ptr(t), ptr(q),
                             ops._stream()), "dvc_cx_rows_tq")
    torch.cuda.synchronize()
    assert torch.isnan(t[:, c.Nx:]).all() and torch.isnan(q[:, c.Nx:]).all()
    return t[:, :c.Nx].cpu(), q[:, :c.Nx].cpu()


def _assert_tq(tag, c, cargi, row0, t, q):
    rt, rq = R.rows_tq(c.S, c.a32, c.l32, cargi, row0, c.h32)
    dt, dq = R.tq_bounds(c.S, c.a32, c.l32, cargi, row0, c.h32)
    none = rt == 0
    assert (t[none] == 0).all() and (q[none] == 0).all(), "a row that owns no column must give exact zeros"
    ratios = (_worst(t, rt, dt + R.TINY), _worst(q, rq, dq + R.TINY))
    print(f"cx_rows_tq {tag}: {int(none.sum())} of {none.numel()} rows own nothing; worst error / bound T {ratios[0]:.3f}, Q {ratios[1]:.3f}")
    assert max(ratios) <= 1.0


@pytest.mark.parametrize("name", list(CASES))
def test_cx_rows_tq(lib, ops, name):
    """The block placed at global row 192 (row0 != 0; the reference's column arg-max shifted with it).  Rows that own no column
    give exact zeros; the others are within
        dT <= sum_owned dA + (ceil(N / 256) + 10) u T,   dQ <= sum_owned d (dA + u A) + (ceil(N / 256) + 10) u Q."""
    c = _case(name)
    cargi = c.cargi + FAKE_ROW0
    t, q = _run_tq(lib, ops, c, cargi, FAKE_ROW0)
    _assert_tq(name, c, cargi, FAKE_ROW0, t, q)


def test_cx_rows_tq_one_row_owns_every_column(lib, ops):
    """cargi = row0 + 2 everywhere: T_2 = sum_j A_2j (~ 1), Q_2 = E_2, every other row exactly 0; same bounds."""
    c = _case("c8_3x63")
    cargi = torch.full((c.B, c.N), FAKE_ROW0 + 2, dtype=torch.long)
    t, q = _run_tq(lib, ops, c, cargi, FAKE_ROW0)
    assert (t[:, :2] == 0).all() and (q[:, :2] == 0).all() and (t[:, 2] > 0.99).all()
    _assert_tq("row 2 owns all", c, cargi, FAKE_ROW0, t, q)


# ------------------------------------------------------------------------------------------------ dvc_cx_finish
@pytest.mark.parametrize("n", [1, 255, 256, 1297])
def test_cx_finish(lib, ops, n):
    """loss = -log mean(v), gscale = -1 / (n mean(v)) for three images: the kernel accumulates and finishes in double and rounds
    once, so both are within 2 ulp of the float64 values (1/2 ulp of the cast, the rest for the double-precision log)."""
    v = torch.rand(3, n, generator=torch.Generator().manual_seed(n)) * 0.99 + 0.01
    loss, gs, vd = nan_tensor(3), nan_tensor(3), v.cuda()
    check(lib.dvc_cx_finish(ptr(vd), 3, n, ptr(loss), ptr(gs), ops._stream()), "dvc_cx_finish")
    torch.cuda.synchronize()
    rl, rg = R.finish(v)
    ratios = (_worst(loss, rl, 2 * R.ulp32(rl) + R.TINY), _worst(gs, rg, 2 * R.ulp32(rg)))
    print(f"cx_finish n={n}: worst error / (2 ulp) loss {ratios[0]:.3f}, gscale {ratios[1]:.3f}")
    assert max(ratios) <= 1.0


# ------------------------------------------------------------------------------------------------ dvc_cx_ds
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("name", list(CASES))
def test_cx_ds(lib, ops, name, mode):
    """dS of a block of rows against float64 autograd of the restated loss (cx_kernels_reference.ds), gout = 0.75.  Nx > 64: the
    block is rows 64 .. Nx - 1 of the image (row0 = 64); else the whole image placed at global row 192.  Fed: the float64
    reference's a, l, r, e, T, Q, gscale rounded to float32, its jstar and cargi.  ld_t = rows rounded up to 32, plus 32.
    Three launches: dS and dST, dS only, dST only.  dS rows >= rows and the bytes behind dST stay NaN, dST[j][i >= rows] is
    exactly 0, dST is the bit-equal transpose of dS, and the three launches agree bit for bit.  Per element
    (cx_kernels_reference.ds_bound), with g = gscale * gout, delta the 0 / 1 indicator, dA <= A (dz + 6 u) + 2^-126:
      mode 0: d(dz) <= |g| r (dA + 6 u |delta - A|),                      d(sdd) <= |g| r (3 u a + u E + 6 u |dmin - E|)
      mode 1: d(dz) <= |g| (dA |delta - T| + A (5 u |delta - T| + u T)),  d(sdd) <= |g| (u Q + 3 u T E + 4 u |Q - T E|)
      d(dS) <= (d(dz) + 3 u |dz|) / (h a) + [k = j*] (d(sdd) + 5 u |sdd|) / (h a^2) + u |dS| + 2^-126."""
    c = _case(name)
    N, B = c.N, c.B
    lo, row0 = (64, 64) if c.Nx > 64 else (0, FAKE_ROW0)
    rows = c.Nx - lo
    sl = slice(lo, c.Nx)
    ref = _ds_ref(name, mode)[:, sl]
    # the float64 pieces of the autograd's own evaluation: cargi from the float64 a and l
    cmax64, cargi64 = R.col_max(c.S, c.a, c.l, c.h32)
    v = c.r if mode == 0 else cmax64
    g64 = R.finish(v)[1]
    cargi = cargi64 + (row0 - lo)
    S = c.S[:, sl].contiguous()
    a, l, r, e, js = c.a[:, sl], c.l[:, sl], c.r[:, sl], c.e[:, sl], c.jstar[:, sl]
    T, Q = R.rows_tq(S, a, l, cargi, row0, c.h32)
    bound = R.ds_bound(S, c.h32, mode, g64 * GOUT, _f32(a).double(), js, _f32(l).double(), _f32(r).double(), _f32(e).double(),
                       cargi, _f32(T).double(), _f32(Q).double(), row0)
    ld, row_bs, tq_bs = _ld(rows, c.padded), rows + 7 if c.padded else rows, rows + 3 if c.padded else rows
    ld_t = (rows + 31) // 32 * 32 + 32
    guard = 256
    Sd = _block(S, ld)
    ad, ldv, rd, ed = (_rowbuf(_f32(t), row_bs) for t in (a, l, r, e))
    jd = _rowbuf(js, row_bs, torch.int32)
    cg = cargi.to(torch.int32).cuda().contiguous()
    td, qd = _rowbuf(_f32(T), tq_bs), _rowbuf(_f32(Q), tq_bs)
    gs = _f32(g64).cuda().contiguous()

    def run(want_ds, want_dst):
        dS = nan_tensor(B, ld, N) if want_ds else None
        dST = nan_tensor(B * N * ld_t + guard) if want_dst else None
        check(lib.dvc_cx_ds(ptr(Sd), B, ld * N, row_bs, tq_bs, ptr(ad), ptr(ldv), ptr(rd), ptr(ed), ptr(jd), ptr(cg) if mode else None,
                            ptr(td) if mode else None, ptr(qd) if mode else None, ptr(gs), GOUT, mode, rows, N, row0, ld_t, c.h,
                            ptr(dS), ptr(dST), ops._stream()), "dvc_cx_ds")
        torch.cuda.synchronize()
        if want_ds:
            assert torch.isnan(dS[:, rows:]).all(), "dS was written behind the block's rows"
        if want_dst:
            assert torch.isnan(dST[B * N * ld_t:]).all(), "dST was written behind its last row"
            dST = dST[:B * N * ld_t].view(B, N, ld_t)
            assert (dST[:, :, rows:] == 0).all(), "dST[j][i >= rows] must be zeros"
        return dS, dST
    dS, dST = run(True, True)
    assert not torch.isnan(dS[:, :rows]).any()
    assert torch.equal(dST[:, :, :rows], dS[:, :rows].transpose(1, 2)), "dST is not the transpose of dS"
    only_ds, _ = run(True, False)
    _, only_dst = run(False, True)
    assert torch.equal(only_ds[:, :rows], dS[:, :rows]) and torch.equal(only_dst, dST)
    err = (dS[:, :rows].double().cpu() - ref).abs() / bound
    ratio = err.max().item()
    star = R.onehot(js, N)
    print(f"cx_ds {name} mode {mode}: rows {rows} at row0 {row0}, ld_t {ld_t}; worst error / bound {ratio:.3f} "
          f"(arg-max columns {err[star].max().item():.3f}, others {err[~star].max().item() if N > 1 else 0.0:.3f})")
    assert ratio <= 1.0


# ------------------------------------------------------------------------------------------------ dvc_cx_normalize_bwd
@pytest.mark.parametrize("P", [1, 63, 100])
@pytest.mark.parametrize("C", [3, 8, 66, 130])
def test_cx_normalize_bwd(lib, ops, C, P):
    """Batch 2; position 0 of image 0 has norm = 0 and xn = 0: the n > 0 guard alone keeps 0 * (0 / 0) out, the result there is
    dxn / eps — exactly, eps = 2^-52 being a power of two.  Elsewhere, against the float64 evaluation from the same float32 xn,
    norm and dxn (cx_kernels_reference.normalize_bwd_bound; the dot product with ceil(C / 16) + 16 roundings as in
    test_cx_prepare_edges):   d(dx) <= 3 u |dxn| / (n + eps) + |xn| (d(dot) / n + 2 u |k|) + u |dx| + 2^-126."""
    B = 2
    g = torch.Generator().manual_seed(100 * C + P)
    x = torch.randn(B, C, P, generator=g, dtype=torch.float64)
    x[0, :, 0] = 0
    n = x.norm(dim=1)
    eps = float(ops.EPS64)
    assert eps == 2.0 ** -52
    xn, norm, dxn = (x / (n.unsqueeze(1) + eps)).float(), n.float(), torch.randn(B, C, P, generator=g)
    dx = nan_tensor(B, C, P)
    xd, nd, dd = xn.cuda(), norm.cuda(), dxn.cuda()             # (held: a temporary's memory would be handed to the next one)
    check(lib.dvc_cx_normalize_bwd(ptr(xd), ptr(nd), ptr(dd), B, C, P, eps, ptr(dx), ops._stream()), "dvc_cx_normalize_bwd")
    torch.cuda.synchronize()
    dx = dx.cpu()
    assert torch.isfinite(dx).all()
    assert torch.equal(dx[0, :, 0], (dxn[0, :, 0].double() * 2.0 ** 52).float())
    ratio = _worst(dx, R.normalize_bwd(xn, norm, dxn, eps), R.normalize_bwd_bound(xn, norm, dxn, eps))
    print(f"cx_normalize_bwd C={C} P={P}: worst error / bound {ratio:.3f}")
    assert ratio <= 1.0


# ------------------------------------------------------------------------------------------------ dvc_corr_softmax_bwd
def _corr_inputs(rows, P, wta, seed):
    """Cosine affinities of clustered unit vectors (rows have a few strong matches), B = 2; wta != 1: row 0 of every image has its
    raw maximum at two columns."""
    B = 2
    g = torch.Generator().manual_seed(seed)
    base = torch.randn(B, 64, 6, generator=g)
    th = torch.randn(B, 64, rows, generator=g) + 2.0 * base[:, :, torch.randint(0, 6, (rows,), generator=g)]
    ph = torch.randn(B, 64, P, generator=g) + 2.0 * base[:, :, torch.randint(0, 6, (P,), generator=g)]
    th, ph = th / th.norm(dim=1, keepdim=True), ph / ph.norm(dim=1, keepdim=True)
    f = torch.einsum("bci,bcj->bij", th, ph).contiguous()
    if wta != 1.0 and P >= 2:
        f[:, 0, P - 1] = f[:, 0, P // 3] = f[:, 0].max(-1)[0] + 0.03125
    blab = torch.randn(B, 3, P, generator=g) * 30
    return f, blab, torch.randn(B, 3, rows, generator=g), torch.randn(B, rows, generator=g)


@pytest.mark.parametrize("wta", [1.0, 0.5])
@pytest.mark.parametrize("rows,P,T", [(70, 63, 0.05), (70, 63, 0.01), (64, 257, 0.05), (64, 257, 0.01), (1, 1, 0.05), (1, 1, 0.01),
                                      (8, 65, 1e-7)])
def test_corr_softmax_bwd(lib, ops, rows, P, T, wta):
    """Batch 2 in buffers laid out for ld_t = 96 with chan_stride = rows + 5, once with gsim / argmax and once without.  The
    reference (cx_kernels_reference.softmax_bwd) forms f' / T in float32 as the kernel does — the same bits, so that T = 1e-7
    compares one problem — and goes on in float64.  Per element
        d(exp) <= ex (u |z - m| + 2 u) + 2^-126,  dl <= sum_j d(exp) + (ceil(P / 256) + 10) u l,  ep = u |z - m| + 3 u + dl / l
        dc <= 3 u (sum_k |g_k B_kj| + sum_k |g_k y_ki|) + u |c|,   c = g . B_j - g . y_i
        d(dS) <= [p (dc + |c| (ep + 2 u)) + 2^-126 |c| / l] / T   (* 1e-4 + 2 u |dS| off the raw maximum when wta != 1;
                                                                    + u |dS| where gsim lands) + 2^-126.
    Every row is finite and sums to the reference's row total within the sum of its bounds; dS rows >= rows stay NaN; dST is the
    bit-equal transpose with zeros in columns rows .. ld_t - 1."""
    B, ld_t, cs = 2, 96, rows + 5
    f, blab, gy, gsim = _corr_inputs(rows, P, wta, 7 * rows + P)
    y = R.softmax_fwd_y(f, blab, T, wta).float()
    am = R.lowest_argmax(f.double(), -1)
    if wta != 1.0 and P >= 2:
        assert (am[:, 0] == P // 3).all()
    fd = nan_tensor(B, ld_t, P)
    fd[:, :rows] = f.cuda()

    def chan(t):            # [B, k, rows] -> device [B, k, cs]
        buf = nan_tensor(B, t.shape[1], cs)
        buf[:, :, :rows] = t.cuda()
        return buf
    gyd, yd, gsd = chan(gy), chan(y), chan(gsim.unsqueeze(1))
    amd = _ints(B, cs)
    amd[:, :rows] = am.to(torch.int32).cuda()
    bd = blab.cuda().contiguous()
    for with_sim in (True, False):
        scratch = nan_tensor(B * 3 * ld_t)
        dS, dST = nan_tensor(B, ld_t, P), nan_tensor(B, P, ld_t)
        check(lib.dvc_corr_softmax_bwd(ptr(fd), ptr(bd), ptr(gyd), ptr(yd), None, ptr(gsd) if with_sim else None,
                                       ptr(amd) if with_sim else None, T, wta, B, rows, P, cs, ld_t, ptr(scratch), ptr(dS), ptr(dST),
                                       ops._stream()), "dvc_corr_softmax_bwd")
        torch.cuda.synchronize()
        assert torch.isnan(dS[:, rows:]).all() and torch.isfinite(dS[:, :rows]).all()
        assert torch.equal(dST[:, :, :rows], dS[:, :rows].transpose(1, 2)) and (dST[:, :, rows:] == 0).all()
        ref, bound = R.softmax_bwd(f, blab, gy, y, gsim if with_sim else None, am, T, wta, with_bound=True)
        got = dS[:, :rows].double().cpu()
        ratio = ((got - ref).abs() / bound).max().item()
        sums = ((got.sum(-1) - ref.sum(-1)).abs() / bound.sum(-1)).max().item()
        print(f"corr_softmax_bwd {rows}x{P} T={T} wta={wta} gsim={with_sim}: worst error / bound {ratio:.3f}, row sums {sums:.3f}")
        assert ratio <= 1.0 and sums <= 1.0


# ------------------------------------------------------------------------------------------------ the modules, Nx != Ny
def test_contextual_modules_unequal_sizes(gemm_mode):
    """X 10 x 15 against Y 9 x 14 (C = 64, B = 2): both losses and dX against float64 autograd through the oracle, at the
    tolerances of test_gpu_contextual.py."""
    from models.ContextualLoss import ContextualLoss, ContextualLoss_forward
    from oracle import contextual_oracle as O
    X, Y = O.synth_features(21, 2, 64, 10, 15)
    Y = Y[:, :, :9, :14].contiguous()           # (X stays a noisy mixture of Y's columns, some of them cut away)
    gout = torch.tensor([0.5, 1.5])
    for tag, mod, fn in (("fwd", ContextualLoss_forward(), O.contextual_loss_forward), ("bwd", ContextualLoss(), O.contextual_loss)):
        x64 = X.double().requires_grad_(True)
        l64 = fn(x64, Y.double(), h=0.1)
        (l64 * gout.double()).sum().backward()
        x = X.cuda().requires_grad_(True)
        loss = mod(x, Y.cuda(), h=0.1)
        (loss * gout.cuda()).sum().backward()
        torch.cuda.synchronize()
        el = (loss.detach().cpu().double() - l64.detach()).abs().max().item()
        scale = x64.grad.abs().max().item()
        eg = (x.grad.cpu().double() - x64.grad).abs().max().item()
        print(f"contextual {tag} 10x15 against 9x14 ({gemm_mode}): loss {l64.tolist()} err {el:.2e}; dX max err {eg:.2e} (max |dX| {scale:.2e})")
        assert x.grad.shape == X.shape
        assert el < 2e-6 * max(1.0, l64.abs().max().item()), (tag, el)
        assert eg <= 5e-5 * scale, (tag, eg, scale)
