"""CPU: the host side of the bf16x3 split GEMM (csrc/bgemm_split3.hip) — header / ctypes table / export agreement, its refusals
(every one before any launch), the `engine` keyword of ops.bgemm and the "split3" backend of dvc_amd.block_products; and the
arithmetic of the split, on the numpy restatement tests/bgemm_split3_reference.py: exactness of the three terms, the size of
what the kernel drops, and exactness of the integer and one-hot cases the GPU file runs on the kernel.

What is dropped must stay below U / 4 |a||b| per product (U = 2^-24), on split_inputs() (10^6 random values and the edge
values, each paired with the value 499 979 places on).  A term of 8 significant bits leaves a residual of up to half its last
place, so |x2| <= 2^-8 |x| and |x3| <= 2^-16 |x|, both reached just above a power of two.  Dropping a2 b3, a3 b2 and a3 b3
together misses the budget: they reach 2 U in the worst case and measure 0.845 U at the largest on these inputs (0.089 U
root mean square) — which is why the kernel computes a2 b3 and a3 b2 and drops a3 b3 alone, at most 2^-32 |a||b| = U / 256."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import bgemm_split3_reference as R
from cabi_common import _fails, _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ONE, TWO, THREE = ctypes.c_void_p(256), ctypes.c_void_p(1024), ctypes.c_void_p(4096)   # never dereferenced: validation fails first
NEW = ["dvc_bgemm_split3", "dvc_bgemm_split3_workspace_bytes"]
SHIFT = 499979


def test_new_entry_points_in_header_table_and_exports():
    from dvc_amd import _lib as binding
    hdr = open(os.path.join(ROOT, "include", "dvc_hip.h")).read()
    out = subprocess.run(["nm", "-D", "--defined-only", binding.LIB_PATH], capture_output=True, text=True).stdout
    exports = open(os.path.join(os.path.dirname(os.path.dirname(binding.LIB_PATH)), "csrc", "exports.map")).read()
    assert re.search(r"global:\s*dvc_\*;", exports)                      # every dvc_ symbol leaves the library
    for name in NEW:
        assert re.search(r"\b%s\(" % name, hdr), name
        assert name in binding.SIGNATURES, name
        assert re.search(r"\b%s\b" % name, out), name
    assert binding.SIGNATURES["dvc_bgemm_split3"] == binding.SIGNATURES["dvc_bgemm_splitk"]
    assert _lib().dvc_abi_version() == binding.ABI_VERSION == 20


def test_split3_refusals_and_workspace_rules_without_gpu():
    lib = _lib()
    f = lib.dvc_bgemm_split3

    def call(A=ONE, B=TWO, C=THREE, batch=2, M=8, N=8, K=8, a=(64, 8, 1), b=(64, 8, 1), c_sb=64, ldc=8, acc=0):
        return f(A, B, C, batch, M, N, K, *a, *b, c_sb, ldc, acc, None, 0, None)
    for kw in (dict(A=None), dict(B=None), dict(C=None)):
        _fails(call(**kw), lib, "null argument")
    for kw in (dict(batch=0), dict(M=0), dict(N=-1), dict(K=0)):
        _fails(call(**kw), lib, "bad shape")
    _fails(call(ldc=7), lib, "ldc")
    _fails(call(a=(64, 8, 2)), lib, "inner stride of A")
    _fails(call(b=(64, 16, 2)), lib, "inner stride of B")
    _fails(call(a=(64, -8, 1)), lib, "negative stride")
    _fails(call(acc=2), lib, "accumulate")
    _fails(call(batch=70000), lib, "too large")
    # one split policy: the same workspace as the fp32 kernel at every size
    for sizes in ((0, 8, 8, 8), (1, 2048, 5184, 256), (3, 128, 128, 256), (1, 256, 2048, 5184), (16, 256, 2048, 5184),
                  (1, 66, 64, 5184), (3, 130, 257, 66)):
        assert lib.dvc_bgemm_split3_workspace_bytes(*sizes) == lib.dvc_bgemm_workspace_bytes(*sizes), sizes
    assert lib.dvc_bgemm_split3_workspace_bytes(1, 66, 64, 5184) == 16 * 66 * 64 * 4
    args = (ONE, TWO, THREE, 1, 66, 64, 5184, 0, 5184, 1, 0, 64, 1, 0, 64, 0)
    _fails(f(*args, None, 0, None), lib, "need a workspace")
    _fails(f(*args, ctypes.c_void_p(8192), 100, None), lib, "workspace too small")
    _fails(f(*args, ctypes.c_void_p(8193), 1 << 30, None), lib, "aligned")


def test_ops_bgemm_engine_keyword():
    from dvc_amd import ops
    a, b = torch.zeros(2, 4, 3), torch.zeros(2, 3, 5)
    with pytest.raises(ValueError, match="bogus"):
        ops.bgemm(a, b, engine="bogus")                                    # before anything looks at a device
    for engine in ("fp32", "split3"):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            ops.bgemm(a, b, engine=engine)


def test_backend_selector_takes_split3():
    from dvc_amd import block_products as bp, ops
    assert bp.backend() is None
    with bp.use_backend("split3"):
        assert bp.backend() == "split3"
        with bp.use_backend("native"):
            assert bp.backend() == "native"
        assert bp.backend() == "split3"
    assert bp.backend() is None
    with pytest.raises(ValueError, match="bogus"):
        bp.set_backend("bogus")
    bp.set_backend("split3")
    try:
        assert bp.backend() == "split3"
    finally:
        bp.set_backend(None)
    assert bp.backend() is None
    assert "split3" in bp.__doc__ and "split3" in bp.backend.__doc__
    assert issubclass(bp._Split3, bp._Views) and bp._Split3.scores is bp._Native.scores      # native's row-block loop
    assert bp._Split3.product.func is ops.bgemm and bp._Split3.product.keywords == {"engine": "split3"}


def test_selection_picks_split3(monkeypatch):
    from dvc_amd import block_products as bp
    picked = []
    monkeypatch.setattr(bp._Views, "__init__", lambda self, *a: picked.append(type(self).__name__))
    with bp.use_backend("split3"):
        bp.block_products(None, None, None, 64, 1)
    assert picked == ["_Split3"]


# ------------------------------------------------------------------------------------------------ the arithmetic, restated
def test_split_is_exact_and_every_term_is_a_bf16():
    x = R.split_inputs()
    assert x.size == 10 ** 6 + 4 + 4 * 228 and np.isfinite(x).all()
    terms = R.split3(x)
    for t in terms:
        assert R.is_bf16(t).all() and np.isfinite(t).all()
    total = terms[0].astype(np.float64) + terms[1].astype(np.float64) + terms[2].astype(np.float64)      # exact in float64
    assert np.array_equal(total.astype(np.float32).view(np.uint32) & 0x7fffffff, x.view(np.uint32) & 0x7fffffff)
    assert np.array_equal(total, x.astype(np.float64))
    zero = x == 0
    assert zero.sum() == 2 and all((t[zero] == 0).all() for t in terms)                                   # zeros stay zeros
    assert np.array_equal(np.signbit(terms[0]), np.signbit(x))
    # the sizes of the terms the bound on the dropped products rests on; the clamped values (|x| >= 0x1.FFp127, x1 = BF16_MAX)
    # have |x2| <= 2^120 against |x| >= 2^128 (1 - 2^-8): the factor 1 + 2^-7 covers them
    ax = np.abs(x[~zero]).astype(np.float64) * (1 + 2.0 ** -7)
    assert (np.abs(terms[1][~zero]) <= 2.0 ** -8 * ax).all() and (np.abs(terms[2][~zero]) <= 2.0 ** -16 * ax).all()
    fmax = np.finfo(np.float32).max
    assert [float(t[0]) for t in R.split3(np.array([fmax], np.float32))] == [float(R.BF16_MAX), 2.0 ** 120, -2.0 ** 104]


def _dropped_ratio(dropped, what):
    a = R.split_inputs()
    b = np.roll(a, SHIFT)
    nz = (a != 0) & (b != 0)
    assert (dropped(a, b)[~nz] == 0).all()
    ratio = np.abs(dropped(a, b)[nz]) / (np.abs(a[nz]).astype(np.float64) * np.abs(b[nz]).astype(np.float64)) / R.U
    print(f"split3 {what} / (U |a||b|): largest {ratio.max():.6f}, rms {np.sqrt((ratio ** 2).mean()):.6f}")
    return ratio.max()


def test_dropped_terms_stay_below_a_quarter_U():
    """What the kernel drops (a3 b3) against U / 4 |a||b| per product; by |x3| <= 2^-16 |x| (1 + 2^-7) it is below U / 250."""
    worst = _dropped_ratio(R.dropped, "dropped term")
    assert worst <= 0.25
    assert worst <= (1 + 2.0 ** -7) ** 2 / 256


def test_the_cross_terms_could_not_be_dropped_too():
    """a2 b3 + a3 b2 + a3 b3, what six products would leave out: over the budget on these inputs, inside its own bound
    (2^-24 + 2^-24 + 2^-32) (1 + 2^-7)^2 < 2 (1 + 2^-5) U."""
    worst = _dropped_ratio(R.dropped_with_the_cross_terms, "dropped term with a2 b3 and a3 b2")
    assert 0.25 < worst <= 2 * (1 + 2.0 ** -5)


def test_integer_and_one_hot_cases_are_exact_in_the_restatement():
    cases = R.integer_cases()
    assert len(cases) == 2 * (5 + 4)
    for name, (A, B, C) in cases.items():
        assert A.shape[0] in (33, 130) and B.shape[1] in (33, 130) and A.shape[1] == B.shape[0] <= 70
        if "one_hot" not in name:
            assert np.array_equal(C.astype(np.int64), A.astype(np.int64) @ B.astype(np.int64)), name
        got = R.kept_products(A, B)
        assert np.array_equal(got, C.astype(np.float64)), name
    # what each case is for: the terms it has, so the products it needs
    A, B, _ = cases["two_planes_33x130"]
    assert all(np.any(t != 0) for t in R.split3(A)[:2] + R.split3(B)[:2]) and not np.any(R.split3(A)[2]) and not np.any(R.split3(B)[2])
    A, B, _ = cases["a_three_33x130"]
    assert np.any(R.split3(A)[2] != 0) and not np.any(R.split3(B)[1])
    A, B, _ = cases["b_three_33x130"]
    assert np.any(R.split3(B)[2] != 0) and not np.any(R.split3(A)[1])
    for name, two, three in (("a2b3_33x130", 0, 1), ("a3b2_33x130", 1, 0)):
        ops_ = cases[name]
        t2, t3 = R.split3(ops_[two]), R.split3(ops_[three])
        assert np.any(t2[1] != 0) and not np.any(t2[2]) and np.any(t3[2] != 0)
        cross = t2[1].astype(np.float64) @ t3[2].astype(np.float64) if two == 0 else t3[2].astype(np.float64) @ t2[1].astype(np.float64)
        assert (cross != 0).all()                                           # every element of C needs the cross product
    A, _, _ = cases["b_one_hot_17_33x130"]
    assert np.any(R.split3(A)[2] != 0)
