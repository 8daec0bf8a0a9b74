"""CPU: the host side of the library's own batched fp32 GEMM (csrc/bgemm.hip) — header / ctypes table / export agreement, the
C-ABI's argument validation (every refusal comes before any launch, so no device is needed), ops.bgemm's refusals, and the
backend selector of dvc_amd.block_products."""
import ctypes
import os
import re
import subprocess

import pytest
import torch

from cabi_common import _fails, _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ONE, TWO, THREE = ctypes.c_void_p(256), ctypes.c_void_p(1024), ctypes.c_void_p(4096)   # never dereferenced: validation fails first
NEW = ["dvc_bgemm", "dvc_bgemm_splitk", "dvc_bgemm_workspace_bytes"]


def test_new_entry_points_in_header_table_and_exports():
    from dvc_amd import _lib as binding
    hdr = open(os.path.join(ROOT, "include", "dvc_hip.h")).read()
    out = subprocess.run(["nm", "-D", "--defined-only", binding.LIB_PATH], capture_output=True, text=True).stdout
    for name in NEW:
        assert re.search(r"\b%s\(" % name, hdr), name
        assert name in binding.SIGNATURES, name
        assert re.search(r"\b%s\b" % name, out), name
    assert _lib().dvc_abi_version() == binding.ABI_VERSION == 20


def _call(lib, A=ONE, B=TWO, C=THREE, batch=2, M=8, N=8, K=8, a=(64, 8, 1), b=(64, 8, 1), c_sb=64, ldc=8, acc=0):
    return lib.dvc_bgemm(A, B, C, batch, M, N, K, *a, *b, c_sb, ldc, acc, None)


def test_bgemm_validation_without_gpu():
    lib = _lib()
    for kw in (dict(A=None), dict(B=None), dict(C=None)):
        _fails(_call(lib, **kw), lib, "null argument")
    for kw in (dict(batch=0), dict(M=0), dict(N=-1), dict(K=0)):
        _fails(_call(lib, **kw), lib, "bad shape")
    _fails(_call(lib, ldc=7), lib, "ldc")
    _fails(_call(lib, a=(64, 8, 2)), lib, "inner stride of A")
    _fails(_call(lib, b=(64, 16, 2)), lib, "inner stride of B")
    _fails(_call(lib, a=(64, -8, 1)), lib, "negative stride")
    _fails(_call(lib, acc=2), lib, "accumulate")
    _fails(_call(lib, batch=70000), lib, "too large")


def test_bgemm_splitk_workspace_rules_without_gpu():
    lib = _lib()
    wsb = lib.dvc_bgemm_workspace_bytes
    assert wsb(0, 8, 8, 8) == 0 and wsb(1, 8, 0, 8) == 0
    # many tiles or a short K: not split, no workspace
    assert wsb(1, 2048, 5184, 256) == 0
    assert wsb(3, 128, 128, 256) == 0
    # d L = M dS^T of the production size: 2 x 16 tiles, K = 5184 -> 8 slices; the slice count does not depend on the batch
    one = wsb(1, 256, 2048, 5184)
    assert one == 8 * 256 * 2048 * 4
    assert wsb(16, 256, 2048, 5184) == 16 * one
    assert wsb(1, 66, 64, 5184) == 16 * 66 * 64 * 4                     # one tile: the cap of 16 slices
    f = lib.dvc_bgemm_splitk
    args = (ONE, TWO, THREE, 1, 66, 64, 5184, 0, 5184, 1, 0, 64, 1, 0, 64, 0)
    _fails(f(*args, None, 0, None), lib, "need a workspace")
    _fails(f(*args, ctypes.c_void_p(8192), 100, None), lib, "workspace too small")
    _fails(f(*args, ctypes.c_void_p(8193), 1 << 30, None), lib, "aligned")
    _fails(f(None, TWO, THREE, 1, 8, 8, 8, 0, 8, 1, 0, 8, 1, 0, 8, 0, None, 0, None), lib, "null argument")
    _fails(f(ONE, TWO, THREE, 1, 8, 8, 8, 0, 8, 1, 0, 8, 1, 0, 4, 0, None, 0, None), lib, "ldc")


def test_ops_bgemm_refuses_cpu_tensors():
    from dvc_amd import ops
    a, b = torch.zeros(2, 4, 3), torch.zeros(2, 3, 5)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.bgemm(a, b)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.bgemm(a, b, out=torch.zeros(2, 4, 5), accumulate=True)


def test_inner_stride_rule():
    """One inner stride must be 1; a dimension of size 1 never decides."""
    from dvc_amd import ops
    t = torch.zeros(2, 6, 8)
    assert ops._inner_strides(t, "a") == (48, 8, 1)
    assert ops._inner_strides(t.transpose(1, 2), "a") == (48, 1, 8)
    assert ops._inner_strides(t[:, :, 2:5], "a") == (48, 8, 1)
    assert ops._inner_strides(t[:1], "a")[0] == 0
    assert ops._inner_strides(t[:, :, ::2][:, :, :1], "a") == (48, 8, 1)         # K = 1 with a stride of 2
    assert ops._inner_strides(t[:, :1, ::2].transpose(1, 2), "a")[1:] in ((2, 1), (1, 2))
    with pytest.raises(RuntimeError, match="inner stride"):
        ops._inner_strides(t[:, :, ::2], "a")


def test_backend_selector():
    from dvc_amd import block_products as bp
    assert bp.backend() is None
    with pytest.raises(ValueError, match="bogus"):
        bp.set_backend("bogus")
    assert bp.backend() is None
    for name in ("vendor", "engine", "native"):
        with bp.use_backend(name):
            assert bp.backend() == name
            with bp.use_backend(None):
                assert bp.backend() is None
            assert bp.backend() == name
        assert bp.backend() is None
    with pytest.raises(KeyError):
        with bp.use_backend("native"):
            raise KeyError("x")
    assert bp.backend() is None
    with pytest.raises(ValueError):
        with bp.use_backend("nope"):
            pass
    assert bp.backend() is None
    bp.set_backend("native")
    try:
        assert bp.backend() == "native"
    finally:
        bp.set_backend(None)
    assert bp.backend() is None


def test_selection_picks_the_class_and_default_follows_gemm_lib(monkeypatch):
    from dvc_amd import block_products as bp, ops
    picked = []
    for cls in ("_Vendor", "_Engine", "_Native"):
        monkeypatch.setattr(getattr(bp, cls), "__init__", lambda self, *a, _c=cls: picked.append(_c))
    for lib_on, expect in ((True, "_Vendor"), (False, "_Engine")):
        monkeypatch.setattr(ops, "_gemm_lib", lib_on)
        bp.block_products(None, None, None, 64, 1)
        assert picked[-1] == expect
        for name, cls in (("vendor", "_Vendor"), ("engine", "_Engine"), ("native", "_Native")):
            with bp.use_backend(name):
                bp.block_products(None, None, None, 64, 1)
            assert picked[-1] == cls
    assert bp._Vendor.product is ops.bmm and bp._Native.product is ops.bgemm
    assert bp._Vendor.scores is bp._Native.scores                       # one implementation, two product functions
