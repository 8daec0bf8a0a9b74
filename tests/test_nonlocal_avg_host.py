"""CPU: NonlocalWeightedAverage's host side — C-ABI validation, the workspace bound, the drop-in forwarding of
models/NonlocalNet.py, and the float64 restatement (tests/nlwa_reference.py) against an independent composition."""
import ctypes
import os
import subprocess
import sys
import textwrap

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "deep-exemplar-based-video-colorization_amd")
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import nlwa_reference as R  # noqa: E402


def _fwd(lib, patch_size=3, alpha=0.5, ws_bytes=None):
    one = ctypes.c_void_p(256)
    B, C, H, W = 1, 8, 6, 7
    if ws_bytes is None:
        ws_bytes = lib.dvc_nlwa_workspace_bytes(B, C, 3, H, W)
    return lib.dvc_nlwa_fwd(one, 3, H, W, one, C, H, W, B, H, W, 1.0, 1.0, 1.0, 1.0, patch_size, alpha, one, one, ws_bytes,
                            None)


def test_nlwa_argument_validation_without_gpu():
    """dvc_nlwa_fwd reports bad arguments through the return code + dvc_last_error, before any launch."""
    from dvc_amd import _lib
    lib = _lib.load()
    assert lib.dvc_abi_version() == _lib.ABI_VERSION == 20
    rc = _fwd(lib, patch_size=4)
    assert rc != 0 and b"patch_size must be odd" in lib.dvc_last_error()
    rc = _fwd(lib, patch_size=0)
    assert rc != 0 and b"patch_size must be odd" in lib.dvc_last_error()
    for alpha in (0.0, -0.1, float("inf"), float("nan")):
        rc = _fwd(lib, alpha=alpha)
        assert rc != 0 and b"alpha must be > 0" in lib.dvc_last_error(), alpha
    need = lib.dvc_nlwa_workspace_bytes(1, 8, 3, 6, 7)
    assert need > 0
    rc = _fwd(lib, ws_bytes=need - 1)
    assert rc != 0 and b"workspace too small" in lib.dvc_last_error()
    assert lib.dvc_nlwa_workspace_bytes(0, 8, 3, 6, 7) == 0


def test_nlwa_workspace_holds_nothing_n_by_n():
    """At the benchmark shape's largest batch the whole workspace is smaller than ONE N x N fp32 affinity matrix."""
    from dvc_amd import _lib
    lib = _lib.load()
    N = 54 * 96
    ws = lib.dvc_nlwa_workspace_bytes(16, 128, 3, 54, 96)
    assert 0 < ws < N * N * 4, ws


def test_python_guards_without_gpu():
    """Argument errors of the module are raised before anything touches a device."""
    from dvc_amd.nonlocal_avg import NonlocalWeightedAverage, workspace_layout
    m = NonlocalWeightedAverage()
    x, f = torch.zeros(1, 3, 8, 8), torch.zeros(1, 4, 8, 8)
    for kw, msg in ((dict(patch_size=2), "odd"), (dict(patch_size=0), "odd"), (dict(alpha=0.0), "alpha"),
                    (dict(alpha=float("nan")), "alpha"), (dict(alpha=-1.0), "alpha")):
        with pytest.raises(ValueError, match=msg):
            m(x, f, **kw)
    with pytest.raises(ValueError, match="batch sizes differ"):
        m(x, torch.zeros(2, 4, 8, 8))
    with pytest.raises(NotImplementedError, match=r"\.detach\(\)"):
        m(x, f.clone().requires_grad_())
    with pytest.raises(RuntimeError, match="no CPU"):
        m(x, f)
    lay = workspace_layout(2, 40, 3, 5, 7)
    assert lay["fpad"] == (0, (2, 64, 7, 9)) and lay["ab"][1] == (2, 2, 5, 7) and lay["ab"][0] % 256 == 0


def _run(code):
    env = dict(os.environ, PYTHONDONTWRITEBYTECODE="1")
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stdout + "\n" + r.stderr
    return r.stdout


def test_dropin_forwards_reference_only_names(tmp_path):
    """models.NonlocalNet: NonlocalWeightedAverage from this package, every other name from the reference's file behind it."""
    ref = tmp_path / "reference"
    (ref / "models").mkdir(parents=True)
    (ref / "models" / "NonlocalNet.py").write_text(
        "class WeightedAverage:\n    pass\n\n\nclass NonlocalWeightedAverage:\n    pass\n")
    code = textwrap.dedent(f'''
        import sys
        sys.dont_write_bytecode = True
        sys.path[:0] = [{PKG!r}, {str(ref)!r}]
        from models.NonlocalNet import VGG19_pytorch, WarpNet, NonlocalWeightedAverage, WeightedAverage
        import dvc_amd.nets, dvc_amd.nonlocal_avg
        assert VGG19_pytorch is dvc_amd.nets.VGG19_pytorch and WarpNet is dvc_amd.nets.WarpNet
        assert NonlocalWeightedAverage is dvc_amd.nonlocal_avg.NonlocalWeightedAverage
        assert sys.modules[WeightedAverage.__module__].__file__ == {str(ref / "models" / "NonlocalNet.py")!r}
        try:
            from models.NonlocalNet import no_such_name
        except ImportError:
            pass
        else:
            raise AssertionError("unknown name resolved")
        print("OK")
    ''')
    assert "OK" in _run(code)


def test_dropin_without_reference_explains():
    code = textwrap.dedent(f'''
        import sys
        sys.dont_write_bytecode = True
        sys.path.insert(0, {PKG!r})
        from models.NonlocalNet import NonlocalWeightedAverage
        import models.NonlocalNet as M
        try:
            M.WeightedAverage
        except AttributeError as e:
            assert "no reference" in str(e) and "WeightedAverage" in str(e), str(e)
        else:
            raise AssertionError("WeightedAverage resolved without a reference behind the package")
        print("OK")
    ''')
    assert "OK" in _run(code)


def _direct(x_lab, feature, k, alpha, scale_factor):
    """Independent float64 composition: explicit zero-padded patch gather (no F.unfold), numpy GEMM, max-shifted softmax."""
    xr, fr = R.resize(x_lab, feature, scale_factor)
    B, C, H, W = fr.shape
    p = k // 2
    fp = np.zeros((B, C, H + 2 * p, W + 2 * p))
    fp[:, :, p:p + H, p:p + W] = fr.double().numpy()
    U = np.empty((B, C, k, k, H, W))
    for ky in range(k):
        for kx in range(k):
            U[:, :, ky, kx] = fp[:, :, ky:ky + H, kx:kx + W]
    U = U.reshape(B, C * k * k, H * W)
    ab = xr[:, 1:3].double().numpy().reshape(B, 2, H * W)
    out = np.empty((B, 2, H * W))
    for b in range(B):
        S = U[b].T @ U[b] / alpha
        E = np.exp(S - S.max(axis=1, keepdims=True))
        A = E / E.sum(axis=1, keepdims=True)
        out[b] = (A @ ab[b].T).T
    return out.reshape(B, 2, H, W)


@pytest.mark.parametrize("case", [
    # x_lab shape, feature shape, k, alpha, scale_factor
    ((1, 3, 7, 9), (1, 5, 7, 9), 3, 0.5, 1),
    ((2, 3, 12, 10), (2, 3, 3, 5), 5, 0.1, 0.5),
    ((1, 3, 16, 20), (1, 2, 7, 6), 1, 2.0, 0.25),
    ((1, 4, 9, 11), (1, 6, 9, 11), 3, 10.0, 1),
])
def test_restatement_matches_independent_composition(case):
    xs, fs, k, alpha, sf = case
    g = torch.Generator().manual_seed(7)
    x = torch.rand(xs, generator=g) * 220 - 110
    f = torch.randn(fs, generator=g) * 0.6
    got = R.nonlocal_weighted_average(x, f, k, alpha, sf)
    ref = _direct(x, f, k, alpha, sf)
    assert got.dtype == torch.float64 and tuple(got.shape) == ref.shape
    np.testing.assert_allclose(got.numpy(), ref, rtol=0, atol=1e-9)
