"""CPU: WarpingLayer's host side — C-ABI validation, the module's guards, the drop-in of utils/warping.py, and the float64
restatement (tests/flow_warp_reference.py) against an independent numpy composition with analytic gradients."""
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
REF_STANDIN = os.path.join(ROOT, "tests", "golden", "reference_tree")
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import flow_warp_reference as R  # noqa: E402


def _call(lib, which, x=256, flow=256, G=256, B=1, C=3, H=6, W=7, align=0, y=256, dx=256, dflow=256, ws=256, ws_bytes=None):
    p = lambda v: ctypes.c_void_p(v) if v else None  # noqa: E731
    if which == "fwd":
        return lib.dvc_flow_warp_fwd(p(x), p(flow), B, C, H, W, align, p(y), None)
    if ws_bytes is None:
        ws_bytes = 8 * (B * C * H * W + B) if min(B, C, H, W) > 0 else 0
    return lib.dvc_flow_warp_bwd(p(x), p(flow), p(G), B, C, H, W, align, p(dx), p(dflow), p(ws), ws_bytes, None)


@pytest.mark.parametrize("which", ["fwd", "bwd"])
def test_flow_warp_argument_validation_without_gpu(which):
    """dvc_flow_warp_fwd / dvc_flow_warp_bwd report bad arguments through the return code + dvc_last_error, before any launch."""
    from dvc_amd import _lib
    lib = _lib.load()
    assert lib.dvc_abi_version() == _lib.ABI_VERSION == 20
    name = f"dvc_flow_warp_{which}".encode()

    def bad(msg, **kw):
        rc = _call(lib, which, **kw)
        err = lib.dvc_last_error()
        assert rc != 0 and msg in err and err.startswith(name + b":"), (kw, rc, err)

    bad(b"null argument", x=0)
    bad(b"null argument", flow=0)
    bad(b"null argument", **({"y": 0} if which == "fwd" else {"G": 0}))
    for kw in (dict(B=0), dict(B=-1), dict(C=0), dict(C=-2)):
        bad(b"bad shape", **kw)
    for kw in (dict(H=1), dict(W=1), dict(H=0), dict(W=-3), dict(H=1, W=1)):
        bad(b"at least 2", **kw)
    bad(b"above 2^22", H=2048, W=2049)
    bad(b"above 2^22", H=2, W=(1 << 21) + 1)
    for a in (2, -1, 7):
        bad(b"align_corners must be 0 or 1", align=a)
    if which == "bwd":
        bad(b"neither dx nor dflow", dx=0, dflow=0)
        bad(b"workspace", ws=0)
        bad(b"workspace too small", ws_bytes=8 * (3 * 6 * 7 + 1) - 1)
        bad(b"workspace too small", ws_bytes=0)
        # the size the Python side asks for is the one the entry point checks against
        assert lib.dvc_flow_warp_bwd_workspace_bytes(1, 3, 6, 7) == 8 * (3 * 6 * 7 + 1)
        assert lib.dvc_flow_warp_bwd_workspace_bytes(16, 3, 216, 384) == 8 * (16 * 3 * 216 * 384 + 16)
        assert lib.dvc_flow_warp_bwd_workspace_bytes(1, 3, 1, 7) == 0 and lib.dvc_flow_warp_bwd_workspace_bytes(0, 3, 6, 7) == 0


def test_python_guards_without_gpu():
    """Argument errors of the module are raised before anything touches a device."""
    from dvc_amd.flow_warp import WarpingLayer, flow_warp
    x, f = torch.zeros(2, 3, 8, 9), torch.zeros(2, 2, 8, 9)
    for m in (WarpingLayer(), WarpingLayer(True), WarpingLayer(align_corners=False)):
        with pytest.raises(TypeError, match="must be tensors"):
            m(x, f.numpy())
        with pytest.raises(TypeError, match="must be tensors"):
            m(None, f)
        with pytest.raises(ValueError, match="4-D"):
            m(x[0], f)
        with pytest.raises(ValueError, match="4-D"):
            m(x, f[None])
        with pytest.raises(ValueError, match="flow needs 2 channels"):
            m(x, torch.zeros(2, 3, 8, 9))
        with pytest.raises(ValueError, match="batch sizes differ"):
            m(x, f[:1])
        with pytest.raises(ValueError, match="x is 8 x 9, flow is 8 x 8"):
            m(x, f[..., :8])
        with pytest.raises(ValueError, match="x is 8 x 9, flow is 7 x 9"):
            m(x, f[:, :, :7])
        with pytest.raises(ValueError, match="at least 2"):
            m(x[:, :, :1], f[:, :, :1])
        with pytest.raises(ValueError, match="at least 2"):
            m(x[..., :1], f[..., :1])
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            m(x, f)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        flow_warp(x, f, True)
    assert WarpingLayer().align_corners is False and WarpingLayer(None).align_corners is False
    assert WarpingLayer(False).align_corners is False and WarpingLayer(True).align_corners is True


def _run(code):
    env = dict(os.environ, PYTHONDONTWRITEBYTECODE="1")
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stdout + "\n" + r.stderr
    return r.stdout


@pytest.mark.parametrize("behind", [None, REF_STANDIN], ids=["alone", "reference_tree"])
def test_dropin_serves_warping_layer(behind):
    """train.py's `from utils.warping import WarpingLayer` gets the HIP module, with or without a reference tree behind the
    package; get_grid is plain torch on the input's device; a name nobody defines is an AttributeError that says so."""
    path = [PKG] + ([behind] if behind else [])
    code = textwrap.dedent(f'''
        import sys
        sys.dont_write_bytecode = True
        sys.path[:0] = {path!r}
        import torch
        from utils.warping import WarpingLayer, get_grid
        import dvc_amd.flow_warp
        import utils.warping as U
        assert WarpingLayer is dvc_amd.flow_warp.WarpingLayer and U.WarpingLayer is WarpingLayer
        x = torch.zeros(2, 3, 5, 7)
        g = get_grid(x)
        assert g.shape == (2, 2, 5, 7) and g.device == x.device
        assert torch.equal(g[:, 0], torch.linspace(-1.0, 1.0, 7).view(1, 1, 7).expand(2, 5, 7))
        assert torch.equal(g[:, 1], torch.linspace(-1.0, 1.0, 5).view(1, 5, 1).expand(2, 5, 7))
        try:
            U.no_such_name
        except AttributeError as e:
            assert "no reference" in str(e) and "no_such_name" in str(e), str(e)
        else:
            raise AssertionError("an unknown name resolved")
        print("OK")
    ''')
    assert "OK" in _run(code)


def _direct(x, flow, G, align_corners):
    """Independent float64 composition in numpy: explicit floor, weights and in-range masks; analytic dx (scatter) and dflow."""
    x, flow, G = x.double().numpy(), flow.double().numpy(), G.double().numpy()
    B, C, H, W = x.shape
    X = np.arange(W, dtype=np.float64)[None, None, :] + flow[:, 0]
    Y = np.arange(H, dtype=np.float64)[None, :, None] + flow[:, 1]
    sx, sy = (1.0, 1.0) if align_corners else (W / (W - 1), H / (H - 1))
    px, py = (X, Y) if align_corners else (X * W / (W - 1) - 0.5, Y * H / (H - 1) - 0.5)
    x0, y0 = np.floor(px), np.floor(py)
    fx, fy = px - x0, py - y0
    x0, y0 = x0.astype(np.int64), y0.astype(np.int64)
    y, dx, df = np.zeros_like(x), np.zeros_like(x), np.zeros_like(flow)
    bi = np.arange(B)[:, None, None] * np.ones((1, H, W), dtype=np.int64)
    val = {}
    for (oy, ox), w in (((0, 0), (1 - fy) * (1 - fx)), ((0, 1), (1 - fy) * fx), ((1, 0), fy * (1 - fx)), ((1, 1), fy * fx)):
        cy, cx = y0 + oy, x0 + ox
        inr = (cy >= 0) & (cy <= H - 1) & (cx >= 0) & (cx <= W - 1)
        cyc, cxc = np.clip(cy, 0, H - 1), np.clip(cx, 0, W - 1)
        val[oy, ox] = np.stack([np.where(inr, x[bi, c, cyc, cxc], 0.0) for c in range(C)], 1)    # [B, C, H, W], 0 when outside
        y += w[:, None] * val[oy, ox]
        for c in range(C):
            np.add.at(dx, (bi[inr], c, cy[inr], cx[inr]), (w * G[:, c])[inr])
    df[:, 0] = sx * (G * ((1 - fy)[:, None] * (val[0, 1] - val[0, 0]) + fy[:, None] * (val[1, 1] - val[1, 0]))).sum(1)
    df[:, 1] = sy * (G * ((1 - fx)[:, None] * (val[1, 0] - val[0, 0]) + fx[:, None] * (val[1, 1] - val[0, 1]))).sum(1)
    return y, dx, df


@pytest.mark.parametrize("align_corners", [False, True])
@pytest.mark.parametrize("shape", [(2, 3, 7, 9), (1, 1, 2, 2)])
def test_restatement_matches_independent_composition(shape, align_corners):
    B, C, H, W = shape
    gen = torch.Generator().manual_seed(5)
    x = torch.randn(shape, generator=gen) * 50
    G = torch.randn(shape, generator=gen)
    if shape == (1, 1, 2, 2):
        # by hand: a corner out on the left and top, on the right, at the bottom, and one footprint that stays inside
        flow = torch.tensor([[[[-0.6, 0.4], [0.3, -0.55]], [[-0.7, 0.3], [0.45, -0.6]]]])
    else:
        # integer + U(0.05, 0.95): away from the kinks of the derivative; wide enough to push corners out on every side
        flow = torch.randint(-max(H, W) - 1, max(H, W) + 2, (B, 2, H, W), generator=gen).float() * \
            (torch.rand(B, 2, H, W, generator=gen) < 0.3).float() + torch.randint(-2, 3, (B, 2, H, W), generator=gen).float() + \
            0.05 + 0.9 * torch.rand(B, 2, H, W, generator=gen)
    # the kink is at integer SAMPLE coordinates, not integer flows: nudge what lands within 1e-3 of one
    for _ in range(4):
        px, py = R.sample_coords(flow, align_corners)
        flow[:, 0] += ((px - px.round()).abs() < 2e-3).float() * 0.013
        flow[:, 1] += ((py - py.round()).abs() < 2e-3).float() * 0.013
    px, py = R.sample_coords(flow, align_corners)
    assert ((px - px.round()).abs() >= 1e-3).all() and ((py - py.round()).abs() >= 1e-3).all()
    x0, y0 = px.floor(), py.floor()
    inside = (x0 >= 0) & (x0 + 1 <= W - 1) & (y0 >= 0) & (y0 + 1 <= H - 1)
    assert not inside.all()
    if shape != (1, 1, 2, 2):
        # corners leave the image on every side, whole footprints too, and some stay inside
        assert (x0 == -1).any() and (x0 == W - 1).any() and (y0 == -1).any() and (y0 == H - 1).any()
        assert ((x0 < -1) | (x0 > W - 1) | (y0 < -1) | (y0 > H - 1)).any() and inside.any()

    y, dx, df = R.gradients(x, flow, G, align_corners, torch.float64)
    ry, rdx, rdf = _direct(x, flow, G, align_corners)
    assert y.dtype == torch.float64 and tuple(y.shape) == ry.shape

    def rel(a, b):
        return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)

    assert np.abs(ry).max() > 1.0 and np.abs(rdx).max() > 1e-3
    assert np.abs(rdf).max() > 1e-3 * G.abs().max().item()            # dflow is not all-but-zero
    assert rel(y.numpy(), ry) <= 1e-12
    assert rel(dx.numpy(), rdx) <= 1e-12
    assert rel(df.numpy(), rdf) <= 1e-12
    # the float32 yardstick is the same composition
    assert R.warp(x, flow, align_corners, dtype=torch.float32).dtype == torch.float32


def test_default_of_grid_sample_is_align_corners_false():
    """The decision INTEGRATION.md records: the unmodified reference file computes align_corners=False under this torch."""
    import torch.nn.functional as F
    gen = torch.Generator().manual_seed(1)
    x = torch.randn(1, 2, 5, 6, generator=gen, dtype=torch.float64)
    flow = torch.randn(1, 2, 5, 6, generator=gen, dtype=torch.float64)
    f = torch.stack((flow[:, 0] / ((6 - 1.0) / 2.0), flow[:, 1] / ((5 - 1.0) / 2.0)), 1)
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        y = F.grid_sample(x, (R.get_grid(x) + f).permute(0, 2, 3, 1))
    assert torch.equal(y, R.compose(x, flow, False)) and not torch.allclose(y, R.compose(x, flow, True))
