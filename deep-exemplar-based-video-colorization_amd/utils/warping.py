"""Drop-in for the reference's utils/warping.py.

train.py does
    from utils.warping import WarpingLayer
and `consistent_loss_fn` (utils/util.py) warps the current prediction by the forward flow with it.  `WarpingLayer` is this
package's HIP-backed module (dvc_amd/flow_warp.py); `get_grid` is the reference's, restated in plain torch on the input's
device (the reference's calls `.cuda()`).  Every other name is forwarded, on first use, to the next `utils/warping.py` found
on `utils.__path__` — the reference's own file, loaded unmodified under the module name `utils._reference_warping` — exactly
as utils/util.py forwards.
"""
import importlib.util as _ilu
import os as _os
import sys as _sys

import torch as _torch

from dvc_amd.flow_warp import WarpingLayer, flow_warp  # noqa: F401

_HERE = _os.path.dirname(_os.path.abspath(__file__))
_REF_NAME = "utils._reference_warping"


def get_grid(x):
    """[B, 2, H, W]: channel 0 = linspace(-1, 1, W) along x, channel 1 = linspace(-1, 1, H) along y, on x's device."""
    B, _, H, W = x.size()
    torchHorizontal = _torch.linspace(-1.0, 1.0, W, device=x.device).view(1, 1, 1, W).expand(B, 1, H, W)
    torchVertical = _torch.linspace(-1.0, 1.0, H, device=x.device).view(1, 1, H, 1).expand(B, 1, H, W)
    return _torch.cat([torchHorizontal, torchVertical], 1)


def _reference_warping():
    """The reference's utils/warping.py (the first one on utils.__path__ that is not this file), or None."""
    mod = _sys.modules.get(_REF_NAME)
    if mod is not None:
        return mod
    import utils as _pkg
    for d in list(getattr(_pkg, "__path__", [])):
        cand = _os.path.join(d, "warping.py")
        if _os.path.abspath(d) == _HERE or not _os.path.isfile(cand):
            continue
        spec = _ilu.spec_from_file_location(_REF_NAME, cand)
        mod = _ilu.module_from_spec(spec)
        _sys.modules[_REF_NAME] = mod
        try:
            spec.loader.exec_module(mod)
        except BaseException:
            del _sys.modules[_REF_NAME]
            raise
        return mod
    return None


def __getattr__(name):   # PEP 562: only reached for names this module does not define
    if name.startswith("__") and name.endswith("__"):
        raise AttributeError(name)
    ref = _reference_warping()
    if ref is None:
        raise AttributeError(
            f"module 'utils.warping' has no attribute '{name}': this drop-in provides WarpingLayer and get_grid, and no "
            "reference utils/warping.py is on sys.path behind it to forward to")
    return getattr(ref, name)
