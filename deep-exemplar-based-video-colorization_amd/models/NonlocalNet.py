"""Drop-in for /root/reference/models/NonlocalNet.py.  The hot-path classes (test.py:19 imports `VGG19_pytorch, WarpNet`)
live in dvc_amd.nets, the training side's smoothness terms `NonlocalWeightedAverage` in dvc_amd.nonlocal_avg and
`WeightedAverage_color` in dvc_amd.local_avg, all MI355X HIP implementations.  Every other name of the reference's file
(`WeightedAverage`, `find_local_patch`, the GAN and VGG helpers) is forwarded, on first use, to the next
`models/NonlocalNet.py` on `models.__path__` — the reference's own file, loaded unmodified."""
import importlib.util as _ilu
import os as _os
import sys as _sys

from dvc_amd.local_avg import WeightedAverage_color  # noqa: F401
from dvc_amd.nets import VGG19_pytorch, WarpNet  # noqa: F401
from dvc_amd.nonlocal_avg import NonlocalWeightedAverage  # noqa: F401

_HERE = _os.path.dirname(_os.path.abspath(__file__))
_REF_NAME = "models._reference_NonlocalNet"


def _reference_module():
    mod = _sys.modules.get(_REF_NAME)
    if mod is not None:
        return mod
    import models as _pkg
    for d in list(getattr(_pkg, "__path__", [])):
        cand = _os.path.join(d, "NonlocalNet.py")
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
    ref = _reference_module()
    if ref is None:
        raise AttributeError(f"module 'models.NonlocalNet' has no attribute '{name}' and no reference "
                             "models/NonlocalNet.py is on sys.path behind it to forward to")
    return getattr(ref, name)
