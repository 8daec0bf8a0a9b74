"""Shared by the GPU test modules that call the C-ABI (include/dvc_hip.h) directly: the `ops` / `lib` fixtures (imported into a
test module's namespace), raw-pointer arguments, the return-code check and NaN-filled device tensors."""
import ctypes

import pytest
import torch

NAN = float("nan")


@pytest.fixture(scope="module")
def ops():
    from dvc_amd import ops as o
    return o


@pytest.fixture(scope="module")
def lib():
    from dvc_amd import _lib
    return _lib.load()


def ptr(t):
    """Raw device address of a tensor as a ctypes argument (None -> NULL)."""
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def check(rc, what):
    """Raise with dvc_last_error() unless the entry returned 0."""
    from dvc_amd import _lib
    _lib.check(rc, what)


def nan_tensor(*shape):
    return torch.full(shape, NAN, device="cuda")
