"""Shared by the host-side tests of the backward entry points (test_vgg / test_cvn / test_warp_backward_host.py): the loaded
library, and the check that a call was refused with a given text in dvc_last_error()."""


def _lib():
    from dvc_amd import _lib
    return _lib.load()


def _fails(rc, lib, needle):
    assert rc != 0, "accepted"
    msg = lib.dvc_last_error()
    assert needle.encode() in msg, msg
