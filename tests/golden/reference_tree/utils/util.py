"""Placeholder for the reference's utils/util.py: the host I/O helpers test.py:20-21 imports."""


def batch_lab2rgb_transpose_mc(*args, **kwargs):
    raise NotImplementedError("placeholder")


def folder2vid(*args, **kwargs):
    raise NotImplementedError("placeholder")


def mkdir_if_not(*args, **kwargs):
    raise NotImplementedError("placeholder")


def save_frames(*args, **kwargs):
    raise NotImplementedError("placeholder")
