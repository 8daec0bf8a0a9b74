"""Placeholder for the reference's utils/util_distortion.py: the transforms test.py:22 imports."""


class CenterPad:
    pass


class Normalize:
    pass


class RGB2Lab:
    pass


class ToTensor:
    pass
