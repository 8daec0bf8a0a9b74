"""Placeholder for the reference's models/ContextualLoss.py: the names other than the two losses this package provides."""


class ContextualLoss:
    pass


class ContextualLoss_forward:
    pass


class ContextualLoss_complex:
    pass


class ChamferDistance_loss:
    pass
