"""A float64 restatement of the pixel-loss terms of dvc_amd.losses (csrc/loss.hip), on any device, and the bounds the tests hold
the kernels to.

A term is value = scale * mean(w * |x - t|^p), p in {1, 2}; `term(...)` returns, all float64 on the fp32 inputs as they are,
    value64 = scale * mean(w * |x - t|^p)
    A       = |scale| * mean(|w| * |x - t|^p)        what the value's error is measured in: no cancellation between elements
    dx64    = d value / d x, per element: scale / n * w * 2 (x - t)   or   scale / n * w * sgn(x - t), sgn(0) = 0

The bounds are derived, not measured.  Per element the kernel rounds at most four times in fp32 (the subtraction; the square, or
none for |d|; the weight; the subtraction's error enters the square twice: (1 + e)^2), the value is rounded once at its store, and
the double accumulation of n <= 2^24 fp32 numbers contributes below 2^-28: |value - value64| <= C_VALUE * EPS * A with no
absolute term.  A gradient element sees the coefficient's rounding, the subtraction, the product with the weight and the product
with d: |dx - dx64| <= C_GRAD * EPS * |dx64|.
"""
import torch

EPS = 2.0 ** -24
C_VALUE = 6.0
C_GRAD = 6.0
POWER = {"mse": 2, "l1": 1}


def expand_weights(x, w):
    """w as the kernel reads it: None, x's shape, or [B,1,H,W] over the channels of x [B,C,H,W]."""
    return None if w is None else w.expand_as(x)


def term(kind, x, t=0, w=None, scale=1.0, upstream=1.0):
    """-> dict(value64, A, dx64): see the module docstring.  `t` a tensor of x's shape or a Python number; `upstream` multiplies
    dx64 (the gradient that reaches the term's value)."""
    p = POWER[kind]
    x64 = x.detach().double()
    t64 = t.detach().double() if isinstance(t, torch.Tensor) else torch.full_like(x64, float(torch.tensor(float(t), dtype=torch.float32)))
    d = x64 - t64
    e = d * d if p == 2 else d.abs()
    w64 = torch.ones_like(x64) if w is None else expand_weights(x, w).detach().double()
    s = float(torch.tensor(float(scale), dtype=torch.float32))          # the table carries the scale as fp32
    n = x.numel()
    value64 = s * (w64 * e).sum() / n
    A = abs(s) * (w64.abs() * e).sum() / n
    dx64 = upstream * s / n * w64 * (2 * d if p == 2 else torch.sign(d))
    return dict(value64=float(value64), A=float(A), dx64=dx64)


def value_within_bound(value, ref):
    return abs(float(value) - ref["value64"]) <= C_VALUE * EPS * ref["A"]


def value_error(value, ref):
    """|value - value64| in units of EPS * A (the bound is C_VALUE)."""
    return abs(float(value) - ref["value64"]) / (EPS * ref["A"]) if ref["A"] > 0 else (0.0 if float(value) == ref["value64"] else float("inf"))


def grad_error(dx, ref):
    """max over elements of |dx - dx64| / (EPS * |dx64|) (the bound is C_GRAD); inf if an element with dx64 == 0 is not 0."""
    dx, want = dx.detach().double().cpu(), ref["dx64"].cpu()
    zero = want == 0
    if bool((dx[zero] != 0).any()):
        return float("inf")
    if bool(zero.all()):
        return 0.0
    return float(((dx[~zero] - want[~zero]).abs() / (EPS * want[~zero].abs())).max())


def fp32_composition(kind, x, t=0, w=None, scale=1.0):
    """The same expression in fp32 arithmetic with a float64 sum — what a correct kernel computes, on any device."""
    d = x - t
    e = d * d if POWER[kind] == 2 else d.abs()
    v = e if w is None else expand_weights(x, w) * e
    s = float(torch.tensor(float(scale), dtype=torch.float32))
    return float(torch.tensor(float(v.double().sum()) * s / x.numel(), dtype=torch.float32))


def make_case(shape, seed, mask=None, signed=False, device="cpu"):
    """x, t ~ randn of `shape`, and a weight of shape `mask` (None: no weight) drawn from {0, 1}, or signed: randn."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(shape, generator=g)
    t = torch.randn(shape, generator=g)
    w = None
    if mask is not None:
        w = torch.randn(mask, generator=g) if signed else (torch.rand(mask, generator=g) < 0.6).float()
    return x.to(device), t.to(device), None if w is None else w.to(device)
