"""A float64 restatement of every term kind of dvc_amd.losses.Plan (csrc/loss_plan.hip), on any device, and the bounds the tests hold
the kernels to.  The bounds are derived here, not measured; u = EPS = 2^-24 is the unit roundoff of fp32.

"l1", "mse": tests/losses_reference.py, unchanged (|value - value64| <= 6 u A, |dx - dx64| <= 6 u |dx64|).

"mean", value = scale * mean(w * (x - t)).  Per element the kernel rounds twice (the subtraction, the product with w; once without
w), the value once at its store; the scale is the fp32 number the table carries and the restatement uses the same.  The double
accumulation of n <= 2^24 fp32 numbers adds below n 2^-53 <= u / 32.  There is no |.|, so the error is measured against
    A = |scale| * mean(|w| * |x - t|)                       not against the possibly cancelling value:
    |value - value64| <= C_MEAN_VALUE u A,  C_MEAN_VALUE = 4  (three roundings, and one unit for second order and the accumulation).
dx = c_k * w with c_k = (float)(upstream * scale / n): two roundings, |dx - dx64| <= C_MEAN_GRAD u |dx64|, C_MEAN_GRAD = 3.

"rel", value = scale * mean(d^2), d = (x - m) - c, m = mean(y).  With m64 the exact mean of the fp32 y and M = mean|y|:
    m = fl(S_y / n_y), S_y a double sum:  |m - m64| <= u |m64| (1 + 2^-5) <= u M (1 + 2^-5).
    a = fl(x - m) = (x - m)(1 + e1),  d = fl(a - c) = (a - c)(1 + e2),  and x - m = d64 + c - (m - m64), so
    |d - d64| = |(x - m)(e1 + e2 + e1 e2) - c e2 - (m - m64)| <= u E (1 + 2^-4),   E = 2 |x - m64| + |c| + M
    — the last summand of E is the extra term for the fp32 mean: it is off by a relative 2^-24 of mean|y|.
    v = fl(d^2) = d^2 (1 + e3):  |v - d64^2| <= |d - d64| (2 |d64| + |d - d64|) + u d^2
                                          <= u (2 |d64| E + d64^2) (1 + 2^-4) + 4 u^2 (E^2 + d64^2)
    and the value is rounded once more at its store, so with A = |scale| * mean(d64^2) = |value64|
    |value - value64| <= SLACK u (|scale| * mean(2 |d64| E) + 2 A) + 4 u^2 |scale| * mean(E^2 + d64^2),   SLACK = 1 + 2^-4;
    the mean's error enters through 2 mean|d| M.  SLACK covers the double accumulations (n <= 2^24: n 2^-53 <= u / 32) and what is
    left of the second order; the explicit u^2 term keeps the bound meaningful when every d64 is 0.
    dx = fl(c2 d), c2 = 2 fl(upstream scale / n) (the doubling is exact), g = 2 upstream scale / n:
    |dx - dx64| <= SLACK u |g| (E + 2 |d64|)                      (the error of d, the coefficient's rounding, the product's)
    dy = fl(-c2 (sum d) / n_y), sum d a double sum of the fp32 d:  |sum d - sum d64| <= SLACK u sum E, then two roundings:
    |dy - dy64| <= SLACK u |g| / n_y (sum E + 2 |sum d64|).

The literal torch expression torch.mean((x - torch.mean(y) - c) ** 2) sums in fp32 in an order torch does not state; for ANY order
the sum of n numbers is off by at most (n - 1) u sum|.|, so its m is within (n_y + 1) u M and its outer mean within (n_x + 1) u of the
sum of its squares: `torch_rel_bound` is the bound above with M replaced by (n_y + 1) M in E and 2 A by (n_x + 3) A.
"""
import torch

from losses_reference import C_GRAD, C_VALUE, EPS, term as pixel_term  # noqa: F401  (the two unchanged kinds)

C_MEAN_VALUE = 4.0
C_MEAN_GRAD = 3.0
SLACK = 1.0 + 2.0 ** -4


def _f32(v):
    return float(torch.tensor(float(v), dtype=torch.float32))


def mean_term(x, t=0, w=None, scale=1.0, upstream=1.0):
    """-> dict(value64, A, dx64) of scale * mean(w * (x - t)); dt64 = -dx64."""
    x64 = x.detach().double()
    t64 = t.detach().double() if isinstance(t, torch.Tensor) else torch.full_like(x64, _f32(t))
    w64 = torch.ones_like(x64) if w is None else w.expand_as(x).detach().double()
    s, n = _f32(scale), x.numel()
    d = x64 - t64
    return dict(value64=float(s * (w64 * d).sum() / n), A=float(abs(s) * (w64.abs() * d.abs()).sum() / n),
                dx64=upstream * s / n * w64)


def mean_value_bound(ref):
    return C_MEAN_VALUE * EPS * ref["A"]


def mean_grad_error(dx, ref):
    """max |dx - dx64| / (EPS |dx64|) (the bound is C_MEAN_GRAD); inf if an element with dx64 == 0 is not 0."""
    dx, want = dx.detach().double().cpu().reshape(-1), ref["dx64"].cpu().reshape(-1)
    zero = want == 0
    if bool((dx[zero] != 0).any()):
        return float("inf")
    return 0.0 if bool(zero.all()) else float(((dx[~zero] - want[~zero]).abs() / (EPS * want[~zero].abs())).max())


def rel_term(x, y, c, scale=1.0, upstream=1.0, y_sum_slack=1.0, x_sum_slack=0.0):
    """-> dict(value64, value_bound, dx64, dx_bound (per element), dy64, dy_bound) of scale * mean(((x - mean(y)) - c)^2): see the
    module docstring.  y_sum_slack multiplies M in E and x_sum_slack is added to the 2 of 2 A (torch_rel_bound's replacements)."""
    x64, y64 = x.detach().double().reshape(-1), y.detach().double().reshape(-1)
    s, cc, n, n_y = _f32(scale), _f32(c), x.numel(), y.numel()
    m64 = y64.sum() / n_y
    M = y64.abs().sum() / n_y
    d = x64 - m64 - cc
    E = 2 * (x64 - m64).abs() + abs(cc) + y_sum_slack * M
    A = abs(s) * (d * d).sum() / n
    value_bound = (SLACK * EPS * (abs(s) * (2 * d.abs() * E).sum() / n + (2 + x_sum_slack) * A)
                   + 4 * EPS * EPS * abs(s) * (E * E + d * d).sum() / n)
    g = 2 * upstream * s / n
    return dict(value64=float(s * (d * d).sum() / n), value_bound=float(value_bound),
                dx64=(g * d).reshape(x.shape), dx_bound=(SLACK * EPS * abs(g) * (E + 2 * d.abs())).reshape(x.shape),
                dy64=float(-g * d.sum() / n_y), dy_bound=float(SLACK * EPS * abs(g) / n_y * (E.sum() + 2 * d.sum().abs())))


def torch_rel_bound(x, y, c, scale=1.0):
    """The bound of the literal fp32 torch expression against float64, whatever order torch sums in."""
    return rel_term(x, y, c, scale, y_sum_slack=y.numel() + 1, x_sum_slack=x.numel() + 1)["value_bound"]


def torch_rel(x, y, c, scale=1.0):
    """INTEGRATION.md's expression, literally, on x's device in fp32."""
    return scale * torch.mean((x - torch.mean(y) - c) ** 2)


def rel_fp32_composition(x, y, c, scale=1.0):
    """The kernel's arithmetic restated with torch ops: the double sum of y rounded once to m, two fp32 subtractions, an fp32 square,
    a double sum — what a correct kernel computes up to the order of its double sums."""
    m = (y.detach().double().sum() / y.numel()).float()
    d = (x.detach() - m) - _f32(c)
    return float(torch.tensor(float((d * d).double().sum()) * _f32(scale) / x.numel(), dtype=torch.float32))


def rel_errors(value, dx, dy, ref):
    """(value, worst dx element, dy) errors as fractions of their bounds; a zero bound demands an exact result."""
    def frac(err, bound):
        return 0.0 if err == 0 else (err / bound if bound > 0 else float("inf"))
    ev = frac(abs(float(value) - ref["value64"]), ref["value_bound"])
    ex = ey = 0.0
    if dx is not None:
        err, bound = (dx.detach().double().cpu() - ref["dx64"].cpu()).abs().reshape(-1), ref["dx_bound"].cpu().reshape(-1)
        ok = bound > 0
        ex = float("inf") if bool((err[~ok] != 0).any()) else (float((err[ok] / bound[ok]).max()) if bool(ok.any()) else 0.0)
    if dy is not None:
        flat = dy.detach().double().cpu().reshape(-1)
        ey = max(frac(float((flat - ref["dy64"]).abs().max()), ref["dy_bound"]), 0.0)
    return ev, ex, ey
