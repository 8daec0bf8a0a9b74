"""Float64 restatement of ONE Adam step for ONE tensor (torch.optim.Adam's single-tensor rule), and the bound a float32
implementation of it is held to.  Test infrastructure: tests/test_adam_host.py checks it against torch.optim.Adam on the CPU,
tests/test_gpu_adam.py holds dvc_adam_step (csrc/optim.hip) to it.  Works on any device (torch float64 ops).

The restatement.  Inputs are the float32 p, g, m, v, vmax cast up; the scalars are evaluated in double:
    g'   = g + wd p                       (wd != 0)
    m'   = m + (1 - b1)(g' - m)
    v'   = b2 v + (1 - b2) g'^2
    vmax' = max(vmax, v')                 (amsgrad; it then takes v''s place below)
    denom = sqrt(v') / sqrt(1 - b2^t) + eps
    delta = lr / (1 - b1^t) * m' / denom,      p' = p - delta

The bound, with e = 2^-24 (float32's unit roundoff), G = |g| + wd |p| and S = step_size (|m| + G) / denom:
    |m_hip - m'|       <= C_M e (|m| + G)
    |v_hip - v'|       <= C_V e v'                      (and the same for vmax: a maximum adds no rounding)
    |p_hip - p'|       <= e max(|p|, |p'|) + C_P e (|delta| + S)
It comes from counting the roundings of the kernel's expressions as csrc/optim.hip writes them (explicit fmaf, contraction off,
correctly rounded sqrt and division); each float32 scalar of the table is one rounding of its double value.  To first order in e:
    g' = fma(wd, p, g):                        e wd|p| (wd) + e |g'| (fma)                                <= 2 e G   (0 without wd)
    m  = fma(omb1, g' - m, m):                 omb1 (2 e G  +  e (G + |m|) [the difference]  +  e (G + |m|) [omb1])
                                               + e |m'| [fma], |m'| <= |m| + G, omb1 <= 1                 <= 5 e (|m| + G)
    v  = fma(omb2, g' g', b2 v):               g'^2: 2 x 2 e + e [product] = 5 e, omb2: e  -> 6 e on that term; b2 v: e [b2] + e
                                               [product] = 2 e on the other; both terms >= 0, + e [fma]   <= 7 e v'  (3 e without wd)
    denom = fma(sqrt(v), isbc2, eps):          sqrt: 7/2 e + e, isbc2: e -> 5.5 e on the first term; eps: e on the second;
                                               + e [fma]                                                  <= 6.5 e denom
    p  = fma(-step_size, m / denom, p):        m / denom: 6.5 e + e [division], step_size: e -> 8.5 e |delta|, plus m's own
                                               error 5 e S; the last rounding is the e max(|p|, |p'|) term.
                                               |m'| <= |m| + G makes |delta| <= S, so 8.5 |delta| + 5 S <= 7 (|delta| + S).
Hence C_M = 5, C_V = 7, C_P = 7.  The terms of order e^2 are below 1e-6 of these bounds, and the float64 evaluation's own error
(1e-16 relative) is nine orders below e.

Underflow.  The relative model holds for results in float32's normal range, which the synthetic inputs keep to; the gradients of a
real network do not ask (g = 1e-25 squares to a subnormal).  A result below 2^-126 is rounded with an ABSOLUTE error of at most
h = 2^-149 (one subnormal spacing, twice what round-to-nearest needs) instead; additions and subtractions never underflow
inexactly.  Counting the operations that can: m gets 2 h (the wd fma, the last fma), v gets 3 h (g'^2, b2 v, the fma), and p gets
2 h (the quotient, the fma) plus what v's 3 h does through the square root, |sqrt(v + d) - sqrt(v)| <= sqrt(d):
|delta| sqrt(3 h) / (sqrt(1 - b2^t) denom).  With h = 1.4e-45 these terms are far below every bound above unless the quantities
themselves are below 1e-37; they are added to the bounds as absolute slack.
"""
import math

import torch

EPS = 2.0 ** -24
ETA = 2.0 ** -149          # h above
C_M, C_V, C_P = 5.0, 7.0, 7.0
DEFECTS = ("no_bias_correction", "eps_inside_sqrt", "wd_after_moments")     # (+ a shared step count, seeded by the caller through t)


def step(p, g, m, v, vmax, *, t, lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, amsgrad=False, defect=None):
    """One step number t (>= 1) -> dict(p, m, v, vmax, delta, denom, G, step_size), float64.  vmax may be None without amsgrad."""
    assert defect is None or defect in DEFECTS, defect
    b1, b2 = betas
    p, g, m, v = (x.double() for x in (p, g, m, v))
    G = g.abs() + weight_decay * p.abs()
    g_m = g
    if weight_decay != 0 and defect != "wd_after_moments":
        g_m = g + weight_decay * p
    m2 = m + (1.0 - b1) * (g_m - m)
    v2 = b2 * v + (1.0 - b2) * g_m * g_m
    if defect == "wd_after_moments":        # (the decay added to the update direction instead of to the gradient)
        m2 = m2 + weight_decay * p
    bc1, bc2 = 1.0 - b1 ** t, 1.0 - b2 ** t
    if defect == "no_bias_correction":
        bc1 = bc2 = 1.0
    vm2 = torch.maximum(vmax.double(), v2) if amsgrad else None
    vv = vm2 if amsgrad else v2
    if defect == "eps_inside_sqrt":
        denom = (vv + eps).sqrt() / math.sqrt(bc2)
    else:
        denom = vv.sqrt() / math.sqrt(bc2) + eps
    step_size = lr / bc1
    delta = step_size * m2 / denom
    return dict(p=p - delta, m=m2, v=v2, vmax=vm2, delta=delta, denom=denom, G=G, step_size=step_size, bc2=bc2)


def _ratio(got, ref, unit, slack=None):
    """max over the elements where ref is finite of (|got - ref| - slack) / (EPS unit), 0 where the numerator is <= 0 (so a zero
    unit demands equality up to the slack), as a 0-d tensor; and whether got is non-finite exactly where ref is, NaN for NaN, inf for the same inf."""
    got = got.double()
    finite = torch.isfinite(ref)
    same = torch.equal(torch.isfinite(got), finite) and torch.equal(torch.isnan(got), torch.isnan(ref))
    inf = torch.isinf(ref)
    same = same and bool((got[inf] == ref[inf]).all())
    err = (got - ref).abs()
    if slack is not None:
        err = err - slack
    err, unit = err[finite], (EPS * unit)[finite]
    r = torch.where(err <= 0, torch.zeros_like(err), err / unit)        # err > 0 over unit == 0 -> inf; a NaN unit -> NaN
    worst = r.max() if r.numel() else torch.zeros((), dtype=torch.float64, device=ref.device)
    if r.numel() and bool(torch.isnan(r).any()):
        worst = torch.full_like(worst, float("inf"))
    return worst, same


def achieved(ref, before, got):
    """The constants an implementation reaches on one tensor: before = dict(p, m) BEFORE the step, got = dict(p, m, v[, vmax]) after
    it, ref = step(...).  -> (dict of floats c_m, c_v, c_vmax, c_p; whether every non-finite mask matches)."""
    p0, m0 = before["p"].double(), before["m"].double()
    S = ref["step_size"] * (m0.abs() + ref["G"]) / ref["denom"]
    p_slack = (EPS * torch.maximum(p0.abs(), ref["p"].abs()) + 2 * ETA
               + ref["delta"].abs() * math.sqrt(3 * ETA) / (math.sqrt(ref["bc2"]) * ref["denom"]))
    res = {"c_m": _ratio(got["m"], ref["m"], m0.abs() + ref["G"], slack=2 * ETA),
           "c_v": _ratio(got["v"], ref["v"], ref["v"], slack=3 * ETA),
           "c_p": _ratio(got["p"], ref["p"], ref["delta"].abs() + S, slack=p_slack)}
    if ref["vmax"] is not None:
        res["c_vmax"] = _ratio(got["vmax"], ref["vmax"], ref["vmax"], slack=3 * ETA)
    return {k: float(r[0]) for k, r in res.items()}, all(r[1] for r in res.values())


def within_bound(c):
    return (c["c_m"] <= C_M and c["c_v"] <= C_V and c.get("c_vmax", 0.0) <= C_V and c["c_p"] <= C_P)


def make_p(n, seed, device="cpu"):
    """|p| log-uniform in [1e-4, 1e2], random signs."""
    gen = torch.Generator().manual_seed(seed)
    mag = 10.0 ** (torch.rand(n, generator=gen, dtype=torch.float64) * 6 - 4)
    sign = torch.where(torch.rand(n, generator=gen) < 0.5, -1.0, 1.0).double()
    return (mag * sign).float().to(device)


def make_g(n, seed, like_sign_of=None, device="cpu"):
    """|g| log-uniform in [1e-12, 1e4] with every seventh element exactly 0; random signs, or — for the weight-decay cases, where
    g + wd p must not cancel — the sign of `like_sign_of` (the CURRENT parameter values)."""
    gen = torch.Generator().manual_seed(seed)
    mag = 10.0 ** (torch.rand(n, generator=gen, dtype=torch.float64) * 16 - 12)
    sign = torch.where(torch.rand(n, generator=gen) < 0.5, -1.0, 1.0).double()
    g = (mag * sign).float()
    g[::7] = 0.0
    g = g.to(device)
    if like_sign_of is not None:
        g = g.abs() * torch.sign(like_sign_of.detach().reshape(-1)).to(g)
    return g
