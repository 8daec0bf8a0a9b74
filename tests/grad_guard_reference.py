"""Float64 restatement of the gradient guard (csrc/optim.hip: dvc_grad_norm, dvc_adam_advance_guarded, dvc_adam_step_guarded,
dvc_grad_scale; dvc_amd.optim.GuardedAdam / grad_norm / clip_grad_norm_) and the bounds an implementation is held to.  Test
infrastructure: tests/test_grad_guard_host.py checks it against torch.nn.utils.clip_grad_norm_ and torch.optim.Adam on float64 CPU
tensors, tests/test_gpu_grad_guard.py holds the kernels to it.

The restatement.  For fp32 gradients g (all tensors of a step together, n elements):
    S    = sum g_i^2          every square is exact in double (24 x 24 bits of significand, exponent range to spare), and the sum is
                              taken with math.fsum, i.e. S is the correctly rounded value of the exact sum
    norm = sqrt(S),   c = min(1, max_norm / (norm + 1e-6))         (torch.nn.utils.clip_grad_norm_'s coefficient; max_norm None: 1)
    S NaN or inf:     the step is skipped — no state changes, `step` included — and skipped += 1
    otherwise:        every tensor takes tests/adam_reference.py's step number t + 1 on the gradient fl32(fl32(c) * g)

The bounds, with u = 2^-53 and e = 2^-24, for results in fp32's NORMAL range (no absolute terms):

  Norm.  The device adds the n exact squares in double in some fixed order: n - 1 additions of non-negative numbers, each with
  relative error at most u, so S_dev = S (1 + d) with |d| <= (1 + u)^(n-1) - 1 =: gamma.  Its sqrt is taken with an error of at
  most one double ulp (|s| <= 2 u; a correctly rounded sqrt halves that), and sqrt(1 + d) lies within 1 +- |d| / 2 (1 + |d|), so
  norm_dev64 = norm (1 + r), |r| <= gamma / 2 (1 + gamma) + 2 u (1 + gamma).  One rounding to fp32 multiplies by (1 + h),
  |h| <= e.  For n <= 2^20, gamma <= n u (1 + 2^-32), and collecting terms
      |total_norm - norm| <= (e + (n / 2 + 2) u) (1 + 2^-23) norm  <=  (1 + (n + 5) 2^-30) 2^-24 norm =: NORM_BOUND(n) norm,
  because (n / 2 + 2) u = (n + 4) 2^-30 2^-24 and the remaining factor (1 + 2^-23) costs less than the one extra 2^-30 2^-24.
  (The restatement's own S is correctly rounded: another u, inside the + 5.)  For the test sizes (n <= 21,000) this is 1.00002 e:
  the fp32 rounding is all that can be seen, and sumsq itself is held to |S_dev - S| <= n u S.

  Coefficient.  Let c64 be the restatement's double value.  The device evaluates max_norm / (norm_dev64 + 1e-6) in double from a
  norm that is off by r above (<= 1.2e-12 relative for the test sizes) with two more double roundings, then min, then ONE rounding
  to fp32.  The double result is within 2e-12 relative of c64 — 3e-5 of an fp32 ulp — so the two fp32 roundings can land on
  adjacent floats only:  |clip_coef - fl32(c64)| <= 1 fp32 ulp.

  Step.  dvc_adam_step_guarded is dvc_adam_step on the gradient fl32(clip_coef * g): one IEEE multiply, which the restatement
  performs identically in fp32 before casting up.  Given the DEVICE's clip_coef, adam_reference's bounds hold with its constants
  C_M, C_V, C_P unchanged.
"""
import math
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import adam_reference as A  # noqa: E402

E = 2.0 ** -24
U = 2.0 ** -53
DEFECTS = ("eps_dropped", "no_clamp", "advance_on_skip", "per_tensor_norm")


def norm_bound(n):
    """Relative bound on |total_norm - norm| for n <= 2^20 elements (the derivation is in the module docstring)."""
    assert 1 <= n <= 2 ** 20, n
    return (1.0 + (n + 5) * 2.0 ** -30) * E


def sumsq(grads):
    """The correctly rounded double value of sum g^2 over every tensor of `grads` (fp32 or fp64 tensors), as a Python float."""
    total = []
    for g in grads:
        d = g.detach().double().cpu().reshape(-1)
        total.append((d * d).numpy())           # exact for fp32 inputs
    return math.fsum(np.concatenate(total).tolist()) if total else 0.0


def norm(grads):
    s = sumsq(grads)
    return math.sqrt(s) if s == s and s >= 0 else s     # (sqrt(nan) = nan, sqrt(inf) = inf; math.sqrt raises on neither)


def coefficient(total_norm, max_norm, defect=None):
    """clip_grad_norm_'s coefficient in double for a FINITE norm; max_norm None: 1."""
    assert defect is None or defect in DEFECTS, defect
    if max_norm is None:
        return 1.0
    denom = total_norm + (0.0 if defect == "eps_dropped" else 1e-6)
    c = max_norm / denom if denom > 0 else math.inf
    return c if defect == "no_clamp" else min(1.0, c)


def clipped(g, c):
    """fl32(fl32(c) * g): what the guarded step uses in g's place, and what dvc_grad_scale leaves in .grad."""
    return g.detach().float() * torch.tensor(c, dtype=torch.float32, device=g.device)


def ulps(a, b):
    """|a - b| in fp32 units in the last place, for positive finite values."""
    a, b = np.float32(a), np.float32(b)
    assert a > 0 and b > 0 and np.isfinite(a) and np.isfinite(b), (a, b)
    return abs(int(a.view(np.int32)) - int(b.view(np.int32)))


def guarded_step(states, grads, cfgs, *, max_norm=None, skip_nonfinite=True, skipped=0, coef=None, defect=None):
    """One guarded step over all tensors.  states: list of dict(p, m, v, vmax, t) (fp32 tensors, int t); grads: list of tensors or
    None (that tensor sits out); cfgs: adam_reference.step's keyword arguments per tensor (lr, betas, eps, weight_decay, amsgrad).
    coef: use this coefficient (the device's own) in place of the restatement's.
    -> (new states — float64 p, m, v, vmax; the SAME dicts when skipped —, refs per tensor or None, info dict)."""
    assert defect is None or defect in DEFECTS, defect
    live = [g for g in grads if g is not None]
    s = sumsq(live)
    nonfinite = not math.isfinite(s)
    info = dict(sumsq=s, norm=norm(live), found_inf=int(nonfinite and skip_nonfinite), coef=1.0)
    info["skipped"] = skipped + info["found_inf"]
    if info["found_inf"]:
        out = [dict(st, t=st["t"] + 1) if (defect == "advance_on_skip" and g is not None) else st for st, g in zip(states, grads)]
        return out, [None] * len(states), info
    if not nonfinite:
        info["coef"] = coefficient(info["norm"], max_norm, defect)
    out, refs = [], []
    for st, g, cfg in zip(states, grads, cfgs):
        if g is None:
            out.append(st)
            refs.append(None)
            continue
        c = info["coef"] if coef is None else coef
        if defect == "per_tensor_norm" and not nonfinite:
            c = coefficient(norm([g]), max_norm)
        ref = A.step(st["p"], clipped(g, c), st["m"], st["v"], st["vmax"], t=st["t"] + 1, **cfg)
        out.append(dict(p=ref["p"], m=ref["m"], v=ref["v"], vmax=ref["vmax"] if ref["vmax"] is not None else st["vmax"], t=st["t"] + 1))
        refs.append(ref)
    return out, refs, info
