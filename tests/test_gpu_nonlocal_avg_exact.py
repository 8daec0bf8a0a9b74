"""GPU: NonlocalWeightedAverage (dvc_nlwa_fwd, csrc/nonlocal_avg.hip) on the one-hot cases of tests/nlwa_exact_cases.py.

Exact regime (integer features and ab, alpha = 2^-8): the output is float32(sum of ab over the maximal keys) / float32(count),
bit for bit where the count is a power of two and within 1 ulp otherwise; the maximal keys come from the float64 reference.
Graded regime (alpha = float32(log2 e), the kernel's constant exactly 1.0f): the rule of test_matches_float64_restatement,
4 x the error of the float32 CPU restatement + 1e-6 max|ref|.  Every case runs twice (identical bits) and, for B > 1, image by
image (each image equals its own B = 1 call bit for bit).
"""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import nlwa_exact_cases as X  # noqa: E402

pytestmark = pytest.mark.gpu


def _run(c, x, f):
    from dvc_amd.nonlocal_avg import nonlocal_weighted_average
    with torch.no_grad():
        out = nonlocal_weighted_average(x, f, c["k"], c["alpha"], c["sf"])
    torch.cuda.synchronize()
    return out


def _repeat_and_split(c, x, f, full):
    again = _run(c, x, f)
    assert torch.equal(full, again), (c["id"], "the second run differs")
    if c["B"] > 1:
        for b in range(c["B"]):
            one = _run(c, x[b:b + 1].contiguous(), f[b:b + 1].contiguous())
            assert torch.equal(one, full[b:b + 1]), (c["id"], f"image {b} differs from its own B = 1 call")


@pytest.mark.parametrize("c", X.exact_cases(), ids=lambda c: c["id"])
def test_one_hot_case_is_exact(c):
    x, f, want, count, _ = X.solved(c)
    xd, fd = x.cuda(), f.cuda()
    full = _run(c, xd, fd)
    msg = X.judge(c, full)
    assert msg is None, msg
    _repeat_and_split(c, xd, fd, full)


@pytest.mark.parametrize("c", X.graded_cases(), ids=lambda c: c["id"])
def test_graded_case_matches_float64_restatement(c):
    x, f = X.make_inputs(c)
    xd, fd = x.cuda(), f.cuda()
    full = _run(c, xd, fd)
    got = full.cpu().double()
    ref64 = X.float64_restatement(c, x, f)
    ref32 = X.float64_restatement(c, x, f, dtype=torch.float32).double()
    assert got.shape == ref64.shape
    err, err32 = (got - ref64).abs().max().item(), (ref32 - ref64).abs().max().item()
    tol = 4 * err32 + 1e-6 * ref64.abs().max().item()
    print(f"{c['id']}: max-abs err {err:.3e}, fp32 CPU restatement {err32:.3e}, bound {tol:.3e}, err / bound {err / tol if tol else 0.0:.3f}")
    assert torch.isfinite(got).all()
    assert err <= tol, (c["id"], err, err32)
    _repeat_and_split(c, xd, fd, full)
