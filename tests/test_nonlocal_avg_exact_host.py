"""CPU side of NonlocalWeightedAverage's one-hot cases (tests/nlwa_exact_cases.py): the generator covers every allowed pair of
levels with stable ids, the integer ranges keep the kernel's arithmetic exact, the exact reference agrees with the float64
restatement (tests/nlwa_reference.py) at the same alpha, the generated set really holds every placement of the maxima it was
written for, and five deliberately wrong restatements each differ from the reference on a named case."""
import importlib
import itertools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import nlwa_exact_cases as X  # noqa: E402


def test_tile_constants_come_from_the_kernel_source():
    t = X.tile_constants()
    assert t == dict(NL_QB=128, NL_KT=128, NL_KC=32, NL_WG_TARGET=512)
    # the smallest size class with two tiles in one split, and the size with no ragged tile
    for N in (2880, 2944):
        pl = X.plan(N)
        assert (pl["ntiles"], pl["nqb"], pl["nsplit"]) == (23, 23, 22) and pl["ranges"][-1] == (21, 23)
    assert all(t1 - t0 == 1 for N in (1, 2, 127, 128, 129, 255, 256, 257, 2816) for t0, t1 in X.plan(N)["ranges"])
    assert X.plan(5184)["nsplit"] == 12                              # the benchmark map
    assert 2944 % t["NL_KT"] == 0 and 2880 % t["NL_KT"] == 64 and X.BIG_N == 2880
    assert {32, 33} <= set(X.CHANNELS) and t["NL_KC"] == 32


def test_generator_covers_every_allowed_pair():
    cases, impossible = X.generate()
    names = sorted(X.FACTORS)
    seen = {(a, c[a], b, c[b]) for c in cases for a, b in itertools.combinations(names, 2)}
    missing = {(a, va, b, vb) for a, b in itertools.combinations(names, 2) for va in X.FACTORS[a] for vb in X.FACTORS[b]
               if (a, va, b, vb) not in seen}
    assert len(missing) == len(impossible)
    # a pair no case holds is one the two rules forbid: a large map with C > 4 or a patch, a two-tile placement on a small map
    big = {s for s in X.SIZES if s[0] * s[1] >= X.BIG_N}
    assert big == {(45, 64), (46, 64)}
    for a, va, b, vb in missing:
        lv = {a: va, b: vb}
        assert (lv.get("size") in big and (lv.get("C", 1) > 4 or lv.get("k", 1) > 1)) or \
               (lv.get("place") in ("later_tile", "earlier_tile") and
                (lv.get("C", 1) > 4 or lv.get("k", 1) > 1 or ("size" in lv and lv["size"] not in big))), (a, va, b, vb)
    assert all(X._valid(c) for c in cases)
    # every size, patch, channel count, batch, resize and feature size runs
    for name in names:
        assert {c[name] for c in cases} == set(X.FACTORS[name]), name
    assert any(c["k"] > c["W"] for c in cases) and any(c["H"] == 1 and c["k"] == 7 for c in cases)
    assert all(c["C"] <= 4 and c["k"] == 1 for c in cases if c["N"] >= X.BIG_N)
    assert all(c["N"] <= 257 for c in cases if c["k"] == 7 or c["C"] == 65)


def test_ids_are_unique_and_stable():
    first = [dict(c) for c in X.exact_cases() + X.graded_cases()]
    ids = [c["id"] for c in first]
    assert len(ids) == len(set(ids))
    again = importlib.reload(X)                                      # drops the caches: the generator runs a second time
    assert again.exact_cases() + again.graded_cases() == first
    a, b = again.make_inputs(first[3]), X.make_inputs(first[3])
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_graded_list_is_a_dozen_of_the_same_geometries():
    g, e = X.graded_cases(), X.exact_cases()
    assert 10 <= len(g) <= 14
    geo = lambda c: (c["size"], c["k"], c["C"], c["B"], c["sf"], c["fsize"])        # noqa: E731
    assert {geo(c) for c in g} <= {geo(c) for c in e}
    assert {2880, 2944, 1} <= {c["N"] for c in g} and {5, 7} <= {c["k"] for c in g} and {32, 33, 65} <= {c["C"] for c in g}
    assert all(c["alpha"] == X.ALPHA_GRADED for c in g)
    assert np.float32(X.LOG2E / X.ALPHA_GRADED) == np.float32(1.0)
    # the weights are graded: the second-largest affinity of a typical row is within a few units of the largest
    c = next(c for c in g if c["N"] == 257)
    x, f = X.make_inputs(c)
    _, U = X.resized(c, x, f)
    A = np.sort(U[0].T @ U[0], axis=1)
    assert np.median(A[:, -1] - A[:, -2]) <= 3


def test_exactness_guard_holds_for_every_case():
    """K max|f|^2 < 2^24 (every affinity, and every partial sum of one in any order, is an fp32 integer) and N max|ab| < 2^24
    (so is every sum of ab values); integer data throughout; non-maximal keys at least 1 below the maximum weigh exactly 0."""
    worst = (0.0, 0.0)
    for c in X.exact_cases() + X.graded_cases():
        x, f = X.make_inputs(c)
        assert torch.equal(x, x.round()) and torch.equal(f, f.round())
        assert x.abs().max() <= X.AB_MAX and f.abs().max() <= X.F_MAX
        ga, gs = X.exactness_guard(c, f)
        worst = (max(worst[0], ga), max(worst[1], gs))
    assert worst[0] < 2 ** 24 / 16 and worst[1] < 2 ** 24 / 16, worst       # four bits to spare
    c_exact = np.float32(min(X.LOG2E / X.ALPHA_EXACT, np.finfo(np.float32).max))
    assert 369 < c_exact < 370 and -1.0 * c_exact < -149                      # exp2 of it is below the smallest denormal


@pytest.mark.parametrize("c", X.exact_cases(), ids=lambda c: c["id"])
def test_exact_reference_equals_float64_restatement(c):
    """At alpha = 2^-8 the softmax of the restatement is the one-hot mean up to exp(-256): its own accuracy."""
    x, f, want, count, _ = X.solved(c)
    ref = X.float64_restatement(c, x, f)
    assert tuple(ref.shape) == tuple(want.shape) == (c["B"], 2, c["H"], c["W"])
    assert (want.double() - ref).abs().max().item() <= 1e-9 + 2.0 ** -24 * X.AB_MAX        # float32 rounding of the quotient
    assert count.min() >= 1 and count.max() <= c["N"]


def test_resize_indices_are_atens():
    import torch.nn.functional as F
    for c in X.exact_cases():
        x, f = X.make_inputs(c)
        iy, ix, fy, fx = X.resize_indices(c)
        xr, fr = X.R.resize(x, f, c["sf"])
        assert torch.equal(xr, x[:, :, torch.from_numpy(iy)][:, :, :, torch.from_numpy(ix)]), c["id"]
        assert torch.equal(fr, f[:, :, torch.from_numpy(fy)][:, :, :, torch.from_numpy(fx)]), c["id"]
        assert tuple(F.interpolate(x, scale_factor=c["sf"]).shape[2:]) == (c["H"], c["W"])
    sizes = {(np.sign(c["H"] * c["W"] - X._f_in(c["H"], c["fsize"]) * X._f_in(c["W"], c["fsize"]))) for c in X.exact_cases()}
    assert sizes == {-1, 0, 1}                                       # the feature larger than, equal to, smaller than the map


def test_placement_inventory_is_complete():
    found, by_size, ulp_cases = {}, {}, []
    for c in X.exact_cases():
        _, _, _, count, tags = X.solved(c)
        for t in tags:
            found.setdefault(t, c["id"])
            by_size.setdefault((t, c["N"]), c["id"])
        if not X.is_pow2(count).all():
            ulp_cases.append(c["id"])
    print({t: found.get(t) for t in X.INVENTORY}, {k: v for k, v in by_size.items() if k[0] in X.INVENTORY_BIG})
    assert not [t for t in X.INVENTORY if t not in found]
    assert not [(t, N) for t in X.INVENTORY_BIG for N in (2880, 2944) if (t, N) not in by_size]
    # the constant feature with patch 1: every key maximal, the output the plain mean of ab
    c = next(c for c in X.exact_cases() if c["place"] == "const" and c["k"] == 1 and c["N"] > 1)
    x, f, want, count, tags = X.solved(c)
    assert "all_keys_maximal" in tags
    ab, _ = X.resized(c, x, f)
    assert np.allclose(want.double().numpy().reshape(c["B"], 2, -1), ab.mean(axis=2, keepdims=True), rtol=2.0 ** -23, atol=0)
    # the 1-ulp rule judges a minority of the cases
    n = len(X.exact_cases())
    print(f"{n} exact cases, {len(ulp_cases)} with a count that is no power of two, {len(X.graded_cases())} graded")
    assert 0 < len(ulp_cases) < n / 2, (len(ulp_cases), n)


@pytest.mark.parametrize("mutation", X.MUTATIONS)
def test_wrong_restatement_is_seen(mutation):
    """Each wrong restatement fails the acceptance rule on a generated case; the assertion message of a miss names none."""
    seen = []
    for c in X.exact_cases():
        x, f, _, _, _ = X.solved(c)
        wrong, _ = X.exact_reference(c, x, f, mutate=mutation)
        msg = X.judge(c, wrong)
        if msg is not None:
            seen.append(c["id"])
            first = first if len(seen) > 1 else msg
    print(f"{mutation}: seen by {len(seen)} of {len(X.exact_cases())} cases, first {seen[:1]}")
    assert seen, mutation
    assert seen[0] in first and "(b, channel, y, x)" in first and "maximal keys" in first


def test_judge_rule():
    """Bit-equal where the count is a power of two, 1 ulp where it is not, nothing for a NaN."""
    c = next(c for c in X.exact_cases() if c["place"] == "tie3" and (X.solved(c)[3][0] == 3).any() and (X.solved(c)[3][0] == 1).any())
    x, f, want, count, _ = X.solved(c)
    assert X.judge(c, want) is None
    flat = want.clone().view(c["B"], 2, -1)
    q3 = int(np.flatnonzero(count[0] == 3)[0])
    q1 = int(np.flatnonzero(X.is_pow2(count[0]))[0])
    up = lambda v: torch.nextafter(v, torch.tensor(float("inf")))     # noqa: E731
    t = flat.clone()
    t[0, 0, q3] = up(t[0, 0, q3])
    assert X.judge(c, t.view_as(want)) is None
    t[0, 0, q3] = up(t[0, 0, q3])
    assert X.judge(c, t.view_as(want)) is not None
    t = flat.clone()
    t[0, 1, q1] = up(t[0, 1, q1])
    assert "(b, channel, y, x) = (0, 1," in X.judge(c, t.view_as(want))
    t = flat.clone()
    t[0, 0, q3] = float("nan")
    assert X.judge(c, t.view_as(want)) is not None
