"""CPU-side checks of tests/instnorm_cases.py: the generators cover their pairs with stable ids, the probe data are exact, the
float32 restatement of the partial sums is what it claims, the bound holds for a correct implementation on every graded case,
and every seeded wrong restatement is seen by at least one case (a sweep that cannot tell them apart pins nothing)."""
import itertools

import numpy as np
import pytest

import instnorm_cases as IC


def _graded_cases():
    return [c for e in IC.ENTRIES for c in IC.cases(e)]


@pytest.fixture(scope="module")
def graded():
    """(case, data, reference) of every graded case, computed once."""
    out = []
    for c in _graded_cases():
        t = IC.make_data(c)
        out.append((c, t, IC.reference(t["x"], second=IC.second_of(c, t), **IC.ref_args(c, t))))
    return out


# ---- generators
def test_constants_and_plane_levels_follow_the_source():
    assert IC.K == dict(VT=1024, B1024=32768, B512=8192, PBLOCK=4096, LDS=16384, SMAX=8, GMAX=4, FLY=12288, PIECES=4)
    assert [h * w for h, w in IC.PLANES] == [1, 3, 15, 1215, 4096, 4097, 8190, 8192, 12288, 12292, 16384, 16388, 32761, 32768, 32772]
    assert IC.PLANE_OVER_LDS == (68, 241) and max(h * w for h, w in IC.PLANES_PARTIALS) == 16384


@pytest.mark.parametrize("entry", IC.ENTRIES)
def test_every_pair_of_levels_is_in_a_case(entry):
    cases, impossible = IC.generate(entry)
    f = IC.factors(entry)
    names = sorted(f)
    held = {(a, c[a], b, c[b]) for c in cases for a, b in itertools.combinations(names, 2)}
    missing = [(a, va, b, vb) for a, b in itertools.combinations(names, 2) for va in f[a] for vb in f[b]
               if (a, va, b, vb) not in held]
    # a pair may be missing only where no valid case can hold it: one of its levels belongs to a factor the other's mode switches
    # off (rlay without a residual, slope without an activation), in place with a second output or another layout of y, or more
    # than 5 planes of the largest sizes
    for a, va, b, vb in missing:
        assert not _some_valid(f, names, {a: va, b: vb}), (entry, a, va, b, vb)
    assert len(missing) == len(impossible)
    ids = [c["id"] for c in cases]
    assert len(set(ids)) == len(ids)
    assert IC.generate.__wrapped__(entry)[0] == cases                 # the same list when generated again
    print(f"{entry}: {len(cases)} cases, {len(missing)} pairs no valid case holds")


def _some_valid(f, names, fixed):
    """Independent of the generator's own search: a valid case with these two levels, by exhaustion over the factors _valid reads."""
    reads = [n for n in ("mode", "second", "xlay", "ylay", "rlay", "slope", "plane", "N", "C") if n in f and n not in fixed]
    base = {n: f[n][0] for n in names}
    base.update(fixed)
    levels = dict(f, plane=[f["plane"][0], f["plane"][-1]])           # _valid reads the plane only as "one of the largest"
    return any(IC._valid(dict(base, **dict(zip(reads, combo)))) for combo in itertools.product(*[levels[n] for n in reads]))


def test_group_cases_cover_what_the_issue_lists():
    groups = IC.group_cases()
    thr = IC.K["PBLOCK"]
    sizes = {len(g["items"]) for g in groups}
    assert sizes == {1, 2, 3, 4}
    kinds = lambda g: {c["entry"] for c in g["items"]}                                                     # noqa: E731
    assert any(all(c["HW"] < thr for c in g["items"]) and len(g["items"]) > 1 for g in groups)
    assert any(any(c["HW"] >= thr for c in g["items"]) and any(c["HW"] < IC.K["B512"] and c["entry"] == "apply" for c in g["items"])
               for g in groups)
    assert any(kinds(g) == {"apply", "partials"} for g in groups)
    names = [g["name"] for g in groups]
    assert all(names.count(g["name"]) == 2 for g in groups if len(g["items"]) > 1)
    assert all(len(g["items"]) <= IC.K["GMAX"] and all(c["second"] == "none" for c in g["items"]) for g in groups)
    print(f"group: {len(groups)} cases")


# ---- probe regime
@pytest.mark.parametrize("plane", IC.PLANES, ids=lambda p: "%dx%d" % p)
def test_probe_planes_are_exact_in_double(plane):
    H, W = plane
    HW = H * W
    pos = IC.probe_positions(HW)
    assert {0, HW - 1} <= set(pos) and all(0 <= p < HW for p in pos)
    for want in (HW & ~3, (HW & ~3) - 1, IC.K["FLY"], 4 * IC.VT, 16 * IC.VT + 1):
        assert (want in pos) == (0 <= want < HW)
    for two in (False, True):
        x = IC.probe_tensor(H, W, two)
        assert IC.exact_in_double(x)
        assert ((x != 0).reshape(len(pos), -1).sum(1) == (2 if two and len(pos) > 1 else 1)).all()
        # the double sums in two different orders, and the 60-digit statistics against a plain float64 evaluation
        f = x.reshape(len(pos), HW).astype(np.float64)
        assert (f.sum(1) == f[:, ::-1].cumsum(1)[:, -1]).all()
        sc, sh = IC.probe_stats(x)
        for c in range(len(pos)):
            rstd, shift = IC.model_stats(x.ravel(), c * HW, HW)
            assert IC.ulps(np.float32(rstd), sc[0, c]) <= 1 and IC.ulps(np.float32(shift), sh[0, c]) <= 1
    if HW <= IC.K["LDS"]:
        for S, act in ((1, IC.ACTS["none"]), (3, IC.ACTS["prelu_ptr"]), (IC.K["SMAX"], (IC.ACT_LEAKY, 0.5, None))):
            part, bias = IC.probe_partials(H, W, S, HW + S)
            x = IC.restate_partials(part, bias, act)
            assert IC.exact_in_double(x) and np.abs(x).max() >= IC.PROBE - 4 * S - 3
            # the float32 restatement IS the expression: evaluated in float64 it gives the same bits
            assert np.array_equal(x, IC.restate_partials(part, bias, act, dtype=np.float64).astype(np.float32))


# ---- the bound
def test_a_correct_implementation_stays_inside_the_bound(graded):
    worst = {}
    for c, t, ref in graded:
        got = IC.emulate(t["x"], **IC.ref_args(c, t))
        assert got.shape == ref["y"].shape, c["id"]
        assert IC.first_wrong(got, ref["y"], ref["bound"]) is None, c["id"]
        worst[c["entry"]] = max(worst.get(c["entry"], 0.0), IC.worst_ratio(got, ref["y"], ref["bound"]))
        if "y2" in ref:
            sub2, cs2 = IC.second_of(c, t)
            got2 = IC.emulate(t["x"], sub=sub2, cs=cs2)
            assert IC.first_wrong(got2, ref["y2"], ref["bound2"]) is None, c["id"]
    print("error of the emulated fused form / bound, worst per entry:", {k: round(v, 3) for k, v in worst.items()})
    assert all(0.01 < v <= 1.0 for v in worst.values())           # inside, and the bound is not orders of magnitude too wide


# ---- seeded wrong restatements
def _seen_by_value(graded, bug, pick=lambda c: True):
    """Ids of the graded cases whose float64 reference moves by more than the bound (or changes shape) under the defect."""
    seen = []
    for c, t, ref in graded:
        if not pick(c):
            continue
        wrong = IC.reference(t["x"], second=IC.second_of(c, t), bug=bug, **IC.ref_args(c, t))
        for k, b in (("y", "bound"), ("y2", "bound2")):
            if k in ref and (wrong[k].shape != ref[k].shape or IC.first_wrong(wrong[k].astype(np.float32), ref[k], ref[b]) is not None):
                seen.append(c["id"])
                break
    return seen


@pytest.mark.parametrize("bug, pick", [
    ("sub_floor", lambda c: c["mode"] == "cs_sub2" or c.get("second") == "s2cs"),
    ("rpad_off_by_one", lambda c: IC.mode_params(c["mode"])["rpad"] > 0),
    ("up_ceil", lambda c: IC.mode_params(c["mode"])["up"] > 1),
    ("y2_chan_scale", lambda c: c.get("second", "none") != "none"),
    ("unbiased", lambda c: c["HW"] <= 1215),
], ids=lambda v: v if isinstance(v, str) else "")
def test_wrong_index_maps_and_statistics_are_seen(graded, bug, pick):
    seen = _seen_by_value(graded, bug, pick)
    print(f"{bug}: seen by {len(seen)} cases, first {seen[:1]}")
    assert seen


def test_wrong_partial_sums_are_seen():
    after, reverse = [], []
    for c in IC.cases("partials"):
        t = IC.make_data(c)
        ref = IC.reference(t["x"], **IC.ref_args(c, t))
        xb = IC.restate_partials(t["part"], t["bias"], t["act"], bug="bias_after_act")
        wb = IC.reference(xb, **IC.ref_args(c, t))
        if IC.first_wrong(wb["y"].astype(np.float32), ref["y"], ref["bound"]) is not None:
            after.append(c["id"])
        # the order of the slices moves last bits only: what sees it is check 4's bit equality, which holds where HW % 4 == 0
        if c["HW"] % 4 == 0 and not np.array_equal(t["x"], IC.restate_partials(t["part"], t["bias"], t["act"], bug="reverse_slices")):
            reverse.append(c["id"])
    print(f"bias_after_act: seen by {len(after)} cases; reverse_slices: by {len(reverse)} cases")
    assert after and reverse


@pytest.mark.parametrize("bug", ["drop_tail", "drop_fly", "neighbour"])
def test_wrong_summation_paths_are_seen_by_the_probes(bug):
    """The probe tensors as the GPU module lays them out: [1][P][H][W] from an aligned base and from one float past it."""
    seen = []
    for H, W in IC.PLANES:
        HW = H * W
        for two, base in itertools.product((False, True), (0, 1)):
            x = IC.probe_tensor(H, W, two)
            flat = np.concatenate([np.zeros(base, np.float32), x.ravel(), np.zeros(4, np.float32)])
            sc, sh = IC.probe_stats(x)
            for c in range(x.shape[1]):
                rstd, shift = IC.model_stats(flat, base + c * HW, HW, bug)
                if IC.ulps(np.float32(rstd), sc[0, c]) > 1 or IC.ulps(np.float32(shift), sh[0, c]) > 1:
                    seen.append(("%dx%d" % (H, W), two, base, c))
    print(f"{bug}: seen at {len(seen)} probe planes, first {seen[:1]}")
    assert seen
    if bug == "drop_fly":
        assert {s[0] for s in seen} == {"%dx%d" % p for p in IC.PLANES if (p[0] * p[1] & ~3) > IC.K["FLY"]}
