"""CPU side of the bit-exact convolution sweep (tests/conv_exact_cases.py): the case generator covers every allowed pair of
factor levels with stable ids; the integer ranges keep every engine's arithmetic exact (the guard, and float32 restatements of
the direct sum and of Winograd F(2x2,3x3) that equal the float64 reference bit for bit); the library plans every Winograd case
(host-only dvc_conv2d_winograd_split), so the share of refused plans is known before any GPU run; and a restatement with one
wrong index fails the same equality assertion at the coordinate of the defect."""
import ctypes
import importlib
import itertools

import pytest
import torch

import conv_exact_cases as C

SINGLE = ("direct", "streamk", "image", "ws", "wino", "wino_pool", "per_image")


@pytest.mark.parametrize("engine", C.ENGINES)
def test_generator_covers_every_allowed_pair(engine):
    cases, impossible = C.generate(engine)
    f = C.factors(engine)
    names = sorted(f)
    seen = {(a, c[a], b, c[b]) for c in cases for a, b in itertools.combinations(names, 2)}
    missing = [(a, va, b, vb) for a, b in itertools.combinations(names, 2) for va in f[a] for vb in f[b] if (a, va, b, vb) not in seen]
    assert len(missing) == len(impossible)
    # a pair no case holds is one no valid case CAN hold (an independent search of 3000 completions finds none)
    for a, va, b, vb in missing:
        assert not C.pair_allowed(engine, a, va, b, vb), (engine, a, va, b, vb)
    assert all(C._VALID[engine](c) for c in cases)


def test_pairs_the_rules_forbid_and_pairs_the_suite_never_ran():
    direct, wino = C.cases("direct"), C.cases("wino")
    has = lambda cs, **kv: any(all(c[k] == v for k, v in kv.items()) for c in cs)      # noqa: E731
    assert not has(direct, ks=1, stride=2) and not has(direct, ks=1, dil=2)
    assert not has(wino, Cout=192, cfg=0) and not has(wino, Cin=8, split_k=2) and not has(wino, defer=True, res=True)
    assert not any(c["pad_mode"] == 1 and c["dil"] == 2 and min(C.vdim(c["H"], *C.RESAMPLE[c["resample"]]),
                                                                 C.vdim(c["W"], *C.RESAMPLE[c["resample"]])) <= 2 for c in wino)
    # the combinations the sweep was written for
    assert any(c["resample"] == "1/2" and c["H"] % 2 and c["W"] % 2 for c in wino)                 # in_sub = 2 on odd H and W
    assert has(wino, pad_mode=1, resample="2/1") and has(wino, pad_mode=1, N=3)
    assert any(c["H"] <= 3 and c["W"] <= 3 and c["res"] and c["dst"] == "slice" for c in wino)      # below one tile block
    assert any(c["Cout"] == 192 and c["cfg"] >= 4 for c in wino)
    assert any(c["Cin"] == 40 and c["split_k"] > 1 for c in wino) and any(c["Cin"] == 40 and c["split_k"] > 1 for c in direct)
    assert has(direct, stride=2, pad_mode=1, N=3) and has(direct, stride=2, pad_mode=1, res=True)


def test_ids_are_unique_and_stable():
    first = [{k: v for k, v in c.items()} for e in C.ENGINES for c in C.cases(e)]
    ids = [c["id"] for c in first]
    assert len(ids) == len(set(ids))
    again = importlib.reload(C)          # drops the caches: the generator runs a second time
    assert [c for e in again.ENGINES for c in again.cases(e)] == first


def test_tile_edges_come_from_the_kernel_sources():
    t = C.tile_tables()
    assert len(t["cfgs"]) == 5 and len(t["wino"]) == 4 and t["tws"] == sorted(t["tws"]) and t["sk_cfgs"] == [2, 3, 4]
    for engine in C.ENGINES:
        Hs, Ws = C.geometry_levels(engine)
        assert max(Hs) <= C.MAX_H and max(Ws) <= C.MAX_W
    Hs, Ws = C.geometry_levels("wino")
    for tr in t["ktr"]:
        for (_wm, wn, _kc, _) in t["wino"]:
            e = 2 * tr * wn
            assert e > C.MAX_H or {e - 1, e, e + 1} <= set(Hs)
        assert {2 * (32 // tr) - 1, 2 * (32 // tr), 2 * (32 // tr) + 1} <= set(Ws)


@pytest.mark.parametrize("engine", C.ENGINES)
def test_exactness_guard_holds_for_every_case(engine):
    """sum |x'| |w'| / q < 2^24 with room: a violation is a bug of the generator's ranges, never a skip."""
    worst = max(C.exactness_bound(c) for c in C.cases(engine))
    assert worst < 2 ** 24 / 16, (engine, worst)            # more than four bits to spare


def _refs(engine):
    for c in C.cases(engine):
        t = C.make_inputs(c)
        yield c, t, C.reference(c, t)


@pytest.mark.parametrize("engine", ["direct", "streamk", "image", "ws", "per_image"])
def test_float32_direct_sum_equals_float64_bit_for_bit(engine):
    for c, t, ref in _refs(engine):
        args = lambda w, n=slice(None): (t["x"][n], w, t["b"], *t["geom"], t["scale"], t["shift"], t["slope"],      # noqa: E731
                                         None if t["res"] is None else t["res"][n], t["act"], t["act_slope"])
        if engine == "per_image":
            taps = torch.cat([C.direct_taps(*args(t["w"][n], slice(n, n + 1))) for n in range(c["N"])])
            aten = torch.cat([C.direct_conv2d(*args(t["w"][n], slice(n, n + 1))) for n in range(c["N"])])
        else:
            taps, aten = C.direct_taps(*args(t["w"])), C.direct_conv2d(*args(t["w"]))
        assert taps.dtype == aten.dtype == torch.float32
        C.assert_exact(taps, ref, c["id"] + " (float32 tap loop)")
        C.assert_exact(aten, ref, c["id"] + " (float32 conv2d)")


@pytest.mark.parametrize("engine", ["wino", "wino_pool"])
def test_float32_winograd_equals_float64_bit_for_bit(engine):
    """U = G g G^T, V = B^T d B, the product summed over Cin and A^T m A, all in float32, with the dilation-2 parity split and
    the up / sub views, on the generator's own inputs: equal to the float64 DIRECT reference.  So on the GPU an unequal element
    is the kernel's, not the data's."""
    for c, t, ref in _refs(engine):
        ks, stride, dil, pad, pad_mode, up, sub = t["geom"]
        y = C.winograd(t["x"], t["w"], t["b"], dil, pad_mode, up, sub, t["res"], t["act"], t["act_slope"])
        assert y.dtype == torch.float32
        if engine == "wino_pool":
            C.assert_exact(torch.nn.functional.max_pool2d(y, 2, 2), ref[1], c["id"] + " (pooled)")
            ref = ref[0]
        C.assert_exact(y, ref, c["id"])


def test_float32_winograd_dual_and_group_equal_float64():
    for c in C.cases("wino_dual"):
        t = C.make_dual(c)
        yB = C.winograd(t["xB"], t["wB"], t["bB"], c["dil"], c["pad_mode"], c["upB"], 1, None, 0, 0.0)
        y = C.winograd(t["xA"], t["wA"], t["bA"], c["dil"], c["pad_mode"], c["upA"], 1, yB, t["act"], t["act_slope"])
        C.assert_exact(y, C.ref_dual(c, t), c["id"])
    for c in C.cases("wino_group"):
        items = C.make_group(c)
        a, s = C.ACTS[c["act"]]
        for k, (i, ref) in enumerate(zip(items, C.ref_group(c, items))):
            C.assert_exact(C.winograd(i["x"], i["w"], i["b"], 1, c["pad_mode"], i["up"], 1, None, a, s), ref, f"{c['id']} item {k}")


def _desc(c, **kw):
    from dvc_amd import ops
    Cin, Cout = c["Cin"], c["Cout"]
    up, sub = C.RESAMPLE[c.get("resample", "1/1")]
    return ops._conv_desc(c["N"], Cin, c["H"], c["W"], Cout, dil=c.get("dil", 1), pad_mode=c.get("pad_mode", 0), in_up=up, in_sub=sub,
                          cfg=c.get("cfg", -1), split_k=c.get("split_k", 0), **kw)


def test_the_library_plans_every_winograd_case():
    """dvc_conv2d_winograd_split (host only) on every Winograd case: none is refused, so the Winograd share of skipped cases is
    zero before any GPU run; a forced split is the split the launch uses; and the deferred-reduce cases include split layers."""
    from dvc_amd import _lib, ops
    lib = _lib.load()
    refused, deferred_split = [], 0
    for c in C.cases("wino") + C.cases("wino_pool"):
        sp, ipl = ctypes.c_int32(0), ctypes.c_int32(0)
        if lib.dvc_conv2d_winograd_split(ctypes.byref(_desc(c)), ops.CONV_WORKSPACE_BYTES, ctypes.byref(sp), ctypes.byref(ipl)) != 0:
            refused.append((c["id"], lib.dvc_last_error()))
            continue
        assert ipl.value >= c["N"], c["id"]
        if c.get("split_k", 0) >= 1:
            assert sp.value == c["split_k"], (c["id"], sp.value)
        deferred_split += bool(c.get("defer") and sp.value > 1)
    assert not refused, refused
    assert deferred_split >= 10, deferred_split


def test_forced_plans_the_generator_leaves_out_are_refused_by_the_library():
    """The generator's plan rule is the library's: what wino_plan_exists rejects, dvc_conv2d_winograd_split refuses."""
    from dvc_amd import _lib, ops
    lib = _lib.load()
    f = C.factors("wino")
    for Cin, Cout, cfg, split_k in itertools.product(f["Cin"], f["Cout"], f["cfg"], f["split_k"]):
        c = dict(N=1, Cin=Cin, Cout=Cout, H=9, W=16, cfg=cfg, split_k=split_k)
        sp, ipl = ctypes.c_int32(0), ctypes.c_int32(0)
        rc = lib.dvc_conv2d_winograd_split(ctypes.byref(_desc(c)), ops.CONV_WORKSPACE_BYTES, ctypes.byref(sp), ctypes.byref(ipl))
        assert (rc == 0) == C.wino_plan_exists(Cin, Cout, cfg, split_k), (Cin, Cout, cfg, split_k, lib.dvc_last_error())


# ---- sensitivity: the equality assertion finds one wrong index, at its coordinate
def _first(msg):
    return tuple(int(v) for v in msg.split("(n, c, y, x) = (")[1].split(")")[0].split(","))


def test_a_wrong_reflect_row_in_the_winograd_restatement_is_caught_at_the_bottom_edge():
    c = next(c for c in C.cases("wino") if c["pad_mode"] == 1 and c["dil"] == 1 and c["resample"] == "1/1" and c["H"] >= 7 and c["W"] >= 7)
    t = C.make_inputs(c)
    ref = C.reference(c, t)

    def wrong(p, V, pad_mode, axis):      # below the image the mirror is taken about the last row's lower edge, not its centre
        return V - 1 if (axis == "y" and p >= V) else C.map_virtual(p, V, pad_mode, axis)
    ks, stride, dil, pad, pad_mode, up, sub = t["geom"]
    y = C.winograd(t["x"], t["w"], t["b"], dil, pad_mode, up, sub, t["res"], t["act"], t["act_slope"], index_map=wrong)
    with pytest.raises(AssertionError) as e:
        C.assert_exact(y, ref, c["id"])
    assert c["id"] in str(e.value) and _first(str(e.value))[2] == t["OH"] - 1
    assert (y[:, :, :-1] == ref[:, :, :-1].float()).all()          # every other row is right: the defect is local


def test_a_tap_from_the_neighbouring_column_in_the_direct_restatement_is_caught_at_that_column():
    c = next(c for c in C.cases("direct") if c["ks"] == 3 and c["stride"] == 1 and c["resample"] == "1/1" and c["W"] >= 15 and c["H"] >= 3)
    t = C.make_inputs(c)
    ref = C.reference(c, t)
    args = (t["x"], t["w"], t["b"], *t["geom"], t["scale"], t["shift"], t["slope"], t["res"], t["act"], t["act_slope"])
    C.assert_exact(C.direct_taps(*args), ref, c["id"])
    y = C.direct_taps(*args, wrong_tap=(0, 0, 8))                  # the outputs of column 8 (a tile seam) read tap (0, 0) one column off
    with pytest.raises(AssertionError) as e:
        C.assert_exact(y, ref, c["id"])
    assert _first(str(e.value))[3] == 8
    keep = [x for x in range(t["OW"]) if x != 8]
    assert (y[..., keep] == ref[..., keep].float()).all()
