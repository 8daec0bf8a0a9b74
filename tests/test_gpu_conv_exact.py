"""GPU: every forward convolution engine on integer data (tests/conv_exact_cases.py) must EQUAL the float64 reference, bit
for bit — the general direct kernel and its stride-2 / dilated variant, stream-K, the image-input kernel, conv_ws, the Winograd
family (plain, _pool, _dual, grouped, deferred reduce) and per-image filters.  Per case: equality with the first wrong
(n, c, y, x) on failure; a second run into a destination refilled with a sentinel equals the first (every element written,
deterministic); the canary channels around a sliced destination stay untouched.  tests/test_conv_exact_host.py shows on the CPU
that the data keep fp32 exact in any summation order, so an unequal element here is the kernel's."""
import ctypes

import pytest
import torch

import conv_exact_cases as C
from cabi_helpers import NAN, check as _check, lib, ops, ptr as _p  # noqa: F401  (ops, lib: fixtures)
from test_gpu_ops import report

pytestmark = pytest.mark.gpu
CANARY, SENTINEL = 3.0, -7.0
TALLY = {e: dict(run=0, skipped=0) for e in C.ENGINES}


def _cu(t):
    return None if t is None else t.cuda()


def _params(engine):
    return pytest.mark.parametrize("case", C.cases(engine), ids=[c["id"] for c in C.cases(engine)])


def _place_x(x, strided):
    """(device view, batch stride in elements): dense, or channels [8 : 8 + C] of a NaN-filled wider tensor."""
    if not strided:
        return x.cuda(), 0
    N, Cc, H, W = x.shape
    big = torch.full((N, Cc + 16, H, W), NAN, device="cuda")
    big[:, 8:8 + Cc] = x.cuda()
    return big[:, 8:8 + Cc], (Cc + 16) * H * W


def _destination(c, shape):
    """(whole tensor, the view the engine writes, batch stride in elements)"""
    N, Co, OH, OW = shape
    if c.get("dst", "dense") == "slice":
        big = torch.full((N, Co + 16, OH, OW), CANARY, device="cuda")
        return big, big[:, 8:8 + Co], (Co + 16) * OH * OW
    y = torch.full(shape, SENTINEL, device="cuda")
    return y, y, 0


def _workspace(ops):
    ws = ops._workspace(torch.device("cuda", torch.cuda.current_device()), ops.CONV_WORKSPACE_BYTES, "conv")
    return ctypes.c_void_p(ws.data_ptr()), ws.numel()


def _guarded(c, call):
    """Run `call`; a planning refusal of an explicitly forced plan is a skip, anything else (and any refusal of the automatic
    plan) is the failure it is."""
    forced = c.get("cfg", -1) >= 0 or c.get("split_k", 0) > 1
    try:
        return call()
    except RuntimeError as e:
        if forced and any(m in str(e) for m in C.REFUSALS):
            TALLY[c["engine"]]["skipped"] += 1
            report(f"conv exact {c['id']}: skipped, {e}")
            pytest.skip(str(e))
        raise


def _twice(c, shape, ref, launch):
    """launch(view, batch stride) into a fresh destination; equality with the reference; again into the refilled destination;
    canaries.  Returns the first result."""
    whole, view, bs = _destination(c, shape)
    _guarded(c, lambda: launch(view, bs))
    torch.cuda.synchronize()
    first = view.clone()
    C.assert_exact(first, ref, c["id"])
    view.fill_(SENTINEL)
    launch(view, bs)
    torch.cuda.synchronize()
    C.assert_exact(view, first, c["id"] + " (second run into a refilled destination)")
    if c.get("dst", "dense") == "slice":
        Co = shape[1]
        assert (whole[:, :8] == CANARY).all() and (whole[:, 8 + Co:] == CANARY).all(), c["id"] + ": canary channels written"
    TALLY[c["engine"]]["run"] += 1
    report(f"conv exact {c['id']}: equal to float64 in all {first.numel()} elements")
    return first


def _conv2d_case(ops, lib, c):
    """direct, streamk, image, per_image: dvc_conv2d through ops.conv2d, or the C-ABI where the input is a batch-strided slice."""
    t = C.make_inputs(c)
    ref = C.reference(c, t)
    ks, stride, dil, pad, pad_mode, up, sub = t["geom"]
    cfg, split_k = c.get("cfg", -1), c.get("per_cu", c.get("split_k", 0))
    xv, xbs = _place_x(t["x"], c.get("xin") == "strided")
    if c["engine"] == "per_image":
        wp = torch.stack([ops.pack_conv_weight(t["w"][n].cuda()) for n in range(c["N"])]).contiguous()
    else:
        wp = ops.pack_conv_weight(t["w"].cuda())
    b, res, sc, sh, sl = _cu(t["b"]), _cu(t["res"]), _cu(t["scale"]), _cu(t["shift"]), _cu(t["slope"])
    slope_t = torch.tensor([t["act_slope"]], device="cuda") if t["act"] == 2 else None
    wsp, wsn = _workspace(ops)

    def launch(view, bs):
        if xbs == 0:
            ops.conv2d(xv, wp, b, ksize=ks, stride=stride, dil=dil, pad=pad, pad_mode=pad_mode, in_up=up, in_sub=sub, act=t["act"],
                       act_slope=t["act_slope"], act_slope_t=slope_t, in_scale=sc, in_shift=sh, in_slope_t=sl, residual=res, out=view,
                       out_batch_stride=bs, cfg=cfg, split_k=split_k, tune=False)
            return
        d = ops._conv_desc(c["N"], t["Cin"], c["H"], c["W"], t["Cout"], ksize=ks, stride=stride, dil=dil, pad=pad, pad_mode=pad_mode,
                           in_up=up, in_sub=sub, act=t["act"], act_slope=t["act_slope"], in_prelu=sl is not None, cfg=cfg,
                           split_k=split_k, x_batch_stride=xbs, y_batch_stride=bs)
        _check(lib.dvc_conv2d(ctypes.byref(d), _p(xv), _p(wp), _p(b), _p(sc), _p(sh), _p(sl), _p(slope_t), _p(res), _p(view), wsp, wsn,
                              ops._stream()), "dvc_conv2d")
    _twice(c, (c["N"], t["Cout"], t["OH"], t["OW"]), ref, launch)


@_params("direct")
def test_direct_engine_equals_float64(ops, lib, case):
    _conv2d_case(ops, lib, case)


@_params("streamk")
def test_stream_k_equals_float64(ops, lib, case):
    _conv2d_case(ops, lib, case)


@_params("image")
def test_image_input_kernel_equals_float64(ops, lib, case):
    _conv2d_case(ops, lib, case)


@_params("per_image")
def test_per_image_filters_equal_float64(ops, lib, case):
    _conv2d_case(ops, lib, case)


@_params("ws")
def test_conv_ws_equals_float64(ops, lib, case):
    c = case
    t = C.make_inputs(c)
    ref = C.reference(c, t)
    assert ops.ws_eligible(t["Cin"], t["Cout"], act=t["act"])
    xv, xbs = _place_x(t["x"], c["xin"] == "strided")
    u, b = ops.pack_ws_weight(t["w"].cuda()), _cu(t["b"])
    slope_t = torch.tensor([t["act_slope"]], device="cuda") if t["act"] == 2 else None

    def launch(view, bs):
        if xbs == 0:
            ops.conv2d_ws(xv, u, b, t["Cout"], act=t["act"], act_slope=t["act_slope"], act_slope_t=slope_t, out=view, out_batch_stride=bs)
            return
        d = ops._conv_desc(c["N"], t["Cin"], c["H"], c["W"], t["Cout"], act=t["act"], act_slope=t["act_slope"], x_batch_stride=xbs,
                           y_batch_stride=bs)
        _check(lib.dvc_conv2d_ws(ctypes.byref(d), _p(xv), _p(u), _p(b), _p(slope_t), _p(view), ops._stream()), "dvc_conv2d_ws")
    _twice(c, (c["N"], t["Cout"], c["H"], c["W"]), ref, launch)


@_params("wino")
def test_winograd_equals_float64(ops, lib, case):
    c = case
    t = C.make_inputs(c)
    ref = C.reference(c, t)
    ks, stride, dil, pad, pad_mode, up, sub = t["geom"]
    xv, xbs = _place_x(t["x"], c["xin"] == "strided")
    u, b, res = ops.pack_winograd_weight(t["w"].cuda()), _cu(t["b"]), _cu(t["res"])
    slope_t = torch.tensor([t["act_slope"]], device="cuda") if t["act"] == 2 else None
    kw = dict(dil=dil, pad_mode=pad_mode, in_up=up, in_sub=sub, act=t["act"], act_slope=t["act_slope"], act_slope_t=slope_t,
              cfg=c["cfg"], split_k=c["split_k"])
    wsp, wsn = _workspace(ops)

    def launch(view, bs):
        if xbs == 0:
            ops.conv2d_winograd(xv, u, b, residual=res, out=view, out_batch_stride=bs, **kw)
            return
        d = ops._conv_desc(c["N"], t["Cin"], c["H"], c["W"], t["Cout"], dil=dil, pad_mode=pad_mode, in_up=up, in_sub=sub, act=t["act"],
                           act_slope=t["act_slope"], cfg=c["cfg"], split_k=c["split_k"], x_batch_stride=xbs, y_batch_stride=bs)
        _check(lib.dvc_conv2d_winograd(ctypes.byref(d), _p(xv), _p(u), _p(b), _p(slope_t), _p(res), _p(view), wsp, wsn, ops._stream()),
               "dvc_conv2d_winograd")
    y = _twice(c, (c["N"], t["Cout"], t["OH"], t["OW"]), ref, launch)
    if c["defer"]:
        # the reduce left to the consumer: InstanceNorm of the partial sums == InstanceNorm of the materialised (exact) output
        slope = torch.tensor([0.25], device="cuda")
        part = ops.conv2d_winograd(xv, u, b, defer_reduce=True, **kw)
        got = ops.instnorm_apply(part, slope_t=slope)
        want = ops.instnorm_apply(y, slope_t=slope)
        torch.cuda.synchronize()
        kind = type(part).__name__
        report(f"conv exact {c['id']}: deferred reduce returned {kind}" + (f" (S = {part.S})" if kind == "ConvPartials" else ""))
        C.assert_exact(got, want, c["id"] + " (instnorm_apply of the deferred partial sums)")


@_params("wino_pool")
def test_winograd_pool_equals_float64(ops, case):
    c = case
    t = C.make_inputs(c)
    ref, ref_pool = C.reference(c, t)
    u, b, x = ops.pack_winograd_weight(t["w"].cuda()), _cu(t["b"]), t["x"].cuda()
    slope_t = torch.tensor([t["act_slope"]], device="cuda") if t["act"] == 2 else None
    run = lambda: ops.conv2d_winograd_pool(x, u, b, act=t["act"], act_slope=t["act_slope"], act_slope_t=slope_t,      # noqa: E731
                                           pad_mode=c["pad_mode"], want_full=c["want_full"])
    full, pooled = run()
    full2, pooled2 = run()
    torch.cuda.synchronize()
    assert (full is not None) == c["want_full"]
    C.assert_exact(pooled, ref_pool, c["id"] + " (pooled)")
    C.assert_exact(pooled2, pooled, c["id"] + " (pooled, second run)")
    if c["want_full"]:
        C.assert_exact(full, ref, c["id"])
        C.assert_exact(full2, full, c["id"] + " (second run)")
    TALLY["wino_pool"]["run"] += 1
    report(f"conv exact {c['id']}: equal to float64 in all {pooled.numel()} pooled elements" + (" and the full tensor" if c["want_full"] else ""))


@_params("wino_dual")
def test_winograd_dual_equals_float64(ops, case):
    c = case
    t = C.make_dual(c)
    ref = C.ref_dual(c, t)
    u = torch.cat((ops.pack_winograd_weight(t["wA"].cuda()), ops.pack_winograd_weight(t["wB"].cuda())), dim=1).contiguous()
    b = (t["bA"] + t["bB"]).cuda()
    slope_t = torch.tensor([t["act_slope"]], device="cuda") if t["act"] == 2 else None
    xA, xB = t["xA"].cuda(), t["xB"].cuda()
    run = lambda: ops.conv2d_winograd_dual(xA, xB, u, b, dil=c["dil"], pad_mode=c["pad_mode"], in_upA=c["upA"], in_upB=c["upB"],      # noqa: E731
                                           act=t["act"], act_slope=t["act_slope"], act_slope_t=slope_t)
    y, y2 = run(), run()
    torch.cuda.synchronize()
    C.assert_exact(y, ref, c["id"])
    C.assert_exact(y2, y, c["id"] + " (second run)")
    TALLY["wino_dual"]["run"] += 1
    report(f"conv exact {c['id']}: equal to float64 in all {y.numel()} elements")


@_params("wino_group")
def test_winograd_group_equals_float64(ops, case):
    """ops.conv3x3_group with every item on the Winograd engine: each item equal to its float64 reference; with the reduce
    deferred, instnorm_apply_group of the items' partial sums equals instnorm_apply of the materialised outputs."""
    c = case
    data = C.make_group(c)
    refs = C.ref_group(c, data)
    act, act_slope = C.ACTS[c["act"]]
    slope_t = torch.tensor([act_slope], device="cuda") if act == 2 else None
    items = []
    for i in data:
        w = i["w"].cuda()
        packs = (lambda w_: (lambda kind: ops.pack_winograd_weight(w_) if kind == "winograd" else ops.pack_conv_weight(w_)))(w)
        items.append(dict(x=i["x"].cuda(), weight=w, packs=packs, bias=i["b"].cuda(), pad_mode=c["pad_mode"], in_up=i["up"], act=act,
                          act_slope=act_slope, act_slope_t=slope_t))
    algo = ops.conv_algo()
    ops.set_conv_algo("winograd")           # (maps this small are below the automatic choice's 13 x 24 rule)
    try:
        ys = ops.conv3x3_group(items)
        ys2 = ops.conv3x3_group(items)
        torch.cuda.synchronize()
        for k, (y, y2, ref) in enumerate(zip(ys, ys2, refs)):
            C.assert_exact(y, ref, f"{c['id']} item {k}")
            C.assert_exact(y2, y, f"{c['id']} item {k} (second run)")
        if c["defer"]:
            slope = torch.tensor([0.25], device="cuda")
            parts = ops.conv3x3_group([dict(it, defer_reduce=True) for it in items])
            got = ops.instnorm_apply_group([dict(x=p, slope_t=slope) for p in parts])
            torch.cuda.synchronize()
            kinds = [type(p).__name__ for p in parts]
            report(f"conv exact {c['id']}: deferred group returned {kinds}")
            for k, (g, y) in enumerate(zip(got, ys)):
                C.assert_exact(g, ops.instnorm_apply(y, slope_t=slope), f"{c['id']} item {k} (instnorm of the deferred partial sums)")
    finally:
        ops.set_conv_algo(algo)
    TALLY["wino_group"]["run"] += 1
    report(f"conv exact {c['id']}: {len(items)} items equal to float64")


def test_share_of_refused_plans_per_engine():
    """Last in the module: per engine, the cases run and the cases skipped on a planning refusal of a forced plan; at most 20 %
    of an engine's cases may be skips."""
    for e, n in TALLY.items():
        total = n["run"] + n["skipped"]
        report(f"conv exact {e}: {n['run']} cases run, {n['skipped']} skipped ({100.0 * n['skipped'] / max(total, 1):.1f} % of {total}, cap 20 %)")
    for e, n in TALLY.items():
        assert n["skipped"] <= C.SKIP_CAP * max(n["run"] + n["skipped"], 1), (e, n)
