"""Step-wise audit of the backward passes (tests/test_gpu_bwd_audit.py, tests/test_bwd_audit_host.py).

An end-to-end gradient through 31 layers amplifies the forward's fp32 rounding and flips ReLU masks, so its bound at 216x384
is loose (tests/test_gpu_cvn_backward.py).  Each single backward launch, however, is a short, well-conditioned map of ITS
inputs.  This module holds

* a float64 CPU reference per launch kind of `dvc_amd.ops` (`ref_*`), evaluated on the launch's own (device) inputs;
* the error measures, all normalised by the reference, never by the output under test;
* `audit_*`: (result, inputs) -> one record with measures, yardsticks and bounds; `violations(record)` lists what exceeds;
* `Recorder`: a context manager that swaps those attributes of `dvc_amd.ops` for wrappers which run the real function,
  audit the call at once (so a large backward never holds more than one step's tensors on the host) and append the record.

The bounds are named constants here so that the GPU test and the CPU test that seeds defects use the same numbers.
"""
import time

import torch
import torch.nn.functional as F

# ---- bounds.  Input gradients run on the forward's convolution engines and carry their bounds (tests/test_gpu_ops.py: 2e-5 for
# the direct / weights-in-registers / stream-K engines "fp32 accumulation over <= 2304 terms", 5e-5 for Winograd F(2x2,3x3)).
DGRAD_BOUND = {"direct": 2e-5, "direct-ws": 2e-5, "winograd": 5e-5}
# A non-Winograd record over its bound (the 512-channel layers sum 4608 terms, twice what the 2e-5 was stated for) is allowed
# max(bound, YARD_FACTOR x the error of the same step by float32 CPU ATen): 4 covers two legitimate fp32 summation orders.
YARD_FACTOR = 4.0
# Sums over every position (dW, db, d ss, the head's sums) and the elementwise-plus-two-means maps (inorm / head dZ): no constant
# fixed in advance; max(SUM_FLOOR, YARD_FACTOR x the float32 CPU restatement's error against float64), per measure.
SUM_FLOOR = 1e-6
# dvc_vgg_conv1_bwd: 576 fp32 terms in a fixed order, the direct engine's number.
CONV1_BWD_BOUND = 2e-5

BWD_PREFIXES = ("vgg_bwd.", "cvn_bwd.")
PATCHED = ("conv3x3", "cvn_wgrad", "cvn_head_bwd", "cvn_inorm_bwd", "vgg_act_bwd", "vgg_pool_act_bwd", "vgg_conv1_bwd")


# ================================================================================================ measures
def relerr(got, ref):
    """max |got - ref| / max |ref| (the suite's relerr)."""
    ref = ref.double()
    return ((got.double() - ref).abs().max() / ref.abs().max().clamp_min(1e-300)).item()


def _rel_l2(diff, ref, dims):
    """||diff|| / ||ref|| over `dims`; a slice whose reference is exactly 0 gives 0 if it was reproduced exactly, else inf."""
    d, r = diff.pow(2).sum(dims).sqrt(), ref.pow(2).sum(dims).sqrt()
    e = d / r.clamp_min(1e-300)
    return torch.where(r > 0, e, torch.where(d > 0, torch.full_like(e, float("inf")), torch.zeros_like(e)))


def dw_measures(got, ref):
    """whole-tensor relerr, relative L2 per filter tap (nine numbers) and the worst relative L2 per output channel."""
    ref = ref.double()
    diff = got.double() - ref
    taps = _rel_l2(diff, ref, (0, 1)).reshape(-1)
    m = {"dW.whole": relerr(got, ref), "dW.chan": _rel_l2(diff, ref, (1, 2, 3)).max().item()}
    for t in range(taps.numel()):
        m["dW.tap%d" % t] = taps[t].item()
    return m


def map_measures(got, ref, width, prefix=""):
    """relerr over the whole map, over the border ring of `width` pixels and over the interior (None where that set is empty),
    each normalised by the reference over the same set."""
    ref = ref.double()
    H, W = ref.shape[-2:]
    m = {prefix + "whole": relerr(got, ref)}
    ring = torch.zeros(H, W, dtype=torch.bool)
    ring[:width] = ring[-width:] = True
    ring[:, :width] = ring[:, -width:] = True
    d, a = (got.double() - ref).abs(), ref.abs()
    m[prefix + "ring"] = (d[..., ring].max() / a[..., ring].max().clamp_min(1e-300)).item()
    m[prefix + "interior"] = None if ring.all() else (d[..., ~ring].max() / a[..., ~ring].max().clamp_min(1e-300)).item()
    return m


# ================================================================================================ float64 step references
def up2(x):
    return x.repeat_interleave(2, 2).repeat_interleave(2, 3)


def ref_dgrad(dZ, wt, dil=1):
    """conv3x3(dZ, wt, ..., dil=d, layer="*_bwd.*"): wt is already W^T flipped (every zero-padded channel included)."""
    return F.conv2d(dZ.double(), wt.double(), padding=dil, dilation=dil)


def ref_wgrad(dZ, X, dil=1, in_up=1, dtype=torch.float64):
    """cvn_wgrad: (dW, db)."""
    dZ, X = dZ.to(dtype), X.to(dtype)
    Xf = up2(X) if in_up == 2 else X
    dW = torch.nn.grad.conv2d_weight(Xf, (dZ.shape[1], X.shape[1], 3, 3), dZ, padding=dil, dilation=dil)
    return dW, dZ.sum((0, 2, 3))


def ref_head_bwd(ab, g, w, R, slope=0.2, dtype=torch.float64):
    """cvn_head_bwd: (dZ, dW [2, C], db [2]) of conv10_ab (1x1) + tanh * 128 behind a leaky ReLU whose output is R."""
    ab, g, w, R = ab.to(dtype), g.to(dtype), w.to(dtype), R.to(dtype)
    dpre = g * 128 * (1 - (ab / 128) ** 2)
    dR = torch.einsum("oc,bohw->bchw", w, dpre)
    one = torch.ones((), dtype=dtype)
    dZ = dR * torch.where(R > 0, one, one * slope)
    return dZ, torch.einsum("bohw,bchw->oc", dpre, R), dpre.sum((0, 2, 3))


def ref_inorm_bwd(n, rstd, R, g_full=None, g_ss=None, ss_w=None, g_up=None, dtype=torch.float64):
    """cvn_inorm_bwd — the kernel's arithmetic (dvc_cvn_inorm_bwd) restated: (dZ, d ss_w or None).  rstd: one value per
    (image, channel) plane, any shape with N * C elements."""
    cv = lambda t: None if t is None else t.to(dtype)
    n, R, g_full, g_ss, ss_w, g_up = cv(n), cv(R), cv(g_full), cv(g_ss), cv(ss_w), cv(g_up)
    rstd = rstd.to(dtype).reshape(n.shape[0], n.shape[1], 1, 1)
    dn = torch.zeros_like(n)
    if g_full is not None:
        dn = dn + g_full
    if g_ss is not None:
        dn[:, :, ::2, ::2] += ss_w.view(1, -1, 1, 1) * g_ss
    if g_up is not None:
        dn = dn + F.avg_pool2d(g_up, 2) * 4
    md = dn.mean((2, 3), keepdim=True)
    mdn = (dn * n).mean((2, 3), keepdim=True)
    dx = rstd * (dn - md - n * mdn) * (R > 0)
    dss = (n[:, :, ::2, ::2] * g_ss).sum((0, 2, 3)) if g_ss is not None else None
    return dx, dss


def ref_act_bwd(dX, g, R):
    """vgg_act_bwd by ATen float32 CPU autograd: d/dz of <relu(z), dX> + <relu(z), g> at a z whose ReLU is the saved R."""
    z = R.detach().float().clone().requires_grad_(True)
    with torch.enable_grad():
        r = F.relu(z)
        sum((r * t.float()).sum() for t in (dX, g) if t is not None).backward()
    return z.grad


def ref_pool_act_bwd(dP, gP, gR, R, avg=False):
    """vgg_pool_act_bwd by ATen float32 CPU autograd through relu + 2x2 max / average pool: masks and arg-maxes from R."""
    z = R.detach().float().clone().requires_grad_(True)
    with torch.enable_grad():
        r = F.relu(z)
        p = F.avg_pool2d(r, 2, 2) if avg else F.max_pool2d(r, 2, 2)
        terms = [(p * t.float()).sum() for t in (dP, gP) if t is not None]
        if gR is not None:
            terms.append((r * gR.float()).sum())
        sum(terms).backward()
    return z.grad


def ref_conv1_bwd(dZ, w_t):
    return F.conv2d(dZ.double(), w_t.double(), padding=1)


# ================================================================================================ records
def _finish(rec, measures, bounds, yard=None, ref_max=None):
    rec.update(measures=measures, bounds=bounds, yard=yard, ref_max=ref_max)
    return rec


def _yard_bounds(measures, yard, floor):
    return {k: max(floor, YARD_FACTOR * yard[k]) for k, v in measures.items() if v is not None}


def audit_dgrad(got, dZ, wt, dil=1, engine="direct", layer=None, keep=None):
    """An input gradient on a convolution engine.  keep: the number of leading output channels the caller uses (the rest are
    the zero filters of a padded layer and must come out exactly 0)."""
    rec = dict(kind="dgrad", layer=layer, engine=engine, shape=tuple(dZ.shape), out=tuple(got.shape), dil=dil)
    if engine not in DGRAD_BOUND:
        raise KeyError(f"{layer}: no stated bound for engine {engine!r}")
    ref = ref_dgrad(dZ, wt, dil)
    m = map_measures(got, ref, dil)
    if keep is not None:
        rec["pad_zero"] = bool((got[:, keep:] == 0).all()) and bool((ref[:, keep:] == 0).all())
    b0 = DGRAD_BOUND[engine]
    bounds = {k: b0 for k, v in m.items() if v is not None}
    yard = None
    if engine != "winograd" and any(v is not None and v > b0 for v in m.values()):
        # the same step by float32 CPU ATen: how far a legitimate fp32 evaluation of this very sum sits from float64
        yard = map_measures(F.conv2d(dZ.float(), wt.float(), padding=dil, dilation=dil), ref, dil)
        bounds = {k: max(b0, YARD_FACTOR * yard[k]) for k in bounds}
    return _finish(rec, m, bounds, yard, ref.abs().max().item())


def audit_wgrad(got_dW, got_db, dZ, X, dil=1, in_up=1, layer=None):
    rec = dict(kind="wgrad", layer=layer, engine="wgrad", shape=tuple(dZ.shape), out=tuple(got_dW.shape), dil=dil, in_up=in_up)
    dW, db = ref_wgrad(dZ, X, dil, in_up)
    dW32, db32 = ref_wgrad(dZ, X, dil, in_up, dtype=torch.float32)
    m = dw_measures(got_dW, dW)
    m["db.whole"] = relerr(got_db, db)
    yard = dw_measures(dW32, dW)
    yard["db.whole"] = relerr(db32, db)
    rec["dead_channels"] = int((dW.flatten(1).abs().amax(1) == 0).sum())
    return _finish(rec, m, _yard_bounds(m, yard, SUM_FLOOR), yard, min(dW.abs().max().item(), db.abs().max().item()))


def audit_head(got, ab, g, w, R, slope=0.2, layer="conv10_ab"):
    rec = dict(kind="head", layer=layer, engine="head_bwd", shape=tuple(R.shape), out=tuple(R.shape))
    ref = ref_head_bwd(ab, g, w, R, slope)
    r32 = ref_head_bwd(ab, g, w, R, slope, dtype=torch.float32)
    names = ("dZ.whole", "dW.whole", "db.whole")
    m = {k: relerr(a.reshape(b.shape), b) for k, a, b in zip(names, got, ref)}
    yard = {k: relerr(a, b) for k, a, b in zip(names, r32, ref)}
    return _finish(rec, m, _yard_bounds(m, yard, SUM_FLOOR), yard, min(t.abs().max().item() for t in ref))


def audit_inorm(got_dZ, got_dss, n, rstd, R, g_full=None, g_ss=None, ss_w=None, g_up=None, layer=None):
    kinds = "+".join(k for k, t in (("full", g_full), ("ss", g_ss), ("up", g_up)) if t is not None)
    rec = dict(kind="inorm", layer=layer, engine="inorm_bwd:" + kinds, shape=tuple(n.shape), out=tuple(n.shape))
    dZ, dss = ref_inorm_bwd(n, rstd, R, g_full, g_ss, ss_w, g_up)
    z32, s32 = ref_inorm_bwd(n, rstd, R, g_full, g_ss, ss_w, g_up, dtype=torch.float32)
    m, yard = {"dZ.whole": relerr(got_dZ, dZ)}, {"dZ.whole": relerr(z32, dZ)}
    ref_max = dZ.abs().max().item()
    if (got_dss is None) != (dss is None):
        m["dss.whole"], yard["dss.whole"] = float("inf"), 0.0
    elif dss is not None:
        m["dss.whole"], yard["dss.whole"] = relerr(got_dss.reshape(-1), dss), relerr(s32, dss)
        ref_max = min(ref_max, dss.abs().max().item())
    return _finish(rec, m, _yard_bounds(m, yard, SUM_FLOOR), yard, ref_max)


def _audit_exact(rec, got, ref):
    eq = bool(torch.equal(got, ref))
    worst = 0.0 if eq else float((got.double() - ref.double()).abs().nan_to_num(float("inf")).max())
    rec["differing"] = 0 if eq else int((~((got == ref) | (got.isnan() & ref.isnan()))).sum())
    return _finish(rec, {"bitwise.maxdiff": worst if not eq else 0.0, "bitwise.equal": eq}, {"bitwise.equal": True}, None,
                   ref.abs().max().item())


def audit_act(got, dX, g, R, layer=None):
    rec = dict(kind="act", layer=layer, engine="act_bwd", shape=tuple(R.shape), out=tuple(R.shape))
    return _audit_exact(rec, got, ref_act_bwd(dX, g, R))


def audit_pool_act(got, dP, gP, gR, R, avg=False, layer=None):
    rec = dict(kind="pool_act", layer=layer, engine="pool_act_bwd:" + ("avg" if avg else "max"), shape=tuple(R.shape),
               out=tuple(R.shape))
    return _audit_exact(rec, got, ref_pool_act_bwd(dP, gP, gR, R, avg))


def audit_conv1_bwd(got, dZ, w_t, layer="vgg_bwd.conv1_1"):
    rec = dict(kind="conv1_bwd", layer=layer, engine="conv1_bwd", shape=tuple(dZ.shape), out=tuple(got.shape))
    ref = ref_conv1_bwd(dZ, w_t)
    m = map_measures(got, ref, 1)
    return _finish(rec, m, {k: CONV1_BWD_BOUND for k, v in m.items() if v is not None}, None, ref.abs().max().item())


def violations(rec):
    """What in a record exceeds its bound (an empty list: the step passes)."""
    bad = []
    for k, b in rec["bounds"].items():
        v = rec["measures"][k]
        if b is True:
            if v is not True:
                bad.append(f"{k}: not bit-identical ({rec.get('differing')} elements differ)")
        elif not v <= b:            # (a NaN measure fails)
            bad.append(f"{k}: {v:.3e} > {b:.3e}")
    if rec.get("pad_zero") is False:
        bad.append("the zero-padded output channels are not exactly 0")
    if not rec["ref_max"] > 0:
        bad.append("the reference is identically 0 (every relative measure is vacuous)")
    return [f"{rec['kind']} {rec['layer']} [{rec['engine']}] {tuple(rec['shape'])}: {s}" for s in bad]


def line(rec, case=""):
    """One report line per launch: layer, engine, shapes, each measure with its yardstick, ratio and bound."""
    parts = []
    for k, v in rec["measures"].items():
        if k == "bitwise.equal" or v is None:
            continue
        s = f"{k}={v:.2e}"
        y = rec["yard"].get(k) if rec["yard"] else None
        if y is not None:
            s += f"(yard {y:.2e} ratio {v / y:.2f})" if y > 0 else f"(yard {y:.2e})"
        if k in rec["bounds"]:
            s += f"<={rec['bounds'][k]:.1e}"
        parts.append(s)
    if "bitwise.equal" in rec["measures"]:
        parts.append("bit-identical to ATen" if rec["measures"]["bitwise.equal"] else "NOT bit-identical")
    extra = "".join(f" {k}={rec[k]}" for k in ("dil", "in_up", "pad_zero", "dead_channels") if rec.get(k) not in (None, 1, 0))
    return (f"bwd_audit {case} {rec['kind']} {rec['layer']} engine={rec['engine']} in={tuple(rec['shape'])} "
            f"out={tuple(rec['out'])}{extra} ref_max={rec['ref_max']:.2e} {rec['secs']:.1f}s: " + " ".join(parts))


def worst_by_kind(records, key=None):
    """kind -> the record with the largest measure-to-bound ratio (bitwise kinds: any failing one, else the first)."""
    out = {}
    for r in records:
        num = [v / r["bounds"][k] for k, v in r["measures"].items() if k in r["bounds"] and r["bounds"][k] is not True]
        score = max(num) if num else (0.0 if r["measures"].get("bitwise.equal") else float("inf"))
        k = r["kind"] if key is None else key(r)
        if k not in out or score > out[k][0]:
            out[k] = (score, r)
    return {k: v[1] for k, v in out.items()}


# ================================================================================================ the recorder
def _cpu(t):
    return None if t is None else t.detach().cpu()


class Recorder:
    """with Recorder() as rec: ... — every backward launch made through `dvc_amd.ops` inside the block is run, audited against
    its float64 reference on its own inputs, and appended to rec.records in launch order.  `nets.py` looks the functions up as
    `ops.X`, so an attribute swap is enough; every attribute (and ops.conv_record) is restored on exit, exception or not.
    Forward launches (conv3x3 with a layer name outside *_bwd.*) pass straight through."""

    def __init__(self, ops=None):
        if ops is None:
            from dvc_amd import ops
        self.ops = ops
        self.records = []
        self._saved = None

    def __enter__(self):
        ops = self.ops
        self._saved = {name: getattr(ops, name) for name in PATCHED}
        self._conv_record = ops.conv_record
        if ops.conv_record is None:
            ops.conv_record = []
        for name in PATCHED:
            setattr(ops, name, getattr(self, "_wrap_" + name)(self._saved[name]))
        return self

    def __exit__(self, *exc):
        for name, fn in self._saved.items():
            setattr(self.ops, name, fn)
        self.ops.conv_record = self._conv_record
        self._saved = None
        return False

    @staticmethod
    def _sync(t):
        if t.is_cuda:
            torch.cuda.synchronize(t.device)

    def _add(self, t0, rec):
        rec["secs"] = time.time() - t0
        self.records.append(rec)

    def _wrap_conv3x3(self, real):
        def conv3x3(x, weight, packs, bias, *args, **kw):
            layer = kw.get("layer")
            if layer is None or not layer.startswith(BWD_PREFIXES):
                return real(x, weight, packs, bias, *args, **kw)
            log = self.ops.conv_record
            mark = len(log)
            y = real(x, weight, packs, bias, *args, **kw)
            self._sync(y)
            t0 = time.time()
            new = log[mark:]
            assert len(new) == 1, (layer, "expected one convolution launch, conv_record has", new)
            engine = new[0].get("algo", "direct")
            w = _cpu(weight)
            live = (w.flatten(1) != 0).any(1).nonzero()
            keep = int(live.max()) + 1 if live.numel() else 0     # (cvn_bwd.conv1_1.0: zero filters appended up to pad_to)
            self._add(t0, audit_dgrad(_cpu(y), _cpu(x), w, kw.get("dil", 1), engine, layer, keep if keep < w.shape[0] else None))
            return y
        return conv3x3

    def _wrap_cvn_wgrad(self, real):
        def cvn_wgrad(dZ, X, *, dil=1, in_up=1, splits=None):
            dW, db = real(dZ, X, dil=dil, in_up=in_up, splits=splits)
            self._sync(dW)
            t0 = time.time()
            self._add(t0, audit_wgrad(_cpu(dW), _cpu(db), _cpu(dZ), _cpu(X), dil, in_up, layer=self._wgrad_layer(dZ, X, dil, in_up)))
            return dW, db
        return cvn_wgrad

    @staticmethod
    def _wgrad_layer(dZ, X, dil, in_up):
        return f"wgrad {X.shape[1]}->{dZ.shape[1]} d{dil} up{in_up}"

    def _wrap_cvn_head_bwd(self, real):
        def cvn_head_bwd(ab, grad_ab, w_ab, R, slope=0.2):
            out = real(ab, grad_ab, w_ab, R, slope=slope)
            self._sync(out[0])
            t0 = time.time()
            self._add(t0, audit_head(tuple(_cpu(t) for t in out), _cpu(ab), _cpu(grad_ab), _cpu(w_ab), _cpu(R), slope))
            return out
        return cvn_head_bwd

    def _wrap_cvn_inorm_bwd(self, real):
        def cvn_inorm_bwd(n, rstd, R, g_full=None, g_ss=None, ss_w=None, g_up=None):
            dZ, dss = real(n, rstd, R, g_full=g_full, g_ss=g_ss, ss_w=ss_w, g_up=g_up)
            self._sync(dZ)
            t0 = time.time()
            self._add(t0, audit_inorm(_cpu(dZ), _cpu(dss), _cpu(n), _cpu(rstd), _cpu(R), _cpu(g_full), _cpu(g_ss), _cpu(ss_w),
                                      _cpu(g_up), layer=f"inorm C{n.shape[1]}"))
            return dZ, dss
        return cvn_inorm_bwd

    def _wrap_vgg_act_bwd(self, real):
        def vgg_act_bwd(dX, g, R, out=None):
            dX0 = _cpu(dX)              # (out may be dX: the call then overwrites its own input)
            if dX0 is not None and not dX.is_cuda:
                dX0 = dX0.clone()
            y = real(dX, g, R, out=out)
            self._sync(y)
            t0 = time.time()
            self._add(t0, audit_act(_cpu(y), dX0, _cpu(g), _cpu(R), layer=f"act C{R.shape[1]}"))
            return y
        return vgg_act_bwd

    def _wrap_vgg_pool_act_bwd(self, real):
        def vgg_pool_act_bwd(dP, gP, gR, R, avg=False):
            y = real(dP, gP, gR, R, avg=avg)
            self._sync(y)
            t0 = time.time()
            self._add(t0, audit_pool_act(_cpu(y), _cpu(dP), _cpu(gP), _cpu(gR), _cpu(R), avg, layer=f"pool_act C{R.shape[1]}"))
            return y
        return vgg_pool_act_bwd

    def _wrap_vgg_conv1_bwd(self, real):
        def vgg_conv1_bwd(dZ, w_t):
            y = real(dZ, w_t)
            self._sync(y)
            t0 = time.time()
            self._add(t0, audit_conv1_bwd(_cpu(y), _cpu(dZ), _cpu(w_t)))
            return y
        return vgg_conv1_bwd


# ================================================================================================ expected launches
def expected_cvn_kinds(convs, need_dx=True):
    """The step kinds ColorVidNet._backward must launch, in order, derived from arch.CVN_CONVS: the head; then per layer in
    reverse its dZ step (unless it is the head's, or a skip convolution sharing its block's), its weight gradient, and its input
    gradient (the layer reading `x`: only when d x is wanted)."""
    adder = {c["add"] for c in convs if c["add"] is not None}
    kinds = ["head"]
    have = {convs[-1]["dst"]}
    for c in reversed(convs):
        if c["dst"] not in have and c["dst"] not in adder:
            normed = any(e["src"] == c["dst"] and e["pre"] is not None for e in convs)
            kinds.append("inorm" if normed else "act")
            have.add(c["dst"])
        kinds.append("wgrad")
        if c["src"] != "x" or need_dx:
            kinds.append("dgrad")
    return kinds


def expected_vgg_kinds(keys, out_keys):
    """The step kinds VGG19_pytorch._input_grad must launch for the requested keys (arch.VGG_KEYS order)."""
    i = max(keys.index(k) for k in out_keys)
    kinds = []
    while i >= 0:
        if keys[i][0] == "p":
            kinds.append("pool_act")
            i -= 1
        else:
            kinds.append("act")
        if i == 0:
            kinds.append("conv1_bwd")
            break
        kinds.append("dgrad")
        i -= 1
    return kinds
