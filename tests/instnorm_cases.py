"""Cases, data and references for the InstanceNorm launches of csrc/norm_pool.hip (dvc_instnorm_stats, dvc_affine_act,
dvc_instnorm_apply, dvc_instnorm_apply_partials, dvc_instnorm_apply_group), importable without a GPU
(tests/test_instnorm_cases_host.py checks the generators, the references and the bound on the CPU,
tests/test_gpu_instnorm_sweep.py runs the cases on the kernels).

Plane sizes come from the constants of the source (`constants`: the 1024 virtual threads of plane_stats, the block-size
thresholds, the LDS limit of the partial-sum variant): the smallest planes at which plane_stats takes each of its loops, one
element before and at every threshold, one past the LDS limit.  The module does not import when a constant is not found.

Two data regimes.

*Probe*: every channel of a tensor is zero except for the value 4096 at one position (`probe_positions`: the ends, the
hand-over of the float4 loops to the scalar tail, every multiple of 4 * VT and 16 * VT with its neighbours, the first piece the
four-in-flight loop fetches ahead); a second tensor has two such values per plane, so that "dropped" (S = 0 or 4096) and
"counted twice" (S = 8192 or 12288) read differently.  S <= 2^13 and Q <= 2^25 are integers, exact in double in any order, so
(scale, shift) must be within one float32 ulp of the exact value (`probe_stats`, 60 decimal digits) and bit-equal from every
entry point, block size and alignment.  For the partial-sum variant the slices hold integers in [-4, 4] plus the probe, the
bias is an integer and the slope 0.25 or 0.5: the plane holds multiples of 1/4 below 2^13, its S and Q are exact as well
(`exact_in_double`).

*Graded*: standard normal draws * 3 + 1.5 in float32, the suite's usual.

The bound.  tests/instnorm_bound.py derives, for y = fma(x, sc, sh) with sc = fl(rstd), sh = fl(-mean * rstd) and
u = 2^-24: |y_kernel - y| <= u * (2 * max|x| * rstd + max|y|) <= 2^-23 * (max|x| * rstd + max|y| + 1) per plane.  Here
sc = fl(rstd * cs) and sh = fl(-mean * rstd * cs): both roundings are relative, so the two terms in max|x| * rstd carry the
factor |cs|, and y is the scaled value t = (x - mean) * rstd * cs:
    e0 = 2^-23 * (max|x| * rstd * |cs| + max|t| + 1).
A residual is added in float32, r = fl(t + res): one more rounding of at most u * max|t + res| (the reference's values; the
`+ 1` of e0 covers the second order).  The PReLU multiplies the negative values by the slope in float32: one more rounding of
at most u * max|out|; the error carried in is multiplied by |slope| <= 1, and where the computed r and the true r' have
different signs both are within the carried error e of zero and of each other, |r - slope * r'| <= |r - r'| <= e.  So
    bound = e0 [+ 2^-24 * max|t + res|] [+ 2^-24 * max|out|],
per plane, maxima over the whole plane (the index maps only gather).  The second output is t2 = (x - mean) * rstd * cs2 with
its own e0.  Nothing here is fitted to the kernel; `emulate` (instnorm_bound.emulate_fma extended to the modes) is the error a
correct implementation makes, and the host test shows it inside the bound on every graded case.
"""
import decimal
import functools
import os
import re
import zlib

import numpy as np

from conv_exact_cases import all_pairs

SRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "deep-exemplar-based-video-colorization_amd", "csrc",
                   "norm_pool.hip")
EPS = float(np.float32(1e-5))                   # what the float argument of the entry points holds
ACT_NONE, ACT_RELU, ACT_PRELU, ACT_LEAKY = 0, 1, 2, 3          # include/dvc_hip.h
PROBE = 4096.0


# ---- the kernel's constants, from its source
def _find(pattern, text, what):
    m = re.search(pattern, text)
    if m is None:
        raise RuntimeError(f"instnorm_cases: {what} not found in {SRC} (pattern {pattern!r})")
    return [int(g) for g in m.groups()]


@functools.lru_cache(None)
def constants():
    with open(SRC) as f:
        text = f.read()
    (vt,) = _find(r"constexpr int VT = (\d+);", text, "VT")
    b1024, b512 = _find(r"return HW >= (\d+) \? 1024 : HW >= (\d+) \? 512 : 256;", text, "the instnorm_block thresholds")
    (pblock,) = _find(r"dim3\(H \* W >= (\d+) \? 1024 : 512\)", text, "the partials block threshold")
    (gblock,) = _find(r"if \(HW >= (\d+)\) block = 1024;", text, "the group block threshold")
    (lds,) = _find(r"\(long\)H \* W <= (\d+), \"dvc_instnorm_apply_partials", text, "the LDS limit")
    (glds,) = _find(r"HW <= (\d+), \"dvc_instnorm_apply_group", text, "the group's LDS limit")
    (smax,) = _find(r"S >= 1 && S <= (\d+)", text, "the largest S")
    (gmax,) = _find(r"#define INSTNORM_GROUP_MAX (\d+)", text, "INSTNORM_GROUP_MAX")
    ahead, pieces = _find(r"for \(; i \+ (\d+) \* VT \* 4 < HW4; i \+= (\d+) \* VT \* 4\)", text, "the in-flight loop")
    if gblock != pblock or glds != lds or pieces != ahead + 1:
        raise RuntimeError("instnorm_cases: the group launch and dvc_instnorm_apply_partials no longer share their limits")
    return dict(VT=vt, B1024=b1024, B512=b512, PBLOCK=pblock, LDS=lds, SMAX=smax, GMAX=gmax, FLY=ahead * 4 * vt, PIECES=pieces)


K = constants()
VT = K["VT"]


def _planes():
    """(H, W) per level; the element count comes from the constants, the factorisation is written next to it."""
    p, fly, lds, b5, b10 = 4 * VT, K["FLY"], K["LDS"], K["B512"], K["B1024"]
    table = [(1, 1, 1), (3, 1, 3), (15, 3, 5), (1215, 27, 45),
             (p, 64, 64),                       # one full pass of the virtual threads; the partials block threshold
             (p + 1, 17, 241), (b5 - 2, 90, 91), (b5, 64, 128),
             (fly, 96, 128),                    # the in-flight loop is not entered
             (fly + 4, 28, 439),                # entered by virtual thread 0 only
             (lds, 128, 128), (lds + 4, 68, 241),
             (b10 - 7, 181, 181), (b10, 128, 256), (b10 + 4, 12, 2731)]
    if K["PBLOCK"] != p:
        raise RuntimeError("instnorm_cases: the partials block threshold is no longer one pass of the virtual threads")
    for hw, h, w in table:
        if h * w != hw:
            raise RuntimeError(f"instnorm_cases: the level {h}x{w} no longer sits at {hw}: a constant of norm_pool.hip moved")
    return [(h, w) for _, h, w in table]


PLANES = _planes()
PLANES_PARTIALS = [s for s in PLANES if s[0] * s[1] <= K["LDS"]]
PLANE_OVER_LDS = next(s for s in PLANES if s[0] * s[1] > K["LDS"])
BIG = K["B1024"] - 7                            # from here on a case holds at most 5 planes (the float64 reference's time)
BATCHES, CHANNELS = [1, 2], [1, 3, 5]
UPS = [f"up{u}r{r}" for u in (2, 3, 4) for r in (0, 1, 2)] + ["up1r1", "up1r2"]
MODES = ["plain", "inplace", "res_slope", "slope", "cs_sub2"] + UPS
SECOND = ["none", "s1", "s2cs"]
LAYOUTS = ["dense", "slice"]
SLOPES = [0.25, 0.0, -0.5]
ENTRIES = ("apply", "stats", "partials")


def mode_params(mode):
    """up, sub, rpad and what else a mode switches on: res(idual), act (the norm's own PReLU), cs (chan_scale), inplace."""
    d = dict(up=1, sub=1, rpad=0, res=False, act=mode != "plain", cs=False, inplace=False)
    if mode == "inplace":                       # the residual blocks' form: y = x = prelu(norm(x) + res)
        d.update(res=True, inplace=True)
    elif mode == "res_slope":
        d.update(res=True)
    elif mode == "cs_sub2":
        d.update(cs=True, sub=2)
    elif mode.startswith("up"):
        d.update(up=int(mode[2]), rpad=int(mode[4]))
    return d


def _factors(entry):
    f = dict(plane=PLANES, N=BATCHES, C=CHANNELS, xlay=LAYOUTS, ylay=LAYOUTS, rlay=LAYOUTS, slope=SLOPES)
    if entry == "apply":
        f.update(mode=MODES, second=SECOND, scale_out=[False, True])
    elif entry == "stats":                      # dvc_instnorm_stats -> dvc_affine_act: no sub, one output, chan_scale by itself
        f.update(mode=["plain", "res_slope", "slope"] + UPS, cs=[False, True])
    else:
        del f["xlay"]
        f.update(plane=PLANES_PARTIALS, mode=[m for m in MODES if m != "inplace"], second=SECOND, scale_out=[False, True],
                 S=[1, 2, 3, K["SMAX"]], bias=[False, True], act=["none", "relu", "prelu_ptr", "leaky"], part=["aligned", "off1"])
    return f


def _valid(c):
    m = mode_params(c["mode"])
    if m["inplace"] and (c.get("second", "none") != "none" or c["ylay"] != c["xlay"]):
        return False                            # refused: a second output excludes in-place operation; y IS x
    if not m["res"] and c["rlay"] != "dense":   # levels of a factor the mode does not use: one id per launch
        return False
    if not m["act"] and c["slope"] != SLOPES[0]:
        return False
    if c["plane"][0] * c["plane"][1] >= BIG and c["N"] * c["C"] > 5:
        return False
    return True


def _case_id(entry, k, c):
    bits = [entry, f"{k:03d}", "%dx%d" % c["plane"], f"n{c['N']}c{c['C']}", c["mode"]]
    if entry == "partials":
        bits.append(f"S{c['S']}")
    return "-".join(bits)


@functools.lru_cache(None)
def generate(entry):
    """(cases, pairs of levels no valid case holds); a case is a dict of its levels + entry, H, W, HW, id, seed."""
    cases, impossible = all_pairs(_factors(entry), _valid, zlib.crc32(("instnorm_" + entry).encode()))
    out = []
    for k, c in enumerate(cases):
        cid = _case_id(entry, k, c)
        H, W = c["plane"]
        out.append(dict(c, entry=entry, H=H, W=W, HW=H * W, id=cid, seed=zlib.crc32(cid.encode()) % (1 << 31)))
    return out, impossible


def cases(entry):
    return generate(entry)[0]


def factors(entry):
    return _factors(entry)


@functools.lru_cache(None)
def group_cases():
    """1 to 4 items out of the apply and partials cases that have no second output, picked by what the group launch decides
    from all its items at once: the block size (512, or 1024 as soon as one item reaches the threshold) and the LDS image (the
    largest partial-sum item).  Every list also runs reversed."""
    A = [c for c in cases("apply") if c["second"] == "none"]
    P = [c for c in cases("partials") if c["second"] == "none"]
    thr = K["PBLOCK"]

    def pick(pool, pred, skip=0):
        hits = [c for c in pool if pred(c)]
        if len(hits) <= skip:
            raise RuntimeError("instnorm_cases: no case for a group item")
        return hits[skip]

    small = lambda c: c["HW"] < thr                                                          # noqa: E731
    lists = {
        "one_small": [pick(A, small)],
        "one_partials_at_the_limit": [pick(P, lambda c: c["HW"] == K["LDS"])],
        "two_small_mixed": [pick(A, lambda c: small(c) and c["HW"] % 4), pick(P, small)],
        "three_256_next_to_1024": [pick(A, lambda c: small(c) and c["C"] > 1), pick(P, lambda c: c["HW"] >= thr),
                                   pick(A, lambda c: c["HW"] >= K["B1024"])],
        "four_mixed": [pick(P, lambda c: small(c) and c["part"] == "off1"), pick(A, lambda c: c["HW"] == thr + 1),
                       pick(P, lambda c: c["HW"] == K["LDS"], 1), pick(A, lambda c: small(c) and mode_params(c["mode"])["inplace"])],
        "four_partials_below": [pick(P, lambda c, s=s: small(c) and c["S"] == s) for s in (1, 2, 3, K["SMAX"])],
        "two_apply_at_and_above": [pick(A, lambda c: c["HW"] == thr), pick(A, lambda c: c["HW"] == K["B512"])],
    }
    out = []
    for name, items in lists.items():
        for rev in (False, True):
            if rev and len(items) == 1:
                continue
            gid = f"group-{name}-{'rev' if rev else 'fwd'}"
            out.append(dict(id=gid, name=name, items=list(reversed(items)) if rev else list(items)))
    return out


# ---- data
def _graded(rng, *shape):
    return (rng.standard_normal(shape) * 3 + 1.5).astype(np.float32)


def _chan_scale(rng, C):
    return ((rng.random(C) + 0.5) * rng.choice([-1.0, 1.0], C)).astype(np.float32)


ACTS = dict(none=(ACT_NONE, 0.0, None), relu=(ACT_RELU, 0.0, None), prelu_ptr=(ACT_PRELU, 0.75, 0.25), leaky=(ACT_LEAKY, 0.2, None))


def make_data(c):
    """Graded inputs of a case as float32 arrays: x [N][C][H][W] (for partials: part [S][N][C][H][W], bias, the activation as
    (act, act_slope, value behind act_slope_ptr or None) and x = the float32 restatement of the plane), cs, cs2, res, slope."""
    rng = np.random.default_rng(c["seed"])
    m = mode_params(c["mode"])
    N, C, H, W = c["N"], c["C"], c["H"], c["W"]
    t = dict(cs=_chan_scale(rng, C) if (m["cs"] or c.get("cs")) else None,
             cs2=_chan_scale(rng, C) if c.get("second") == "s2cs" else None,
             res=_graded(rng, N, C, H, W) if m["res"] else None,
             slope=np.float32(c["slope"]) if m["act"] else None)
    if c["entry"] == "partials":
        S = c["S"]
        t["part"] = (rng.standard_normal((S, N, C, H, W)) * (3 / np.sqrt(S)) + 1.5 / S).astype(np.float32)
        t["bias"] = rng.standard_normal(C).astype(np.float32) if c["bias"] else None
        t["act"] = ACTS[c["act"]]
        t["x"] = restate_partials(t["part"], t["bias"], t["act"])
    else:
        t["x"] = _graded(rng, N, C, H, W)
    return t


def probe_positions(HW):
    v4, v16, HW4 = 4 * VT, 16 * VT, HW & ~3
    pos = {0, HW - 1, HW4 - 1, HW4, K["FLY"] - 1, K["FLY"], K["FLY"] + 1}
    for step in (v4, v16):
        for mult in range(0, HW, step):
            pos |= {mult - 1, mult, mult + 1}
    return sorted(p for p in pos if 0 <= p < HW)


def probe_tensor(H, W, two=False):
    """[1][P][H][W]: channel c is zero but for 4096 at its position (and, `two`, at the next channel's)."""
    pos = probe_positions(H * W)
    x = np.zeros((1, len(pos), H * W), np.float32)
    for c, p in enumerate(pos):
        x[0, c, p] = PROBE
        if two:
            x[0, c, pos[(c + 1) % len(pos)]] = PROBE
    return x.reshape(1, len(pos), H, W)


def probe_partials(H, W, S, seed):
    """Integer partial sums [S][1][P][H][W] in [-4, 4] with the probe of channel c added to slice c % S, an integer bias."""
    rng = np.random.default_rng(seed)
    pos = probe_positions(H * W)
    part = rng.integers(-4, 5, (S, 1, len(pos), H * W)).astype(np.float32)
    for c, p in enumerate(pos):
        part[c % S, 0, c, p] += PROBE
    return part.reshape(S, 1, len(pos), H, W), rng.integers(-3, 4, len(pos)).astype(np.float32)


def exact_in_double(x):
    """True when the sum and the sum of squares of every plane of x are exact in double in ANY order: the values are multiples
    of 1/4 and the sums of |4x| and of (4x)^2 stay below 2^53."""
    q = np.asarray(x, np.float64) * 4
    return bool((q == np.rint(q)).all() and np.abs(q).sum(axis=(-2, -1)).max() < 2.0 ** 53 and (q * q).sum(axis=(-2, -1)).max() < 2.0 ** 53)


def probe_stats(x, eps=EPS):
    """(scale, shift) [N][C] of exact-in-double planes, from integer sums in 60 decimal digits, rounded to double once."""
    decimal.getcontext().prec = 60
    q = np.rint(np.asarray(x, np.float64) * 4).astype(np.int64)
    N, C, H, W = q.shape
    sc, sh = np.zeros((N, C)), np.zeros((N, C))
    cache = {}
    for n in range(N):
        for c in range(C):
            key = (int(q[n, c].sum()), int((q[n, c] * q[n, c]).sum()))
            if key not in cache:
                mean = decimal.Decimal(key[0]) / (4 * H * W)
                var = decimal.Decimal(key[1]) / (16 * H * W) - mean * mean
                rstd = 1 / (var + decimal.Decimal(eps)).sqrt()
                cache[key] = (float(rstd), float(-mean * rstd))
            sc[n, c], sh[n, c] = cache[key]
    return sc, sh


def ulps(got, want):
    """|got - want| in float32 ulps of want (want in double)."""
    want = np.asarray(want, np.float64)
    return np.abs(np.asarray(got, np.float64) - want) / np.spacing(np.abs(want).astype(np.float32)).astype(np.float64)


def model_stats(flat, off, HW, bug=None, eps=EPS):
    """(scale, shift) in double of the plane flat[off : off + HW] as plane_stats would have them with a seeded defect: what a
    probe must notice.  A plane is `aligned` when its first element is a multiple of four floats from the buffer's."""
    lo, idx = off, np.arange(HW)
    keep = np.ones(HW, bool)
    aligned = off % 4 == 0
    if bug == "drop_tail" and aligned:
        keep[HW & ~3:] = False
    elif bug == "drop_fly" and aligned and (HW & ~3) > K["FLY"]:
        keep[(idx < (HW & ~3)) & ((idx // (4 * VT)) % K["PIECES"] == K["PIECES"] - 1)] = False
    elif bug == "neighbour" and not aligned:
        lo = off & ~3
    v = flat[lo:lo + HW].astype(np.float64)[keep]
    mean = v.sum() / HW
    var = max((v * v).sum() / HW - mean * mean, 0.0)
    rstd = 1.0 / np.sqrt(var + eps)
    return rstd, -mean * rstd


# ---- references
def restate_partials(part, bias, act, bug=None, dtype=np.float32):
    """x = act(((0 + p0) + p1 ...) + bias) in the kernel's order; in float32 these are the kernel's own IEEE operations."""
    code, aslope, aptr = act
    aslope = dtype(aptr if aptr is not None else aslope)
    S, _, C = part.shape[:3]
    v = np.zeros(part.shape[1:], dtype)
    for s in (range(S - 1, -1, -1) if bug == "reverse_slices" else range(S)):
        v = v + part[s].astype(dtype)
    b = (np.zeros(C, dtype) if bias is None else bias.astype(dtype)).reshape(1, C, 1, 1)
    if bug != "bias_after_act":
        v = v + b
    if code == ACT_RELU:
        v = np.where(v > 0, v, dtype(0))
    elif code in (ACT_PRELU, ACT_LEAKY):
        v = np.where(v >= 0, v, v * aslope)
    if bug == "bias_after_act":
        v = v + b
    return v.astype(dtype)


def out_size(H, W, up, sub, rpad, bug=None):
    if sub == 2:
        return (H // 2, W // 2) if bug == "sub_floor" else ((H + 1) // 2, (W + 1) // 2)
    return H * up + 2 * rpad, W * up


def index_maps(H, W, up, sub, rpad, bug=None):
    """Source row of every output row and source column of every output column: dvc_hip.h's y = [VH + 2 * rpad][VW],
    VH = H * up or ceil(H / 2), rows replicated `rpad` times on top and bottom."""
    OH, OW = out_size(H, W, up, sub, rpad, bug)
    VH = OH - 2 * rpad
    oy, ox = np.arange(OH), np.arange(OW)
    uy = np.clip(oy - rpad + (1 if bug == "rpad_off_by_one" and rpad else 0), 0, VH - 1)
    if sub == 2:
        return uy * 2, ox * 2
    if bug == "up_ceil":
        return np.minimum(-(-uy // up), H - 1), np.minimum(-(-ox // up), W - 1)
    return uy // up, ox // up


def gather(v, maps):
    rows, cols = maps
    return v[..., rows[:, None], cols[None, :]]


def _stats64(x, eps, bug=None):
    xd = x.astype(np.float64)
    mean = xd.mean(axis=(2, 3), keepdims=True)
    n = x.shape[2] * x.shape[3]
    var = ((xd - mean) ** 2).sum(axis=(2, 3), keepdims=True) / (n - 1 if bug == "unbiased" and n > 1 else n)
    return xd, mean, 1.0 / np.sqrt(var + eps)


def _pmax(a):
    return np.abs(a).max(axis=(2, 3), initial=0.0)


def reference(x, *, up=1, sub=1, rpad=0, cs=None, res=None, slope=None, second=None, eps=EPS, bug=None):
    """The whole chain in float64 on the float32 plane x: InstanceNorm (biased variance) * chan_scale, index map, + residual,
    PReLU.  `second` = (sub2, cs2 or None).  Returns y, bound [N][C], scale / shift [N][C] in double and, with `second`, y2 and
    bound2."""
    xd, mean, rstd = _stats64(x, eps, bug)
    C = x.shape[1]
    csd = np.ones((1, C, 1, 1)) if cs is None else cs.astype(np.float64).reshape(1, C, 1, 1)
    t = (xd - mean) * rstd * csd
    e = 2.0 ** -23 * (_pmax(xd) * (rstd * np.abs(csd))[:, :, 0, 0] + _pmax(t) + 1.0)
    maps = index_maps(x.shape[2], x.shape[3], up, sub, rpad, bug)
    y = gather(t, maps)
    if res is not None:
        r = t + res.astype(np.float64)
        e = e + 2.0 ** -24 * _pmax(r)
        y = gather(r, maps)
    if slope is not None:
        y = np.where(y >= 0, y, y * float(slope))
        e = e + 2.0 ** -24 * _pmax(y)
    out = dict(y=y, bound=e, scale=(rstd * csd)[:, :, 0, 0], shift=(-mean * rstd * csd)[:, :, 0, 0])
    if second is not None:
        sub2, cs2 = second
        if bug == "y2_chan_scale":
            cs2 = cs
        c2 = np.ones((1, C, 1, 1)) if cs2 is None else cs2.astype(np.float64).reshape(1, C, 1, 1)
        t2 = (xd - mean) * rstd * c2
        out["y2"] = gather(t2, index_maps(x.shape[2], x.shape[3], 1, sub2, 0, bug))
        out["bound2"] = 2.0 ** -23 * (_pmax(xd) * (rstd * np.abs(c2))[:, :, 0, 0] + _pmax(t2) + 1.0)
    return out


def emulate(x, *, up=1, sub=1, rpad=0, cs=None, res=None, slope=None, eps=EPS):
    """instnorm_bound.emulate_fma extended to the modes: what a correct implementation returns.  sc and sh rounded to float32
    once, the product and sum exact (float64) and rounded once, then the residual add and the slope multiply in float32."""
    xd, mean, rstd = _stats64(x, eps)
    C = x.shape[1]
    csd = np.ones((1, C, 1, 1)) if cs is None else cs.astype(np.float64).reshape(1, C, 1, 1)
    sc = (rstd * csd).astype(np.float32)
    sh = (-mean * (rstd * csd)).astype(np.float32)
    t = (xd * sc.astype(np.float64) + sh.astype(np.float64)).astype(np.float32)
    if res is not None:
        t = t + res
    y = gather(t, index_maps(x.shape[2], x.shape[3], up, sub, rpad))
    if slope is not None:
        y = np.where(y >= 0, y, y * np.float32(slope))
    return y.astype(np.float32)


def ref_args(c, t):
    """The keywords of `reference` / `emulate` for a case and its data (without `second`)."""
    m = mode_params(c["mode"])
    return dict(up=m["up"], sub=m["sub"], rpad=m["rpad"], cs=t["cs"], res=t["res"], slope=t["slope"])


def second_of(c, t):
    return None if c.get("second", "none") == "none" else ((1, None) if c["second"] == "s1" else (2, t["cs2"]))


def first_wrong(got, want, bound):
    """None, or (n, c, y, x, got, want, bound) of the first element further than its plane's bound from the reference."""
    bad = ~(np.abs(got.astype(np.float64) - want) <= bound[:, :, None, None])       # (a NaN is wrong)
    if not bad.any():
        return None
    n, c, y, x = (int(v) for v in np.argwhere(bad)[0])
    return n, c, y, x, float(got[n, c, y, x]), float(want[n, c, y, x]), float(bound[n, c])


def worst_ratio(got, want, bound):
    return float((np.abs(got.astype(np.float64) - want) / bound[:, :, None, None]).max())
