"""Integer-data cases for the forward convolution engines, importable without a GPU (tests/test_conv_exact_host.py checks the
generator and the arithmetic on the CPU, tests/test_gpu_conv_exact.py runs the cases on the engines).

Why integers: with activations in -4..4, filters in -2..2, bias / residual in -8..8, input scales that are powers of two and
slopes 0.25 / 0.5, every product and every partial sum of every engine is a binary fraction that fp32 holds exactly, the
Winograd transforms included (U = G g G^T is a multiple of 1/4, B^T d B and A^T m A only add).  Summation order, split-K,
stream-K fix-ups and the transforms then cannot change a bit: every engine must EQUAL the float64 reference, element by
element, and a failure names the first wrong (n, c, y, x).  `exactness_bound` is the guard that the ranges really are small
enough, evaluated per case.

Cases come from a deterministic greedy all-pairs generator, one factor table per engine: every pair of factor levels that the
engine's own rules allow (`_VALID`) appears in at least one case.  Tile edges are read from the kernel sources, not restated.
"""
import functools
import os
import random
import re
import zlib

import torch
import torch.nn.functional as F

from test_gpu_ops import ref_conv

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "deep-exemplar-based-video-colorization_amd", "csrc")
MAX_H, MAX_W = 40, 72           # nothing larger, stored or virtual
ACTS = {"none": (0, 0.0), "relu": (1, 0.0), "leaky": (3, 0.25), "prelu": (2, 0.25), "leaky_half": (3, 0.5)}
RESAMPLE = {"1/1": (1, 1), "2/1": (2, 1), "1/2": (1, 2)}        # in_up / in_sub, never both 2
REFUSALS = ("does not fit", "no configuration for cfg", "no tile configuration fits", "workspace too small")
SKIP_CAP = 0.20


# ---- tile edges, from the sources
def _src(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def _int_tuples(text):
    return [tuple(int(v) for v in m.split(",")) for m in re.findall(r"\{([\d,\s]+)\}", text)]


@functools.lru_cache(None)
def tile_tables():
    """kConvCfgs (wm, wn, rm, rn), the pixel-tile widths pick_tw chooses from, CONV_EPT_GEN, the image-input kernel's (TH, TW),
    conv_ws's (strip width, rows per step), kWinoShapes (wm, wn, kc, per_cu) and the tile-block row counts kTR."""
    host = _src("conv_mfma.hip")
    cfgs = _int_tuples(re.search(r"kConvCfgs\[5\] = \{(.*?)\};", _src("conv_kernel.h"), re.S).group(1))
    tw = re.search(r"int best = (\d+),.*?for \(int tw : \{([\d,\s]+)\}\)", host, re.S)
    tws = sorted({int(tw.group(1))} | {int(v) for v in tw.group(2).split(",")})
    ept = int(re.search(r"#define CONV_EPT_GEN (\d+)", _src("conv_kernel.h")).group(1))
    img = re.search(r"constexpr int TH = (\d+), TW = (\d+)", _src("conv_image.hip"))
    ws = _src("conv_ws.hip")
    ws_strip = int(re.search(r"a\.strips = cdiv\(d->W, (\d+)\)", ws).group(1))
    ws_ps = sorted(int(v) for v in re.search(r"const int ps = d->Cin == 32 \? (\d+) : (\d+);", ws).groups())
    wino = next(s for s in (host, _src("conv_wino_kernel.h")) if "kWinoShapes[4]" in s)
    shapes = _int_tuples(re.search(r"kWinoShapes\[4\] = \{(.*?)\};", wino, re.S).group(1))
    ktr = _int_tuples(re.search(r"kTR\[4\] = (\{.*?\});", wino).group(1))[0]
    sk = sorted(int(v) for v in re.search(r"tile configurations (\d), (\d) and (\d) \(cfg 34\.\.36\)", host).groups())
    assert len(cfgs) == 5 and len(shapes) == 4 and len(ktr) == 4, (cfgs, shapes, ktr)
    return dict(cfgs=cfgs, tws=tws, ept_gen=ept, image=(int(img.group(1)), int(img.group(2))), ws=(ws_strip, ws_ps), wino=shapes,
                ktr=ktr, sk_cfgs=sk)


def _levels(edges, cap, odd, lo=1):
    """1, 2, 3, one below / at / one above every tile edge, and an odd value in the 20s."""
    s = {1, 2, 3, odd}
    for e in edges:
        s |= {e - 1, e, e + 1}
    return sorted(v for v in s if lo <= v <= cap)


@functools.lru_cache(None)
def geometry_levels(engine):
    t = tile_tables()
    tiles = lambda ids: sorted({t["cfgs"][i][1] * t["cfgs"][i][3] * (32 // tw) for i in ids for tw in t["tws"]})    # noqa: E731
    if engine in ("direct", "per_image"):
        return _levels(tiles(range(5)), MAX_H, 23), _levels(t["tws"], MAX_W, 27)
    if engine == "streamk":
        return _levels(tiles(t["sk_cfgs"]), MAX_H, 23), _levels(t["tws"], MAX_W, 27)
    if engine == "image":
        return _levels([t["image"][0]], MAX_H, 23), _levels([t["image"][1], 2 * t["image"][1]], MAX_W, 27)
    if engine == "ws":
        return _levels(t["ws"][1] + [2 * max(t["ws"][1])], MAX_H, 23), _levels([t["ws"][0], 2 * t["ws"][0]], MAX_W, 27)
    # Winograd: 2x2 outputs per tile, tile blocks of tr * wn x 32 / tr tiles
    hs = {2 * tr * s[1] for tr in t["ktr"] for s in t["wino"]}
    ws_ = {2 * (32 // tr) for tr in t["ktr"]}
    lo = 2 if engine == "wino_pool" else 1
    return _levels(hs, MAX_H, 23, lo), _levels(ws_, MAX_W, 27, lo)


# ---- the engines' own rules
def vdim(S, up, sub):
    return S * 2 if up == 2 else ((S + 1) // 2 if sub == 2 else S)


def _geometry_ok(c, pad):
    up, sub = RESAMPLE[c.get("resample", "1/1")]
    VH, VW = vdim(c["H"], up, sub), vdim(c["W"], up, sub)
    if VH > MAX_H or VW > MAX_W:
        return False
    return not (c.get("pad_mode", 0) == 1 and pad > 0 and not (pad < VH and pad < VW))      # reflect needs H, W > pad


def pick_tw(OW):
    tws = tile_tables()["tws"]
    return min(sorted(tws, reverse=True), key=lambda tw: -(-OW // tw) * tw)


def direct_cfg_fits(c):
    """conv_cfg_fits: the run-time-geometry (stride 2) kernel stages CONV_EPT_GEN elements per thread."""
    cfg = c["cfg"] % 16
    if c["stride"] == 1 or c["cfg"] < 0:
        return True
    t = tile_tables()
    up, sub = RESAMPLE[c["resample"]]
    OW = (vdim(c["W"], up, sub) + 2 * c["dil"] - (2 * c["dil"] + 1)) // 2 + 1
    tw = pick_tw(OW)
    _, wn, _, rn = t["cfgs"][cfg]
    ph = wn * rn * (32 // tw)
    ext = 2 * c["dil"] + 1
    return 8 * ((ph - 1) * 2 + ext) * ((tw - 1) * 2 + ext) <= t["ept_gen"] * 256


def _valid_direct(c):
    if c["ks"] == 1 and (c["stride"] != 1 or c["dil"] != 1 or c["pad_mode"] == 1):
        return False
    return _geometry_ok(c, c["dil"] if c["ks"] == 3 else 0) and direct_cfg_fits(c)


def _valid_streamk(c):
    """The stream-K "plain layer" rule: stride 1, no fused input transform, Cin a multiple of the chunk, Cout of the tile."""
    if c["ks"] == 1 and (c["dil"] != 1 or c["pad_mode"] == 1 or c["Cin"] % 16):
        return False
    return _geometry_ok(c, c["dil"] if c["ks"] == 3 else 0)


def _cdiv(a, b):
    return -(-a // b)


def wino_plan_exists(Cin, Cout, cfg, split_k):
    """wino_plan's feasibility: a workgroup shape whose channel block divides Cout and whose chunk count takes the split."""
    for m, (wm, _wn, kc, _) in enumerate(tile_tables()["wino"]):
        if (cfg >= 0 and cfg // 4 != m) or (cfg < 0 and m == 3) or Cout % (32 * wm):
            continue
        nch = Cin // kc
        if split_k <= 1 or (split_k <= nch // 2 and _cdiv(nch, _cdiv(nch, split_k)) == split_k):
            return True
    return False


def _valid_wino(c):
    if c.get("defer") and (c["res"] or c["dst"] != "dense" or c["xin"] != "dense"):
        return False        # ops defers only a launch that writes no tensor and carries no residual
    return _geometry_ok(c, c["dil"]) and wino_plan_exists(c["Cin"], c["Cout"], c["cfg"], c["split_k"])


def _valid_dual(c):
    if c["CA"] == c["CB"]:
        return False
    if 2 in (c["upA"], c["upB"]) and (c["H"] % 2 or c["W"] % 2):      # H, W: the virtual size both inputs share
        return False
    return _geometry_ok(dict(c, resample="1/1"), c["dil"])


_COMMON = dict(N=[1, 3], res=[False, True], act=list(ACTS), dst=["dense", "slice"], xin=["dense", "strided"])


def _some(levels, *keep):
    """The variants sweep a part of the family's geometry levels."""
    assert set(keep) <= set(levels), (keep, levels)
    return [v for v in levels if v in keep]


def _factors(engine):
    Hs, Ws = geometry_levels(engine)
    geo = dict(H=Hs, W=Ws)
    pm, rs = [0, 1], list(RESAMPLE)
    if engine == "direct":
        # (Cin 40 is five chunks of eight: an odd chunk count under a forced split, beside the issue's levels)
        return dict(_COMMON, **geo, ks=[1, 3], stride=[1, 2], dil=[1, 2], pad_mode=pm, resample=rs, affine=[False, True],
                    in_prelu=[False, True], Cin=[3, 7, 8, 20, 40, 64], Cout=[4, 36, 64, 128], cfg=[-1, 0, 1, 2, 3, 4, 16, 18, 20],
                    split_k=[0, 2, 3])
    if engine == "streamk":
        return dict(_COMMON, **geo, ks=[1, 3], dil=[1, 2], pad_mode=pm, resample=rs, Cin=[8, 40, 64], Cout=[64, 128],
                    cfg=[34, 35, 36], per_cu=[1, 2])
    if engine == "image":
        # (a residual sends the layer to the general engine, so there is none here)
        return dict(N=[1, 3], act=list(ACTS), dst=_COMMON["dst"], xin=_COMMON["xin"], **geo, io=[(3, 64), (7, 32)], pad_mode=pm,
                    affine=[False, True], bias=[False, True])
    if engine == "ws":
        return dict(N=[1, 3], act=list(ACTS), dst=_COMMON["dst"], xin=_COMMON["xin"], **geo, Cin=[32, 64, 128], Cout=[64, 128],
                    bias=[False, True])
    if engine == "wino":
        return dict(_COMMON, **geo, dil=[1, 2], pad_mode=pm, resample=rs, Cin=[8, 24, 40, 64], Cout=[64, 128, 192],
                    cfg=list(range(-1, 16)), split_k=[0, 1, 2, 3], defer=[False, True])
    if engine == "wino_pool":
        return dict(N=[1, 3], act=list(ACTS), H=_some(Hs, 2, 3, 8, 9, 17, 23), W=_some(Ws, 2, 3, 9, 16, 27, 33, 64), pad_mode=pm,
                    Cin=[8, 24, 40, 64], Cout=[64, 128], want_full=[False, True])
    if engine == "wino_dual":
        # (H, W: the virtual size both inputs share; an upsampled input makes it even)
        return dict(N=[1, 3], act=list(ACTS), H=_some(Hs, 2, 3, 4, 8, 9, 16, 23) + [18], W=_some(Ws, 2, 3, 8, 17, 27, 32, 64) + [34], dil=[1, 2], pad_mode=pm,
                    upA=[1, 2], upB=[1, 2], CA=[8, 24, 40], CB=[8, 16, 64], Cout=[64, 128])
    if engine == "wino_group":
        return dict(N=[1, 3], act=list(ACTS), items=[2, 3, 4], first=list(range(len(GROUP_ITEMS))), pad_mode=pm, defer=[False, True])
    if engine == "per_image":
        return dict(N=[2, 3], res=[False, True], act=list(ACTS), dst=_COMMON["dst"], H=_some(Hs, 1, 2, 3, 8, 9, 17),
                    W=_some(Ws, 1, 3, 8, 9, 16, 27, 33), ks=[1, 3], Cin=[8, 20, 64], Cout=[4, 36, 64], cfg=[-1, 1, 3, 18],
                    split_k=[0, 2])
    raise KeyError(engine)


# items of the grouped launch: (Cin, Cout, H, W, in_up); a case takes `items` consecutive ones starting at `first`
GROUP_ITEMS = [(8, 64, 5, 9, 1), (64, 64, 16, 17, 1), (40, 128, 9, 33, 2), (24, 192, 3, 2, 1), (64, 128, 2, 7, 1), (16, 64, 20, 36, 1)]
_VALID = dict(direct=_valid_direct, streamk=_valid_streamk, image=lambda c: _geometry_ok(c, 1), ws=lambda c: True, wino=_valid_wino,
              wino_pool=lambda c: _geometry_ok(c, 1), wino_dual=_valid_dual, wino_group=lambda c: True, per_image=lambda c: True)
ENGINES = tuple(_VALID)


# ---- greedy all-pairs
def _complete(names, factors, valid, fixed, rng, tries):
    for _ in range(tries):
        c = {n: fixed[n] if n in fixed else rng.choice(factors[n]) for n in names}
        if valid(c):
            return c
    return None


def all_pairs(factors, valid, seed, candidates=10):
    """Cases (dicts) such that every pair of levels that some valid case can hold is in one of them; and the set of pairs no
    valid case was found for (600 random completions each).  Deterministic for a given seed."""
    rng = random.Random(seed)
    names = sorted(factors)
    pairs = [(a, i, b, j) for x, a in enumerate(names) for b in names[x + 1:] for i in range(len(factors[a]))
             for j in range(len(factors[b]))]
    rng.shuffle(pairs)
    uncovered, impossible, cases = set(pairs), set(), []
    key = lambda c: {(a, factors[a].index(c[a]), b, factors[b].index(c[b])) for x, a in enumerate(names) for b in names[x + 1:]}   # noqa: E731
    for p in pairs:
        if p not in uncovered:
            continue
        fixed = {p[0]: factors[p[0]][p[1]], p[2]: factors[p[2]][p[3]]}
        best, best_n = None, -1
        for _ in range(candidates):
            c = _complete(names, factors, valid, fixed, rng, 60)
            if c is None:
                break
            n = len(key(c) & uncovered)
            if n > best_n:
                best, best_n = c, n
        if best is None:
            best = _complete(names, factors, valid, fixed, rng, 600)
            if best is None:
                uncovered.discard(p)
                impossible.add(p)
                continue
        uncovered -= key(best)
        cases.append(best)
    return cases, impossible


def _case_id(engine, k, c):
    bits = [engine, f"{k:03d}"]
    if "ks" in c:
        bits.append(f"k{c['ks']}s{c.get('stride', 1)}d{c.get('dil', 1)}")
    elif "dil" in c:
        bits.append(f"d{c['dil']}")
    if "io" in c:
        bits.append("%dto%d" % c["io"])
    elif "Cin" in c:
        bits.append(f"{c['Cin']}to{c['Cout']}")
    elif "CA" in c:
        bits.append(f"{c['CA']}+{c['CB']}to{c['Cout']}")
    if "H" in c:
        bits.append(f"{c['H']}x{c['W']}")
    if "cfg" in c:
        bits.append(f"cfg{c['cfg']}")
    return "-".join(bits)


@functools.lru_cache(None)
def generate(engine):
    """(cases, pairs no valid case holds) of an engine; a case is a dict of its factor levels + `engine`, `id`, `seed`."""
    factors = _factors(engine)
    cases, impossible = all_pairs(factors, _VALID[engine], zlib.crc32(engine.encode()))
    out = []
    for k, c in enumerate(cases):
        cid = _case_id(engine, k, c)
        out.append(dict(c, engine=engine, id=cid, seed=zlib.crc32(cid.encode()) % (1 << 31)))
    return out, impossible


def cases(engine):
    return generate(engine)[0]


def factors(engine):
    return _factors(engine)


def pair_allowed(engine, a, va, b, vb, tries=3000):
    """Independent of the generator's own search: is there a valid case with factor a at va and b at vb?"""
    f = _factors(engine)
    return _complete(sorted(f), f, _VALID[engine], {a: va, b: vb}, random.Random(12345), tries) is not None


# ---- data
def _ints(g, lo, hi, *shape):
    return torch.randint(lo, hi + 1, shape, generator=g).float()


def conv_geometry(c):
    """(ks, stride, dil, pad, pad_mode, in_up, in_sub) of a single-convolution case."""
    e = c["engine"]
    ks, stride, dil = c.get("ks", 3), c.get("stride", 1), c.get("dil", 1)
    up, sub = RESAMPLE[c.get("resample", "1/1")]
    return ks, stride, dil, (dil if ks == 3 else 0), c.get("pad_mode", 0), up, sub if e != "wino_dual" else 1


def out_hw(H, W, ks, stride, dil, pad, up, sub):
    ext = dil * (ks - 1) + 1
    return (vdim(H, up, sub) + 2 * pad - ext) // stride + 1, (vdim(W, up, sub) + 2 * pad - ext) // stride + 1


def make_inputs(c):
    """CPU float32 tensors of a single-convolution case (direct, streamk, image, ws, wino, wino_pool, per_image): x, w, b, res,
    scale, shift, slope (None where the case has none), and its geometry."""
    g = torch.Generator().manual_seed(c["seed"])
    Cin, Cout = c["io"] if "io" in c else (c["Cin"], c["Cout"])
    N, H, W = c["N"], c["H"], c["W"]
    ks, stride, dil, pad, pad_mode, up, sub = conv_geometry(c)
    OH, OW = out_hw(H, W, ks, stride, dil, pad, up, sub)
    t = dict(Cin=Cin, Cout=Cout, OH=OH, OW=OW, geom=(ks, stride, dil, pad, pad_mode, up, sub))
    t["x"] = _ints(g, -4, 4, N, Cin, H, W)
    t["w"] = _ints(g, -2, 2, *((N,) if c["engine"] == "per_image" else ()), Cout, Cin, ks, ks)
    t["b"] = _ints(g, -8, 8, Cout) if c.get("bias", True) else None
    t["res"] = _ints(g, -8, 8, N, Cout, OH, OW) if c.get("res") else None
    t["scale"] = torch.tensor([0.5, 1.0, 2.0])[torch.randint(0, 3, (N * Cin,), generator=g)] if c.get("affine") else None
    t["shift"] = _ints(g, -2, 2, N * Cin) if c.get("affine") else None
    t["slope"] = torch.tensor([0.25]) if c.get("in_prelu") else None
    t["act"], t["act_slope"] = ACTS[c["act"]]
    return t


def reference(c, t):
    """float64: the output, and its 2x2 max pool for the pool form."""
    ks, stride, dil, pad, pad_mode, up, sub = t["geom"]
    one = lambda x, w, res, sc, sh: ref_conv(x, w, t["b"], ks, stride, dil, pad, pad_mode, up, sub, sc, sh, t["slope"], res, t["act"],  # noqa: E731
                                             t["act_slope"])
    if c["engine"] == "per_image":
        y = torch.cat([one(t["x"][n:n + 1], t["w"][n], None if t["res"] is None else t["res"][n:n + 1], None, None)
                       for n in range(c["N"])])
    else:
        y = one(t["x"], t["w"], t["res"], t["scale"], t["shift"])
    return (y, F.max_pool2d(y, 2, 2)) if c["engine"] == "wino_pool" else y


def make_dual(c):
    g = torch.Generator().manual_seed(c["seed"])
    N, H, W = c["N"], c["H"], c["W"]
    t = dict(xA=_ints(g, -4, 4, N, c["CA"], H // c["upA"], W // c["upA"]), xB=_ints(g, -4, 4, N, c["CB"], H // c["upB"], W // c["upB"]),
             wA=_ints(g, -2, 2, c["Cout"], c["CA"], 3, 3), wB=_ints(g, -2, 2, c["Cout"], c["CB"], 3, 3),
             bA=_ints(g, -8, 8, c["Cout"]), bB=_ints(g, -8, 8, c["Cout"]))
    t["act"], t["act_slope"] = ACTS[c["act"]]
    return t


def ref_dual(c, t):
    """The dual form: the sum of two reference convolutions (the second one's output is the first one's residual)."""
    d = c["dil"]
    yB = ref_conv(t["xB"], t["wB"], t["bB"], 3, 1, d, d, c["pad_mode"], c["upB"], 1, None, None, None, None, 0, 0.0)
    return ref_conv(t["xA"], t["wA"], t["bA"], 3, 1, d, d, c["pad_mode"], c["upA"], 1, None, None, None, yB, t["act"], t["act_slope"])


def make_group(c):
    g = torch.Generator().manual_seed(c["seed"])
    items = []
    for k in range(c["items"]):
        Cin, Cout, H, W, up = GROUP_ITEMS[(c["first"] + k) % len(GROUP_ITEMS)]
        items.append(dict(x=_ints(g, -4, 4, c["N"], Cin, H, W), w=_ints(g, -2, 2, Cout, Cin, 3, 3), b=_ints(g, -8, 8, Cout), up=up))
    return items


def ref_group(c, items):
    a, s = ACTS[c["act"]]
    return [ref_conv(i["x"], i["w"], i["b"], 3, 1, 1, 1, c["pad_mode"], i["up"], 1, None, None, None, None, a, s) for i in items]


# ---- float32 restatements (CPU): the arithmetic the engines do, in plain torch
def map_virtual(p, V, pad_mode, axis):
    """Virtual coordinate -> source coordinate in 0..V-1, or -1 where the tap reads a zero (ReflectionPad2d otherwise)."""
    if 0 <= p < V:
        return p
    if pad_mode == 0:
        return -1
    return -p if p < 0 else 2 * (V - 1) - p


def padded_virtual(x, pad, pad_mode, up, sub, index_map=map_virtual):
    """The virtual input (every 2nd row / column, or nearest x2) with `pad` rows / columns on every side, as a gather."""
    def axis(S, name):
        V = vdim(S, up, sub)
        v = [index_map(p, V, pad_mode, name) for p in range(-pad, V + pad)]
        return torch.tensor([-1 if i < 0 else (i // 2 if up == 2 else i * 2 if sub == 2 else i) for i in v])
    r, q = axis(x.shape[2], "y"), axis(x.shape[3], "x")
    P = x[:, :, r.clamp_min(0)][:, :, :, q.clamp_min(0)]
    return P * (r >= 0).to(x.dtype).view(1, 1, -1, 1) * (q >= 0).to(x.dtype).view(1, 1, 1, -1)


def _finish(y, b, res, act, act_slope):
    if b is not None:
        y = y + b.to(y.dtype).view(1, -1, 1, 1)
    if res is not None:
        y = y + res.to(y.dtype)
    if act == 1:
        y = torch.relu(y)
    elif act in (2, 3):
        y = torch.where(y >= 0, y, y * act_slope)
    return y


def direct_taps(x, w, b, ks, stride, dil, pad, pad_mode, up, sub, scale, shift, slope, res, act, act_slope, *, dtype=torch.float32,
                index_map=map_virtual, wrong_tap=None):
    """The direct sum, tap by tap, in `dtype`.  wrong_tap = (ky, kx, ox): that tap reads the neighbouring column for the outputs
    of column ox (the sensitivity check of the sweep; never set by a comparison)."""
    v = x.to(dtype)
    N, C = v.shape[:2]
    if scale is not None:
        v = v * scale.to(dtype).view(N, C, 1, 1) + shift.to(dtype).view(N, C, 1, 1)
    if slope is not None:
        v = torch.where(v >= 0, v, v * slope.to(dtype))
    P = padded_virtual(v, pad, pad_mode, up, sub, index_map)
    OH, OW = out_hw(x.shape[2], x.shape[3], ks, stride, dil, pad, up, sub)
    y = torch.zeros(N, w.shape[0], OH, OW, dtype=dtype)
    for ky in range(ks):
        for kx in range(ks):
            win = P[:, :, ky * dil: ky * dil + (OH - 1) * stride + 1: stride, kx * dil: kx * dil + (OW - 1) * stride + 1: stride]
            if wrong_tap is not None and wrong_tap[:2] == (ky, kx):
                win = win.clone()
                win[..., wrong_tap[2]] = P[:, :, ky * dil: ky * dil + (OH - 1) * stride + 1: stride, kx * dil + wrong_tap[2] * stride + 1]
            y = y + torch.einsum("oc,nchw->nohw", w[:, :, ky, kx].to(dtype), win)
    return _finish(y, b, res, act, act_slope)


def direct_conv2d(x, w, b, ks, stride, dil, pad, pad_mode, up, sub, scale, shift, slope, res, act, act_slope, *, dtype=torch.float32):
    """The same through ATen's conv2d in `dtype`."""
    v = x.to(dtype)
    N, C = v.shape[:2]
    if scale is not None:
        v = v * scale.to(dtype).view(N, C, 1, 1) + shift.to(dtype).view(N, C, 1, 1)
    if slope is not None:
        v = torch.where(v >= 0, v, v * slope.to(dtype))
    y = F.conv2d(padded_virtual(v, pad, pad_mode, up, sub), w.to(dtype), None, stride=stride, dilation=dil)
    return _finish(y, b, res, act, act_slope)


_G = [[1.0, 0.0, 0.0], [0.5, 0.5, 0.5], [0.5, -0.5, 0.5], [0.0, 0.0, 1.0]]
_BT = [[1.0, 0.0, -1.0, 0.0], [0.0, 1.0, 1.0, 0.0], [0.0, -1.0, 1.0, 0.0], [0.0, 1.0, 0.0, -1.0]]
_AT = [[1.0, 1.0, 1.0, 0.0], [0.0, 1.0, -1.0, -1.0]]


def winograd(x, w, b, dil, pad_mode, up, sub, res, act, act_slope, *, dtype=torch.float32, index_map=map_virtual, absolute=False):
    """F(2x2, 3x3) in `dtype`: U = G g G^T, V = B^T d B per 4x4 patch, M = sum over Cin of U * V, Y = A^T M A; a dilation-2
    layer as four dilation-1 problems, one per parity class of the padded input.  absolute=True: every operand and matrix by
    magnitude (the exactness guard's sum of |x'| |w'|), before bias / residual / activation."""
    mat = lambda m: torch.tensor(m, dtype=dtype).abs() if absolute else torch.tensor(m, dtype=dtype)      # noqa: E731
    G, BT, AT = mat(_G), mat(_BT), mat(_AT)
    v = x.to(dtype).abs() if absolute else x.to(dtype)
    U = torch.einsum("ia,ocab,jb->ocij", torch.tensor(_G, dtype=dtype), w.to(dtype), torch.tensor(_G, dtype=dtype))
    if absolute:
        U = U.abs()
    P = padded_virtual(v, dil, pad_mode, up, sub, index_map)
    N = x.shape[0]
    OH, OW = P.shape[2] - 2 * dil, P.shape[3] - 2 * dil
    y = torch.zeros(N, w.shape[0], OH, OW, dtype=dtype)
    for py in range(dil):
        for px in range(dil):
            D = P[:, :, py::dil, px::dil]                       # valid dilation-1 problem: outputs (dil * a + py, dil * c + px)
            oh, ow = D.shape[2] - 2, D.shape[3] - 2
            if oh <= 0 or ow <= 0:
                continue
            TY, TX = (oh + 1) // 2, (ow + 1) // 2
            D = F.pad(D, (0, 2 * TX + 2 - D.shape[3], 0, 2 * TY + 2 - D.shape[2]))
            d = D.unfold(2, 4, 2).unfold(3, 4, 2)              # [N, C, TY, TX, 4, 4]
            V = torch.einsum("ia,nctuab,jb->nctuij", BT, d, BT)
            M = torch.einsum("ocij,nctuij->notuij", U, V)
            Y = torch.einsum("ia,notuab,jb->notuij", AT, M, AT)            # [N, O, TY, TX, 2, 2]
            Y = Y.permute(0, 1, 2, 4, 3, 5).reshape(N, w.shape[0], 2 * TY, 2 * TX)[:, :, :oh, :ow]
            y[:, :, py::dil, px::dil] = Y
    return y if absolute else _finish(y, b, res, act, act_slope)


def exactness_bound(c, t=None):
    """max over outputs of sum |x'| |w'| (+ |bias| + |residual|), divided by the finest binary fraction q that can occur: below
    2^24 every partial sum in any order is an fp32 number.  q = 1/32 on the direct path (input scale 1/2, input PReLU 1/4, output
    slope 1/4), 1/4 * 1/4 on the Winograd path (U is a multiple of 1/4; output slope 1/4)."""
    e = c["engine"]
    if e == "wino_dual":
        t = t or make_dual(c)
        m = sum(winograd(t["x" + s], t["w" + s], None, c["dil"], c["pad_mode"], c["up" + s], 1, None, 0, 0.0, dtype=torch.float64,
                         absolute=True) for s in "AB").max().item() + 16
        return m * 16
    if e == "wino_group":
        return max(winograd(i["x"], i["w"], None, 1, c["pad_mode"], i["up"], 1, None, 0, 0.0, dtype=torch.float64,
                            absolute=True).max().item() + 8 for i in (t or make_group(c))) * 16
    t = t or make_inputs(c)
    ks, stride, dil, pad, pad_mode, up, sub = t["geom"]
    if e in ("wino", "wino_pool"):
        return (winograd(t["x"], t["w"], None, dil, pad_mode, up, sub, None, 0, 0.0, dtype=torch.float64, absolute=True).max().item() + 16) * 16
    ab = lambda v: None if v is None else v.abs()      # noqa: E731
    w = t["w"].abs().amax(0) if e == "per_image" else t["w"].abs()
    m = ref_conv(t["x"].abs(), w, ab(t["b"]), ks, stride, dil, pad, pad_mode, up, sub, ab(t["scale"]), ab(t["shift"]), None,
                 ab(t["res"]), 0, 0.0)
    return m.max().item() * 32


# ---- comparison
def mismatch(got, want):
    """None if `got` equals `want` bit for bit (a NaN never does), else the count of wrong elements and the first one."""
    got, want = got.detach().cpu(), want.detach().cpu().to(got.dtype)
    if got.shape != want.shape:
        return f"shape {tuple(got.shape)} instead of {tuple(want.shape)}"
    bad = ~(got == want)
    if not bad.any():
        return None
    first = tuple(bad.nonzero()[0].tolist())
    return f"{int(bad.sum())} of {bad.numel()} elements wrong, first at (n, c, y, x) = {first}: got {got[first].item()!r}, want {want[first].item()!r}"


def assert_exact(got, want, what):
    m = mismatch(got, want)
    assert m is None, f"{what}: {m}"
