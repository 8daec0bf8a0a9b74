"""One-hot cases for NonlocalWeightedAverage (csrc/nonlocal_avg.hip), importable without a GPU
(tests/test_nonlocal_avg_exact_host.py checks the generator and the reference on the CPU, tests/test_gpu_nonlocal_avg_exact.py
runs the cases on the kernel).

Why they are exact: features are integers in [-3, 3], ab values integers in [-110, 110] and alpha = 2^-8.  Every affinity
<U_i, U_j> is an integer below 2^24 (`exactness_guard`), so the fp32 MFMA accumulates it exactly in any order.  The kernel's
constant c = log2(e) / alpha is about 369, a key that is not maximal lies at least 1 below its row's maximum and its weight is
exp2(<= -369) = 0 from the raw exponential instruction, the maximum's weight is exp2(0) = 1.  So L is the number of maximal
keys, Y the integer sum of their ab values, both exact in every partial state and through the merge, and

    out = float32(sum of ab over the maximal keys) / float32(count)

bit for bit where count is a power of two (a divide and a reciprocal-multiply agree there), within 1 ulp otherwise.  Which keys
are maximal is decided by the float64 reference below, never by the kernel.

The data raise one channel at "beacon" keys: every position carries a 1 in one of two type channels, beacon A carries a 3 in
the first and beacon B a 3 in the second over their patch windows, the other channels hold a sparse +-1.  A row follows the
beacon of the type its own patch holds more of; beacon A is what a case places (key 0, the last key, the first key of the
ragged tile, a tie of two or three copies ...).  Small integers also tie by accident, so a placement that asks for one
maximum or for a pair redraws an image (at most DRAWS times) until the reference finds only power-of-two counts in it.
`solved` reads from the reference's maximal-key sets which placements (INVENTORY) a case really contains.

The graded regime reuses a dozen geometries with alpha = float32(log2 e): c rounds to exactly 1.0f, weights are powers of two
and the keys below the maximum matter.  It is judged by the rule of test_matches_float64_restatement.
"""
import functools
import os
import re
import zlib

import numpy as np
import torch

import nlwa_reference as R
from conv_exact_cases import all_pairs
from dvc_amd.nonlocal_avg import _out_size, _src_scale_factor, _src_scale_size

SRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "deep-exemplar-based-video-colorization_amd", "csrc",
                   "nonlocal_avg.hip")
ALPHA_EXACT = 2.0 ** -8
ALPHA_GRADED = float(np.float32(np.log2(np.e)))
LOG2E = 1.4426950408889634                      # the constant dvc_nlwa_fwd divides by alpha, in double
assert np.float32(LOG2E / ALPHA_GRADED) == np.float32(1.0)      # the kernel's c is exactly 1.0f in the graded regime
F_MAX, AB_MAX = 3, 110

SIZES = [(1, 1), (1, 2), (7, 9), (8, 8), (5, 13), (1, 127), (8, 16), (3, 43), (15, 17), (16, 16), (1, 257), (45, 64), (46, 64)]
PATCHES = [1, 3, 5, 7]
CHANNELS = [1, 3, 31, 32, 33, 64, 65]
BATCHES = [1, 2, 3]
SCALES = [1, 0.5, 0.25, 0.4]                    # 0.4: source step 2.5, the non-integer ratio
FSIZES = ["smaller", "equal", "larger"]         # the feature against the resized map
PLACES = ["noise", "const", "first", "last", "ragged_first", "upper_half", "tie_pair", "tie_split", "tie3", "later_tile",
          "earlier_tile"]
FACTORS = dict(size=SIZES, k=PATCHES, C=CHANNELS, B=BATCHES, sf=SCALES, fsize=FSIZES, place=PLACES)
BIG_N = 2880                                    # from here on a workgroup sweeps more than one key tile


# ---- the kernel's tiling, from its source
@functools.lru_cache(None)
def tile_constants():
    with open(SRC) as f:
        text = f.read()
    return {n: int(re.search(r"#define %s (\d+)" % n, text).group(1)) for n in ("NL_QB", "NL_KT", "NL_KC", "NL_WG_TARGET")}


def plan(N):
    """nlwa_plan's split of the keys: ntiles, nqb, nsplit and the tile range [t0, t1) of every split."""
    t = tile_constants()
    ntiles, nqb = -(-N // t["NL_KT"]), -(-N // t["NL_QB"])
    nsplit = min(ntiles, max(1, t["NL_WG_TARGET"] // nqb))
    ranges = [(sp * ntiles // nsplit, (sp + 1) * ntiles // nsplit) for sp in range(nsplit)]
    split_of = [sp for sp, (t0, t1) in enumerate(ranges) for _ in range(t0, t1)]
    return dict(KT=t["NL_KT"], ntiles=ntiles, nqb=nqb, nsplit=nsplit, ranges=ranges, split_of=split_of)


# ---- cases
def _valid(c):
    N = c["size"][0] * c["size"][1]
    if N >= BIG_N and not (c["C"] <= 4 and c["k"] == 1):        # the large maps stay cheap for the float64 reference
        return False
    if c["place"] in ("later_tile", "earlier_tile") and N < BIG_N:
        return False
    return True


def _sf_tag(sf):
    return {1: "1", 0.5: "h", 0.25: "q", 0.4: "p4"}[sf]


@functools.lru_cache(None)
def generate():
    """(exact cases, pairs of levels no valid case holds); a case is a dict of its levels + N, id, seed."""
    cases, impossible = all_pairs(FACTORS, _valid, zlib.crc32(b"nlwa_exact"))
    out = []
    for i, c in enumerate(cases):
        H, W = c["size"]
        cid = f"{i:03d}-{H}x{W}-k{c['k']}-c{c['C']}-b{c['B']}-sf{_sf_tag(c['sf'])}-{c['fsize']}-{c['place']}"
        out.append(dict(c, H=H, W=W, N=H * W, id=cid, seed=zlib.crc32(cid.encode()) % (1 << 31), alpha=ALPHA_EXACT, graded=False))
    return out, impossible


def exact_cases():
    return generate()[0]


@functools.lru_cache(None)
def graded_cases():
    """A dozen of the exact list's geometries (the first case that meets each wish), with graded data and alpha."""
    wishes = [lambda c: c["N"] == 2880, lambda c: c["N"] == 2944, lambda c: c["N"] == 1, lambda c: c["N"] == 2,
              lambda c: c["k"] == 7 and c["C"] == 65, lambda c: c["k"] == 7 and c["W"] < 7, lambda c: c["k"] == 5 and c["C"] == 33,
              lambda c: c["k"] == 3 and c["C"] == 32, lambda c: c["N"] == 256 and c["k"] > 1, lambda c: c["N"] == 257,
              lambda c: c["N"] == 255 and c["B"] == 3, lambda c: c["N"] == 127, lambda c: c["N"] == 128 and c["fsize"] == "smaller",
              lambda c: c["N"] == 64 and c["sf"] == 0.4]
    picked = []
    for wish in wishes:
        c = next((c for c in exact_cases() if wish(c) and c not in picked), None)
        if c is not None:
            picked.append(c)
    out = []
    for c in picked:
        cid = "g" + c["id"].rsplit("-", 1)[0]
        out.append(dict(c, place="graded", id=cid, seed=zlib.crc32(cid.encode()) % (1 << 31), alpha=ALPHA_GRADED, graded=True))
    return out


# ---- geometry of a case's inputs
def _x_in(n, sf):
    """An x_lab extent that F.interpolate(scale_factor=sf) turns into n, with a remainder where sf allows one."""
    for cand in ({1: n, 0.5: 2 * n + 1, 0.25: 4 * n + 3}.get(sf, 0), *range(1, 8 * n + 8)):
        if cand >= 1 and _out_size(cand, sf) == n:
            return cand
    raise AssertionError((n, sf))


def _f_in(n, fsize):
    return {"smaller": max(1, (2 * n + 2) // 3), "equal": n, "larger": 2 * n + 1}[fsize]


def nearest_index(n_out, n_in, scale, rounding=False):
    """ATen's nearest source index, min(floor(dst * scale), in - 1) in float32 as the prep launch computes it.
    rounding=True is the wrong rule of the sensitivity check."""
    v = np.arange(n_out, dtype=np.float32) * np.float32(scale)
    if rounding:
        v = v + np.float32(0.5)
    return np.minimum(np.floor(v).astype(np.int64), n_in - 1)


def resize_indices(c, rounding=False):
    """(x_lab rows, x_lab columns, feature rows, feature columns) that the H x W map reads."""
    H, W = c["H"], c["W"]
    sx = _src_scale_factor(c["sf"])
    Hx, Wx, Hf, Wf = _x_in(H, c["sf"]), _x_in(W, c["sf"]), _f_in(H, c["fsize"]), _f_in(W, c["fsize"])
    return (nearest_index(H, Hx, sx, rounding), nearest_index(W, Wx, sx, rounding),
            nearest_index(H, Hf, _src_scale_size(Hf, H), rounding), nearest_index(W, Wf, _src_scale_size(Wf, W), rounding))


# ---- data
def beacon_keys(place, N):
    """The keys beacon A is raised at."""
    pl = plan(N)
    KT, nt = pl["KT"], pl["ntiles"]
    multi = next(((t0, t1) for t0, t1 in pl["ranges"] if t1 - t0 >= 2), (nt - 1, nt))
    if place == "first":
        keys = [0]
    elif place == "last":
        keys = [N - 1]
    elif place == "ragged_first":
        keys = [(nt - 1) * KT]
    elif place == "upper_half":
        keys = [(nt // 2) * KT + KT // 2 + 37]
    elif place == "tie_pair":                   # lanes l and l ^ 32 hold the keys of a 64-key half with bit 2 clear / set
        a = max(0, min((nt // 2) * KT + 9, N - 6)) & ~4
        keys = [a, a + 4]
    elif place == "tie_split":
        keys = [1, N - 1]
    elif place == "tie3":
        keys = [2, N // 2, N - 3]
    elif place == "later_tile":
        keys = [(multi[1] - 1) * KT + 17]
    elif place == "earlier_tile":
        keys = [multi[0] * KT + 90]
    else:
        return []
    return sorted({min(max(k, 0), N - 1) for k in keys})


def _window(y, x, p, h, w):
    return [(dy, dx) for dy in range(-p, p + 1) for dx in range(-p, p + 1) if 0 <= y + dy < h and 0 <= x + dx < w]


def _beacon_map(rng, C, h, w, k, a_pos, b_pos):
    """[C, h, w] integers: type channels C-1 / 0 (a 1 in one of them per position), sparse integers elsewhere, 3 over the
    beacons' windows; the windows of the later A beacons are copies of the first one's, so their patches tie."""
    p = k // 2
    c0, c1 = C - 1, (0 if C >= 2 else None)
    M = np.zeros((C, h, w), dtype=np.int64)
    if c1 is None:
        ty = np.zeros((h, w), dtype=np.int64)
    elif k == 1:
        ty = rng.integers(0, 2, (h, w))
    else:                                       # two halves: few windows hold both types, so few rows tie by accident
        ty = np.broadcast_to(np.arange(w) >= (w + 1) // 2, (h, w)) if w > 1 else np.arange(h)[:, None] >= (h + 1) // 2
    M[c0] = ty == 0
    if c1 is not None:
        M[c1] = ty == 1
    if C > 2:                                   # +-1 on a quarter of a position's channels' worth: below the beacons' margin
        vals = rng.choice([-1, 1], (C - 2, h, w))
        M[1:C - 1] = np.where(rng.random((C - 2, h, w)) < 0.25 / (C - 2), vals, 0)
    for (y, x), ch, other in [(pos, c1, c0) for pos in b_pos] + [(pos, c0, c1) for pos in a_pos]:
        for dy, dx in _window(y, x, p, h, w):
            M[ch, y + dy, x + dx] = F_MAX
            if k == 1:                          # nothing else at a beacon: a row that follows it never ties with itself
                M[1:C - 1, y, x] = 0
            if other is not None and other != ch:
                M[other, y + dy, x + dx] = 0
    if a_pos:
        y0, x0 = a_pos[0]
        for y, x in a_pos[1:]:
            for dy, dx in _window(y, x, p, h, w):
                if 0 <= y0 + dy < h and 0 <= x0 + dx < w:
                    M[:, y + dy, x + dx] = M[:, y0 + dy, x0 + dx]
    return M


TIE_FREE = ("first", "last", "ragged_first", "upper_half", "tie_pair", "tie_split", "later_tile", "earlier_tile")
DRAWS = 8


def _draw_feature(c, rng, fy, fx):
    """One image's feature [C, Hf, Wf]."""
    C, H, W, N, k, place = c["C"], c["H"], c["W"], c["N"], c["k"], c["place"]
    Hf, Wf = _f_in(H, c["fsize"]), _f_in(W, c["fsize"])
    if place == "graded":
        K = C * k * k
        if K <= 3:
            return rng.integers(-2, 3, (C, Hf, Wf))
        return np.where(rng.random((C, Hf, Wf)) < min(1.0, 3.0 / K), rng.choice([-1, 1], (C, Hf, Wf)), 0)
    if place == "const":
        return np.ones((C, Hf, Wf), dtype=np.int64)
    f = rng.integers(-F_MAX, F_MAX + 1, (C, Hf, Wf))              # "noise", and the source pixels no position reads
    if place != "noise":
        keys = beacon_keys(place, N)
        kb = (N // 3) | 1
        b_keys = [kb] if N >= 8 and C >= 2 and kb not in keys else []
        on_source = c["fsize"] == "smaller"                         # an up-sampled feature: structure on its own grid
        pos = lambda j: (int(fy[j // W]), int(fx[j % W])) if on_source else (j // W, j % W)      # noqa: E731
        a_pos, b_pos = list(dict.fromkeys(pos(j) for j in keys)), [pos(j) for j in b_keys]
        if on_source:
            f = _beacon_map(rng, C, Hf, Wf, k, a_pos, b_pos)
        else:
            f[:, fy[:, None], fx[None, :]] = _beacon_map(rng, C, H, W, k, a_pos, b_pos)
    return f


@functools.lru_cache(None)
def _inputs(cid):
    c = next(c for c in exact_cases() + graded_cases() if c["id"] == cid)
    B, H, W = c["B"], c["H"], c["W"]
    iy, ix, fy, fx = resize_indices(c)
    x = np.random.default_rng(c["seed"]).integers(-AB_MAX, AB_MAX + 1, (B, 3, _x_in(H, c["sf"]), _x_in(W, c["sf"])))
    x = torch.from_numpy(x.astype(np.float32))
    f = []
    for b in range(B):
        # a placement that asks for one maximum or for a pair takes the first draw whose rows all have a power-of-two count of
        # maximal keys (by the reference; small integers tie by accident), so that the 1-ulp rule judges a minority of the cases
        draws = DRAWS if c["place"] in TIE_FREE else 1
        for d in range(draws):
            fb = torch.from_numpy(_draw_feature(c, np.random.default_rng([c["seed"], b, d]), fy, fx).astype(np.float32))[None]
            if d == 0:
                keep = fb
            if draws > 1 and is_pow2(exact_reference(dict(c, B=1), x[b:b + 1], fb)[1]).all():
                keep = fb
                break
        f.append(keep)
    f = torch.cat(f)
    assert f.abs().max() <= F_MAX and x.abs().max() <= AB_MAX
    return x, f


def make_inputs(c):
    """CPU float32 tensors x_lab [B, 3, Hx, Wx] and feature [B, C, Hf, Wf] of a case, all integers; computed once per case."""
    return _inputs(c["id"])


def exactness_guard(c, feature):
    """K * max|f|^2 (every affinity and every partial sum of one is an integer no larger) and N * max|ab| (the sum of ab over
    any key set): both must stay below 2^24."""
    K = c["C"] * c["k"] ** 2
    return K * float(feature.abs().max()) ** 2, c["N"] * AB_MAX


# ---- the exact reference
MUTATIONS = ("unmasked_tail", "replicate_border", "swap_ab", "round_resize", "row_mapping")


def _swapped_row(j):
    """The key a lane would take for key j's accumulator row with the 4 * hi and 8 * (r >> 2) terms exchanged."""
    o = j % 32
    return j - o + (o & 3) + 4 * (o >> 3) + 8 * ((o >> 2) & 1)


def resized(c, x_lab, feature, mutate=None):
    """float64 numpy: ab [B, 2, N] and the patches U [B, C k k, N] of the zero-bordered resized feature."""
    iy, ix, fy, fx = resize_indices(c, rounding=mutate == "round_resize")
    B, H, W, k = c["B"], c["H"], c["W"], c["k"]
    p = k // 2
    ab = x_lab.double().numpy()[:, 1:3][:, :, iy[:, None], ix[None, :]].reshape(B, 2, H * W)
    if mutate == "swap_ab":
        ab = ab[:, ::-1]
    fr = feature.double().numpy()[:, :, fy[:, None], fx[None, :]]
    fp = np.pad(fr, ((0, 0), (0, 0), (p, p), (p, p)), mode="edge" if mutate == "replicate_border" else "constant")
    U = np.stack([fp[:, :, ky:ky + H, kx:kx + W] for ky in range(k) for kx in range(k)], axis=2)       # [B, C, k k, H, W]
    return ab, U.reshape(B, -1, H * W)


def exact_reference(c, x_lab, feature, mutate=None, masks=False):
    """(out float32 [B, 2, H, W], count int [B, N]) and, with masks=True, the maximal-key sets bool [B, N, N].
    `mutate` names one of the deliberately wrong restatements (the sensitivity check only)."""
    ab, U = resized(c, x_lab, feature, mutate)
    B, N = c["B"], c["N"]
    fidx = aidx = np.arange(N)
    valid = np.ones(N, dtype=bool)
    if mutate == "unmasked_tail" and N % plan(N)["KT"]:
        fidx = aidx = np.append(fidx, N - 1)                        # the clamped row of the first key past N
        valid = np.ones(N + 1, dtype=bool)
    elif mutate == "row_mapping":
        slots = np.arange(plan(N)["ntiles"] * plan(N)["KT"])
        taken = np.array([_swapped_row(j) for j in slots])
        fidx, valid, aidx = np.minimum(slots, N - 1), taken < N, np.where(taken < N, taken, 0)
    out, count, mk = np.empty((B, 2, N), dtype=np.float32), np.empty((B, N), dtype=np.int64), []
    for b in range(B):
        A = U[b].T @ U[b][:, fidx]
        A[:, ~valid] = -np.inf
        m = A == A.max(axis=1, keepdims=True)
        count[b] = m.sum(axis=1)
        s = m.astype(np.float64) @ ab[b][:, aidx].T                  # [N, 2], integer sums
        out[b] = (s.astype(np.float32) / count[b].astype(np.float32)[:, None]).T
        mk.append(m)
    out = torch.from_numpy(out.reshape(B, 2, c["H"], c["W"]))
    return (out, count, np.stack(mk)) if masks else (out, count)


@functools.lru_cache(None)
def _solved(cid):
    c = next(c for c in exact_cases() if c["id"] == cid)
    x, f = make_inputs(c)
    want, count, m = exact_reference(c, x, f, masks=True)
    return x, f, want, count, frozenset(_placements(c, count, m))


def solved(c):
    """(x_lab, feature, expected output, maximal-key counts, placements found), computed once per case and left unchanged."""
    return _solved(c["id"])


# ---- which placements the reference found
INVENTORY = ("only_first", "only_last", "only_ragged_first", "only_upper_half", "tie_lane_pair", "tie_across_splits", "tie_three",
             "all_keys_maximal")
INVENTORY_BIG = ("later_tile_larger", "earlier_tile_larger")        # asked of each of the two N >= 2880 sizes


def _placements(c, count, m):
    """Tags of what some row of the case shows.  A row with one maximum counts only where that key is not the row itself."""
    N, pl = c["N"], plan(c["N"])
    KT, nt = pl["KT"], pl["ntiles"]
    split_of, ranges = np.array(pl["split_of"]), pl["ranges"]
    found = set()
    rows = np.arange(N)
    for b in range(c["B"]):
        first = m[b].argmax(axis=1)                                 # the lowest maximal key of every row
        last = N - 1 - m[b][:, ::-1].argmax(axis=1)
        one = (count[b] == 1) & (first != rows)
        j = first[one]
        if (j == 0).any():
            found.add("only_first")
        if (j == N - 1).any():
            found.add("only_last")
        if N % KT and nt >= 2 and (j == (nt - 1) * KT).any():
            found.add("only_ragged_first")
        if (j % KT >= KT // 2).any():
            found.add("only_upper_half")
        in_one_tile = (first // KT == last // KT) & ~((count[b] == 1) & (first == rows))
        for t in np.unique(first[in_one_tile] // KT):
            t0, t1 = ranges[split_of[t]]
            if t1 - t0 >= 2:
                found.add("later_tile_larger" if t > t0 else "earlier_tile_larger")
        two = count[b] == 2
        j1, j2 = first[two], last[two]
        if ((j1 // (KT // 2) == j2 // (KT // 2)) & ((j1 >> 2) & 1 != (j2 >> 2) & 1)).any():
            found.add("tie_lane_pair")
        if (split_of[j1 // KT] != split_of[j2 // KT]).any():
            found.add("tie_across_splits")
        if (count[b] == 3).any():
            found.add("tie_three")
        if N > 1 and (count[b] == N).all():
            found.add("all_keys_maximal")
    return found


# ---- comparison
def ulp_distance(got, want):
    """|got - want| in units of the float32 spacing at `want` (int64 tensor); a NaN or an infinity is 2^31 away."""
    g, w = got.detach().cpu().contiguous().float(), want.detach().cpu().contiguous().float()
    key = lambda t: torch.where(t.view(torch.int32) < 0, -(t.view(torch.int32) & 0x7FFFFFFF), t.view(torch.int32)).long()      # noqa: E731
    d = (key(g) - key(w)).abs()
    return torch.where(torch.isfinite(g), d, torch.full_like(d, 2 ** 31))


def is_pow2(count):
    return (count & (count - 1)) == 0


def judge(c, got, want=None, count=None):
    """None if `got` meets the acceptance rule (bit-equal where the count of maximal keys is a power of two, 1 ulp otherwise),
    else a description of the first wrong element: (b, channel, y, x), the keys expected, and the keys whose ab the output equals."""
    x, f, ref, cnt, _ = solved(c)
    want, count = (ref if want is None else want), (cnt if count is None else count)
    got = got.detach().cpu()
    if tuple(got.shape) != tuple(want.shape):
        return f"{c['id']}: shape {tuple(got.shape)} instead of {tuple(want.shape)}"
    B, H, W = c["B"], c["H"], c["W"]
    allowed = torch.from_numpy(np.where(is_pow2(count), 0, 1)).view(B, 1, H, W)
    bad = ulp_distance(got, want) > allowed
    if not bad.any():
        return None
    b, ch, y, xx = bad.nonzero()[0].tolist()
    _, _, m = exact_reference(dict(c, B=1), x[b:b + 1], f[b:b + 1], masks=True)
    ab, _ = resized(dict(c, B=1), x[b:b + 1], f[b:b + 1])
    keys = np.flatnonzero(m[0, y * W + xx]).tolist()
    same = np.flatnonzero(ab[0, ch] == float(got[b, ch, y, xx])).tolist()
    return (f"{c['id']}: {int(bad.sum())} of {bad.numel()} elements wrong, first at (b, channel, y, x) = {(b, ch, y, xx)}: got "
            f"{got[b, ch, y, xx].item()!r}, want {want[b, ch, y, xx].item()!r} = mean of ab over the maximal keys {keys} "
            f"(ab {ab[0, ch, keys].tolist()}); the output equals the ab of keys {same[:8] if same else 'none'}")


def float64_restatement(c, x_lab, feature, dtype=torch.float64):
    """tests/nlwa_reference.py at the case's alpha."""
    return R.nonlocal_weighted_average(x_lab, feature, c["k"], c["alpha"], c["sf"], dtype=dtype)
