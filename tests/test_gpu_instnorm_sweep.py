"""The InstanceNorm launches of csrc/norm_pool.hip over every mode, edge and plane size (tests/instnorm_cases.py), called through
the C-ABI so that S, bias, activation, strides and pointer offsets are the test's.  Per case: the value against the float64
chain inside the derived per-plane bound, NaN margins and guards untouched, inputs unchanged; the index maps bit for bit
against the plain launch gathered on the CPU; apply == stats -> affine_act, group == the per-item calls, two runs, an image of a
batch == that image alone, all bit for bit; the partial-sum variant against dvc_instnorm_apply on the float32 restatement of its
plane.  The probe tests put one value at every position where a loop of plane_stats hands over to the next and require the
statistics within one ulp of the exact value and bit-equal from every entry point, block size and alignment.
`test_zz_report` prints the worst error / bound per entry point and what check 4 found (run with -s)."""
import ctypes

import numpy as np
import pytest
import torch

import instnorm_cases as IC
from cabi_helpers import NAN, lib, ops  # noqa: F401  (fixtures)
from cabi_helpers import check as _check
from cabi_helpers import ptr as _p

pytestmark = pytest.mark.gpu
GUARD = 64                      # floats of NaN before and after a dense buffer: 256 bytes, the alignment of the view is the buffer's
WORST, CHECK4 = {}, dict(aligned=0, unaligned=0, unaligned_cases_with_other_bits=0, elements_with_other_bits=0)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda()


def _bits(t):
    return t.contiguous().view(torch.int32)


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


class Buf:
    """A device tensor the kernels see through `view` (+ `bs`, its batch stride, 0 = dense): either between two NaN guards,
    `off` floats past the 16-byte boundary, or the middle channels of a tensor with one NaN channel on each side."""

    def __init__(self, shape, lay="dense", off=0, data=None):
        n = int(np.prod(shape))
        if lay == "slice":
            N, C, H, W = shape
            self.whole = torch.full((N, C + 2, H, W), NAN, device="cuda")
            self.view, self.bs = self.whole[:, 1:1 + C], (C + 2) * H * W
        else:
            self.whole = torch.full((n + 2 * GUARD + off,), NAN, device="cuda")
            self.view, self.bs = self.whole[GUARD + off:GUARD + off + n].view(*shape), 0
        if data is not None:
            self.view.copy_(_dev(data).view(*shape))
            self.orig = self.whole.clone()

    @property
    def ptr(self):
        return _p(self.view)

    def unchanged(self):
        return torch.equal(_bits(self.whole), _bits(self.orig))

    def only_the_view_written(self):
        return not torch.isnan(self.view).any() and int(torch.isnan(self.whole).sum()) == self.whole.numel() - self.view.numel()


class Prep:
    """The buffers of one dvc_instnorm_apply (x given) or dvc_instnorm_apply_partials (part given) call; `call` launches it,
    `item` describes it to dvc_instnorm_apply_group."""

    def __init__(self, *, x=None, part=None, bias=None, act=IC.ACTS["none"], palign="aligned", xoff=0, cs=None, res=None, slope=None, up=1,
                 sub=1, rpad=0, second=None, scale_out=False, xlay="dense", ylay="dense", rlay="dense", inplace=False):
        self.N, self.C, self.H, self.W = self.shape = (x if part is None else part[0]).shape
        self.up, self.sub, self.rpad, self.act = up, sub, rpad, act
        self.S = 0 if part is None else part.shape[0]
        self.src = Buf(x.shape, xlay, xoff, x) if part is None else Buf(part.shape, "dense", 1 if palign == "off1" else 0, part)
        self.res = None if res is None else Buf(res.shape, rlay, 0, res)
        self.bias, self.cs, self.slope = (None if v is None else _dev(np.atleast_1d(v)) for v in (bias, cs, slope))
        self.aptr = None if act[2] is None else _dev(np.atleast_1d(act[2]))
        OH, OW = IC.out_size(self.H, self.W, up, sub, rpad)
        self.y = self.src if inplace else Buf((self.N, self.C, OH, OW), ylay)
        self.outs = [] if inplace else [self.y]
        self.sub2, self.cs2, self.y2 = 1, None, None
        if second is not None:
            self.sub2, self.cs2 = second[0], None if second[1] is None else _dev(second[1])
            self.y2 = Buf((self.N, self.C) + IC.out_size(self.H, self.W, 1, self.sub2, 0))
            self.outs.append(self.y2)
        self.sc = self.sh = None
        if scale_out:
            self.sc, self.sh = Buf((self.N, self.C)), Buf((self.N, self.C))
            self.outs += [self.sc, self.sh]
        self.ins = [b for b in (self.src, self.res) if b is not None and b is not self.y]

    def _opt(self, b):
        return None if b is None else b.ptr

    def call(self, lib, st):
        tail = (self.y.bs, self.y.ptr, self._opt(self.sc), self._opt(self.sh), _p(self.cs2), self.sub2, self._opt(self.y2), st)
        dims = (IC.EPS, self.N, self.C, self.H, self.W, self.up, self.sub, self.rpad)
        rbs = 0 if self.res is None else self.res.bs
        if self.S == 0:
            return lib.dvc_instnorm_apply(self.src.ptr, self._opt(self.res), _p(self.slope), _p(self.cs), *dims, self.src.bs, rbs, *tail)
        return lib.dvc_instnorm_apply_partials(self.src.ptr, self.S, _p(self.bias), self.act[0], self.act[1], _p(self.aptr),
                                               self._opt(self.res), _p(self.slope), _p(self.cs), *dims, rbs, *tail)

    def run(self, lib, st):
        _check(self.call(lib, st), "dvc_instnorm_apply" + ("_partials" if self.S else ""))
        return self

    def item(self):
        from dvc_amd._lib import DvcInstNormItem
        v = lambda t: None if t is None else t.data_ptr()                                       # noqa: E731
        b = lambda t: None if t is None else t.view.data_ptr()                                  # noqa: E731
        return DvcInstNormItem(x=b(self.src), S=self.S, bias=v(self.bias), act=self.act[0], act_slope=self.act[1], act_slope_ptr=v(self.aptr),
                               residual=b(self.res), slope_ptr=v(self.slope), chan_scale=v(self.cs), eps=IC.EPS, N=self.N, C=self.C,
                               H=self.H, W=self.W, up=self.up, sub=self.sub, rpad=self.rpad, x_batch_stride=self.src.bs if self.S == 0 else 0,
                               res_batch_stride=0 if self.res is None else self.res.bs, y_batch_stride=self.y.bs, y=b(self.y))

    def clean(self):
        """Nothing but the outputs written: their margins and guards still NaN, no NaN inside, every input as it was."""
        return all(o.only_the_view_written() for o in self.outs) and all(i.unchanged() for i in self.ins) and \
            (self.y is not self.src or self._inplace_margins())

    def _inplace_margins(self):
        w, o = self.src.whole.clone(), self.src.orig.clone()
        for t in (w, o):
            (t[:, 1:1 + self.C] if t.dim() == 4 else t[GUARD:t.numel() - GUARD]).zero_()
        return torch.equal(_bits(w), _bits(o)) and not torch.isnan(self.y.view).any()


class StatsPrep(Prep):
    """dvc_instnorm_stats -> dvc_affine_act on the same buffers (scale / shift are always outputs here)."""

    def call(self, lib, st):
        rc = lib.dvc_instnorm_stats(self.src.ptr, self.N, self.C, self.H * self.W, self.src.bs, IC.EPS, _p(self.cs), self.sc.ptr, self.sh.ptr, st)
        if rc:
            return rc
        return lib.dvc_affine_act(self.src.ptr, self.sc.ptr, self.sh.ptr, self._opt(self.res), _p(self.slope), self.N, self.C, self.H, self.W,
                                  self.up, self.rpad, self.src.bs, 0 if self.res is None else self.res.bs, self.y.bs, self.y.ptr, st)


def launch_kw(c, t):
    """The keywords of Prep for a case and its graded data."""
    m = IC.mode_params(c["mode"])
    kw = dict(cs=t["cs"], res=t["res"], slope=t["slope"], up=m["up"], sub=m["sub"], rpad=m["rpad"], second=IC.second_of(c, t),
              scale_out=c.get("scale_out", False), ylay=c["ylay"], rlay=c["rlay"], inplace=m["inplace"])
    if c["entry"] == "partials":
        kw.update(part=t["part"], bias=t["bias"], act=t["act"], palign=c["part"])
    else:
        kw.update(x=t["x"], xlay=c["xlay"])
    return kw


def check_value(entry, cid, what, got, want, bound):
    got = got.contiguous().cpu().numpy()
    assert got.shape == want.shape, (cid, what, got.shape, want.shape)
    w = IC.first_wrong(got, want, bound)
    assert w is None, "%s %s: first wrong (n, c, y, x) = (%d, %d, %d, %d): got %.9g, float64 %.9g, bound %.3g" % ((cid, what) + w)
    WORST[entry] = max(WORST.get(entry, 0.0), IC.worst_ratio(got, want, bound))


def check_outputs(entry, c, p, ref):
    check_value(entry, c["id"], "y", p.y.view, ref["y"], ref["bound"])
    if p.y2 is not None:
        check_value(entry, c["id"], "y2", p.y2.view, ref["y2"], ref["bound2"])
    if p.sc is not None:                        # the float64 statistics' own error is far below the one rounding to float32
        for name, got, want in (("scale_out", p.sc, ref["scale"]), ("shift_out", p.sh, ref["shift"])):
            u = IC.ulps(got.view.cpu().numpy(), want)
            assert (u <= 1).all(), (c["id"], name, float(u.max()))
    assert p.clean(), (c["id"], "something outside the outputs was written, or an input changed")


def outputs_equal(a, b):
    return same_bits(a.y.view, b.y.view) and (a.y2 is None or same_bits(a.y2.view, b.y2.view)) and \
        (a.sc is None or b.sc is None or (same_bits(a.sc.view, b.sc.view) and same_bits(a.sh.view, b.sh.view)))


def check_index_map(lib, st, c, kw, p):
    """The mapped output == the plain launch of the same x, slope and chan_scale gathered through the documented map; y2 == the
    separate launch with chan_scale2 at sub2."""
    if (kw["up"], kw["sub"], kw["rpad"]) != (1, 1, 0):
        plain = Prep(**dict(kw, up=1, sub=1, rpad=0, second=None, scale_out=False, ylay="dense")).run(lib, st)
        want = IC.gather(plain.y.view.cpu().numpy(), IC.index_maps(p.H, p.W, kw["up"], kw["sub"], kw["rpad"]))
        assert same_bits(p.y.view.cpu(), torch.from_numpy(np.ascontiguousarray(want))), (c["id"], "index map")
    if kw["second"] is not None:
        sub2, cs2 = kw["second"]
        alone = Prep(**dict(kw, cs=cs2, sub=sub2, up=1, rpad=0, res=None, slope=None, second=None, scale_out=False, ylay="dense",
                            inplace=False)).run(lib, st)
        assert same_bits(alone.y.view, p.y2.view), (c["id"], "y2 against its own launch")


def check_image_alone(lib, st, c, kw, p, cls=Prep):
    if p.N == 1:
        return
    one = {k: (v[:, 1:2] if k == "part" else v[1:2]) for k, v in kw.items() if k in ("x", "part", "res") and v is not None}
    q = cls(**dict(kw, **one)).run(lib, st)
    assert same_bits(q.y.view, p.y.view[1:2]) and (p.y2 is None or same_bits(q.y2.view, p.y2.view[1:2])), (c["id"], "image 1 alone")
    assert p.sc is None or same_bits(q.sc.view, p.sc.view[1:2]), (c["id"], "statistics of image 1 alone")


# ---- graded regime
@pytest.mark.parametrize("c", IC.cases("apply"), ids=lambda c: c["id"])
def test_apply(lib, ops, c):
    st = ops._stream()
    t = IC.make_data(c)
    kw = launch_kw(c, t)
    ref = IC.reference(t["x"], second=kw["second"], **IC.ref_args(c, t))
    p = Prep(**kw).run(lib, st)
    check_outputs("apply", c, p, ref)
    assert outputs_equal(p, Prep(**kw).run(lib, st)), (c["id"], "two runs")
    check_index_map(lib, st, c, kw, p)
    check_image_alone(lib, st, c, kw, p)


@pytest.mark.parametrize("c", IC.cases("stats"), ids=lambda c: c["id"])
def test_stats_then_affine_act(lib, ops, c):
    st = ops._stream()
    t = IC.make_data(c)
    kw = dict(launch_kw(c, t), scale_out=True)
    ref = IC.reference(t["x"], **IC.ref_args(c, t))
    p = StatsPrep(**kw).run(lib, st)
    check_outputs("stats", c, p, ref)
    assert outputs_equal(p, Prep(**kw).run(lib, st)), (c["id"], "apply == stats -> affine_act")
    assert outputs_equal(p, StatsPrep(**kw).run(lib, st)), (c["id"], "two runs")
    check_image_alone(lib, st, c, kw, p, StatsPrep)


@pytest.mark.parametrize("c", IC.cases("partials"), ids=lambda c: c["id"])
def test_partials(lib, ops, c):
    st = ops._stream()
    t = IC.make_data(c)
    kw = launch_kw(c, t)
    ref = IC.reference(t["x"], second=kw["second"], **IC.ref_args(c, t))
    p = Prep(**kw).run(lib, st)
    check_outputs("partials", c, p, ref)
    assert outputs_equal(p, Prep(**kw).run(lib, st)), (c["id"], "two runs")
    check_index_map(lib, st, c, kw, p)
    check_image_alone(lib, st, c, kw, p)
    # check 4: reduce -> dvc_instnorm_apply, the reduce being the float32 restatement of the plane
    over = {k: v for k, v in kw.items() if k not in ("part", "bias", "act", "palign")}
    q = Prep(x=t["x"], **over).run(lib, st)
    check_outputs("apply", c, q, ref)
    if c["HW"] % 4 == 0:
        CHECK4["aligned"] += 1
        assert outputs_equal(p, q), (c["id"], "partials against reduce -> apply")
    else:                                       # the LDS plane is 16-byte aligned, the tensor's plane c * HW is not: another order in double
        CHECK4["unaligned"] += 1
        n = int((_bits(p.y.view) != _bits(q.y.view)).sum())
        if p.y2 is not None:
            n += int((_bits(p.y2.view) != _bits(q.y2.view)).sum())
        CHECK4["elements_with_other_bits"] += n
        CHECK4["unaligned_cases_with_other_bits"] += n > 0
        print(f"{c['id']}: {n} elements differ from reduce -> apply (both inside the bound)")


def _group_preps(g):
    out = []
    for c in g["items"]:
        t = IC.make_data(c)
        out.append(dict(launch_kw(c, t), second=None, scale_out=False))
    return out


@pytest.mark.parametrize("g", IC.group_cases(), ids=lambda g: g["id"])
def test_group(lib, ops, g):
    from dvc_amd._lib import DvcInstNormItem
    st = ops._stream()
    kws = _group_preps(g)
    grouped, alone = [Prep(**kw) for kw in kws], [Prep(**kw).run(lib, st) for kw in kws]
    arr = (DvcInstNormItem * len(grouped))(*[p.item() for p in grouped])
    _check(lib.dvc_instnorm_apply_group(arr, len(grouped), st), "dvc_instnorm_apply_group")
    for c, a, b in zip(g["items"], grouped, alone):
        assert same_bits(a.y.view, b.y.view), (g["id"], c["id"], "group against the item's own launch")
        assert a.clean() and b.clean(), (g["id"], c["id"])
        t = IC.make_data(c)
        ref = IC.reference(t["x"], **IC.ref_args(c, t))
        check_value("group", c["id"], "y", a.y.view, ref["y"], ref["bound"])


# ---- probe regime
def _probe_stats_ok(name, p, want):
    for got, w in ((p.sc, want[0]), (p.sh, want[1])):
        u = IC.ulps(got.view.cpu().numpy(), w)
        assert (u <= 1).all(), (name, "plane (n, c) = %s is %.3g ulps from the exact statistics" % (tuple(np.argwhere(u > 1)[0]), u.max()),
                                "probe positions", IC.probe_positions(p.H * p.W))


@pytest.mark.parametrize("plane", IC.PLANES, ids=lambda s: "%dx%d" % s)
def test_probe_statistics_from_every_entry_point(lib, ops, plane):
    from dvc_amd._lib import DvcInstNormItem
    st = ops._stream()
    H, W = plane
    HW = H * W
    rng = np.random.default_rng(HW)
    for two in (False, True):
        x = IC.probe_tensor(H, W, two)
        want = IC.probe_stats(x)
        runs = {"stats": StatsPrep(x=x, scale_out=True), "stats, one float off": StatsPrep(x=x, xoff=1, scale_out=True),
                "apply": Prep(x=x, scale_out=True), "apply, one float off": Prep(x=x, xoff=1, scale_out=True)}
        if HW <= IC.K["LDS"]:
            runs["partials"] = Prep(part=x[None], scale_out=True)
            runs["partials, one float off"] = Prep(part=x[None], palign="off1", scale_out=True)
        first = None
        for name, p in runs.items():
            p.run(lib, st)
            _probe_stats_ok((plane, two, name), p, want)
            first = first or p
            assert outputs_equal(first, p), (plane, two, name, "other bits than dvc_instnorm_stats")
            assert p.clean(), (plane, two, name)
        # the group launch has no scale_out: its y against dvc_instnorm_apply's, next to an item that leaves the block at 512
        # (where the probe plane is below the threshold) and next to one that forces 1024
        for side in ((3, 5), (64, 64)):
            other = (rng.standard_normal((1, 2) + side) * 3 + 1.5).astype(np.float32)
            items = [Prep(x=x), Prep(x=other)] + ([Prep(part=x[None])] if HW <= IC.K["LDS"] else [])
            arr = (DvcInstNormItem * len(items))(*[p.item() for p in items])
            _check(lib.dvc_instnorm_apply_group(arr, len(items), st), "dvc_instnorm_apply_group")
            for p in items[:1] + items[2:]:
                assert same_bits(p.y.view, first.y.view) and p.clean(), (plane, two, side, "group")


@pytest.mark.parametrize("plane", IC.PLANES_PARTIALS, ids=lambda s: "%dx%d" % s)
def test_probe_partials_equal_reduce_then_apply(lib, ops, plane):
    """Integer slices, integer bias, slopes 0.25 / 0.5: the plane and its sums are exact, so the bits agree whatever the alignment."""
    st = ops._stream()
    H, W = plane
    for S, act, palign in ((3, IC.ACTS["prelu_ptr"], "aligned"), (IC.K["SMAX"], (IC.ACT_LEAKY, 0.5, None), "off1"), (2, IC.ACTS["relu"], "off1")):
        part, bias = IC.probe_partials(H, W, S, H * W + S)
        x = IC.restate_partials(part, bias, act)
        assert IC.exact_in_double(x)
        p = Prep(part=part, bias=bias, act=act, palign=palign, scale_out=True).run(lib, st)
        q = Prep(x=x, scale_out=True).run(lib, st)
        q1 = Prep(x=x, xoff=1, scale_out=True).run(lib, st)
        _probe_stats_ok((plane, S, "partials"), p, IC.probe_stats(x))
        assert outputs_equal(p, q) and outputs_equal(p, q1), (plane, S, "partials against reduce -> apply")
        assert p.clean() and q.clean()


# ---- the limit and the refusals
def _refused(lib, rc, needle):
    assert rc != 0, "accepted"
    assert needle.encode() in lib.dvc_last_error(), lib.dvc_last_error()


def test_the_lds_limit_and_the_documented_refusals(lib, ops):
    from dvc_amd._lib import DvcInstNormItem
    st = ops._stream()
    side = int(round(IC.K["LDS"] ** 0.5))
    c = dict(entry="partials", id="limit-%dx%d-S2" % (side, side), mode="slope", slope=0.25, N=1, C=3, H=side, W=side, HW=side * side, S=2,
             bias=True, act="prelu_ptr", part="aligned", second="none", ylay="dense", rlay="dense", seed=side)
    t = IC.make_data(c)
    kw = launch_kw(c, t)
    p = Prep(**kw)
    rc = p.call(lib, st)
    assert rc == 0, ("the largest plane the entry point documents was refused", lib.dvc_last_error())
    check_outputs("partials", c, p, IC.reference(t["x"], **IC.ref_args(c, t)))
    H, W = IC.PLANE_OVER_LDS
    over = (np.zeros((1, 1, 2, H, W), np.float32))
    _refused(lib, Prep(part=over).call(lib, st), "does not fit the LDS image")
    Prep(x=over[0]).run(lib, st)                                    # the plain entry takes the same plane
    small = np.ones((1, 2, 3, 5), np.float32)
    items = [Prep(x=small) for _ in range(IC.K["GMAX"] + 1)]
    arr = (DvcInstNormItem * len(items))(*[q.item() for q in items])
    _refused(lib, lib.dvc_instnorm_apply_group(arr, len(items), st), "1..%d items" % IC.K["GMAX"])
    _refused(lib, Prep(x=small, res=small, up=2).call(lib, st), "residual requires up == sub == 1")
    _refused(lib, Prep(part=small[None], res=small, up=2).call(lib, st), "residual requires up == sub == 1")
    _refused(lib, Prep(part=np.ones((IC.K["SMAX"] + 1, 1, 2, 3, 5), np.float32)).call(lib, st), "bad argument")
    torch.cuda.synchronize()


def test_zz_report():
    print("cases:", {e: len(IC.cases(e)) for e in IC.ENTRIES}, "group:", len(IC.group_cases()))
    print("worst error / bound:", {k: round(v, 3) for k, v in WORST.items()})
    print("check 4 (partials against reduce -> apply):", CHECK4)
