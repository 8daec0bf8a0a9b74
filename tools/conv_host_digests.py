"""SHA-256 digests of what the convolution entry points of csrc/conv_mfma.hip write, for comparing two commits bit for bit after a
change of the HOST side (checks, plans, launch arithmetic): dvc_conv2d on the image-input, stream-K and general engines and the
four Winograd entry points.  The shapes are the smallest that still reach every branch of the host code: maps of 13 x 24 and 5 x 7
(ragged in every tile size), N = 3, Cin in {8, 16, 256}, Cout in {4, 32, 64, 128}; every cfg, every split, workspaces absent, ample
and sized for one image's partial sums (several passes), per-image filters, both image-input layers, the automatic stream-K layer,
pool / dual / group / deferred reduce / batch plan.  A refused call prints its error text in place of the digest, so the refusals
are compared too.  Every output buffer carries 64 floats of slack behind it, digested with it.  Fixed seeds, one process; only the
C ABI through dvc_amd._lib is used, so the file runs unchanged on either commit.

    python tools/conv_host_digests.py [--tree PATH_TO_ANOTHER_CHECKOUT] > A.txt   (one line per case: digest, two spaces, label)
    python tools/conv_host_digests.py --compare A.txt B.txt                        (both columns side by side, `same` / `DIFFERS`)
"""
import ctypes
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if "--tree" in sys.argv:
    ROOT = os.path.abspath(sys.argv[sys.argv.index("--tree") + 1])

MAPS = [(13, 24), (5, 7)]
N = 3
RELU, PRELU, LEAKY, TANH128 = 1, 2, 3, 4
REFLECT = 1
DEFER_REDUCE, BATCH_PLAN, GRAY_INPUT = 1, 2, 4
MB = 1 << 20


def compare(path_a, path_b):
    rows_a, rows_b = ([ln.rstrip("\n").split("  ", 1) for ln in open(p) if ln.strip()] for p in (path_a, path_b))
    assert [r[1] for r in rows_a] == [r[1] for r in rows_b], "the two runs list different cases"
    equal = sum(a[0] == b[0] for a, b in zip(rows_a, rows_b))
    print(f"{len(rows_a)} rows, {equal} equal.\n\nparent            branch                   result")
    for (da, label), (db, _) in zip(rows_a, rows_b):
        print(f"{da}  {db}  {'same   ' if da == db else 'DIFFERS'}  {label}")
    return 0 if equal == len(rows_a) else 1


def main():
    sys.path.insert(0, os.path.join(ROOT, "deep-exemplar-based-video-colorization_amd"))
    import torch
    from dvc_amd import _lib

    lib = _lib.load()
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    gen = torch.Generator().manual_seed(1234)
    pool = (torch.rand(1 << 22, generator=gen) * 2 - 1).cuda()       # every input is a slice of one random buffer
    slope = torch.full((1,), 0.25, device="cuda")
    ws_buf = torch.empty(32 * MB, dtype=torch.uint8, device="cuda")

    def rnd(n, at=0):
        return pool[at:at + n]

    def ptr(t):
        return None if t is None else ctypes.c_void_p(t.data_ptr())

    def out_hw(d):
        oh, ow = ctypes.c_int32(), ctypes.c_int32()
        lib.dvc_conv2d_out_hw(ctypes.byref(d), ctypes.byref(oh), ctypes.byref(ow))
        return max(oh.value, 0), max(ow.value, 0)

    def desc(Cin, H, W, Cout, n=N, ksize=3, stride=1, dil=1, pad=None, **kw):
        f = dict(N=n, Cin=Cin, H=H, W=W, Cout=Cout, ksize=ksize, stride=stride, dil=dil,
                 pad=dil * (ksize - 1) // 2 if pad is None else pad, pad_mode=0, in_up=1, in_sub=1, act=0, act_slope=0.0, in_prelu=0,
                 cfg=-1, split_k=0, x_batch_stride=0, y_batch_stride=0, res_batch_stride=0, flags=0, w_batch_stride=0)
        f.update(kw)
        return _lib.DvcConvDesc(**f)

    def emit(label, rc, *tensors):
        if rc != 0:
            print(" ".join(lib.dvc_last_error().decode(errors="replace").split()) + "  " + label, flush=True)
            return
        h = hashlib.sha256()
        for t in tensors:
            h.update(t.cpu().numpy().tobytes())
        print(f"{h.hexdigest()[:16]}  {label}", flush=True)

    def workspace(ws):
        """`ws`: None (no workspace) or a size in bytes; the buffer is refilled so that what a deferred reduce leaves is comparable."""
        if ws is None:
            return None, 0
        assert ws <= ws_buf.numel()
        ws_buf[:ws].fill_(0)
        return ctypes.c_void_p(ws_buf.data_ptr()), ws

    def fresh(n):
        return torch.full((n + 64,), -7.0, device="cuda")

    def conv2d(label, d, ws=8 * MB, affine=False, residual=False, w_per_image=False):
        oh, ow = out_hw(d)
        planes = 1 if d.flags & GRAY_INPUT else d.Cin
        x = rnd(d.N * planes * d.H * d.W)
        wn = d.Cin * d.ksize * d.ksize * d.Cout
        if w_per_image:
            d.w_batch_stride = wn
        w = rnd((d.N if w_per_image else 1) * wn + 4096, 1 << 20)
        y = fresh(d.N * d.Cout * oh * ow)
        sc, sh = (rnd(d.N * d.Cin, 3 << 20) + 1.5, rnd(d.N * d.Cin, (3 << 20) + 4096)) if affine else (None, None)
        res = rnd(d.N * d.Cout * oh * ow, 2 << 20) if residual else None
        wp, wb = workspace(ws)
        rc = lib.dvc_conv2d(ctypes.byref(d), ptr(x), ptr(w), ptr(rnd(d.Cout, 77)), ptr(sc), ptr(sh), ptr(slope) if d.in_prelu else None,
                            ptr(slope) if d.act == PRELU else None, ptr(res), ptr(y), wp, wb, stream)
        emit("conv2d " + label, rc, y)

    def wino(label, d, ws=8 * MB, residual=False, entry="plain", d2=None, y_null=False):
        oh, ow = out_hw(d)
        cin = d.Cin + (d2.Cin if d2 else 0)
        x = rnd(d.N * d.Cin * d.H * d.W)
        x2 = rnd(d2.N * d2.Cin * d2.H * d2.W, 1 << 19) if d2 else None
        u = rnd(lib.dvc_winograd_weight_floats(d.Cout, cin), 1 << 20)
        y = fresh(d.N * d.Cout * oh * ow)
        yp = fresh(d.N * d.Cout * (oh // 2) * (ow // 2))
        res = rnd(d.N * d.Cout * oh * ow, 2 << 20) if residual else None
        wp, wb = workspace(ws)
        bias, sl = ptr(rnd(d.Cout, 77)), ptr(slope) if d.act == PRELU else None
        if entry == "pool":
            rc = lib.dvc_conv2d_winograd_pool(ctypes.byref(d), ptr(x), ptr(u), bias, sl, None if y_null else ptr(y), ptr(yp), 0, wp, wb, stream)
        elif entry == "dual":
            rc = lib.dvc_conv2d_winograd_dual(ctypes.byref(d), ctypes.byref(d2), ptr(x), ptr(x2), ptr(u), bias, sl, ptr(y), wp, wb, stream)
        else:
            rc = lib.dvc_conv2d_winograd(ctypes.byref(d), ptr(x), ptr(u), bias, sl, ptr(res), ptr(y), wp, wb, stream)
        extra = [ws_buf[:wb]] if (d.flags & DEFER_REDUCE) and wb else []
        emit(f"winograd {entry} " + label, rc, y, yp, *extra)

    def group(label, descs, ws_each=2 * MB):
        items = (_lib.DvcConvGroupItem * len(descs))()
        ys = []
        ws_buf.fill_(0)
        for i, d in enumerate(descs):
            oh, ow = out_hw(d)
            ys.append(fresh(d.N * d.Cout * oh * ow))
            items[i].d = d
            items[i].x = rnd(d.N * d.Cin * d.H * d.W, i << 18).data_ptr()
            items[i].u_packed = rnd(lib.dvc_winograd_weight_floats(d.Cout, d.Cin), (1 << 20) + (i << 12)).data_ptr()
            items[i].bias = rnd(d.Cout, 77 + i).data_ptr()
            items[i].y = ys[i].data_ptr()
            items[i].workspace = ws_buf.data_ptr() + i * ws_each
            items[i].workspace_bytes = ws_each
        rc = lib.dvc_conv2d_winograd_group(items, len(descs), stream)
        emit("winograd group " + label, rc, *ys, ws_buf[:len(descs) * ws_each])

    def one_image(d, S):
        oh, ow = out_hw(d)
        return S * d.Cout * oh * ow * 4

    # ---- dvc_conv2d
    for (H, W) in MAPS:
        m = f"{H}x{W}"
        for (ks, st, dil) in [(1, 1, 1), (3, 1, 1), (3, 1, 2), (3, 2, 1), (3, 2, 2), (1, 2, 1), (1, 1, 2)]:
            for pm in (0, REFLECT):
                conv2d(f"{m} 16->32 k{ks} s{st} d{dil} pad_mode={pm}", desc(16, H, W, 32, ksize=ks, stride=st, dil=dil, pad_mode=pm))
        for st in (1, 2):
            conv2d(f"{m} 8->32 in_up=2 s{st}", desc(8, H, W, 32, stride=st, in_up=2, pad_mode=REFLECT))
            conv2d(f"{m} 8->32 in_sub=2 s{st}", desc(8, H, W, 32, stride=st, in_sub=2))
            for prelu in (0, 1):
                conv2d(f"{m} 16->32 s{st} affine in_prelu={prelu} residual", desc(16, H, W, 32, stride=st, in_prelu=prelu, act=RELU),
                       affine=True, residual=True)
        for act in (0, RELU, PRELU, LEAKY, TANH128):
            conv2d(f"{m} 16->32 act={act}", desc(16, H, W, 32, act=act, act_slope=0.2), residual=act == LEAKY)
        for cfg in [-1, 0, 1, 2, 3, 4, 5, 16, 17, 18, 19, 20, 21, 33, 34, 35, 36, 37]:
            conv2d(f"{m} 16->64 cfg={cfg}", desc(16, H, W, 64, cfg=cfg))
            conv2d(f"{m} 16->64 d2 cfg={cfg}", desc(16, H, W, 64, dil=2, cfg=cfg))
            conv2d(f"{m} 16->64 k1 cfg={cfg}", desc(16, H, W, 64, ksize=1, cfg=cfg))
            conv2d(f"{m} 8->4 s2 cfg={cfg}", desc(8, H, W, 4, stride=2, cfg=cfg))
            conv2d(f"{m} 8->4 cfg={cfg}", desc(8, H, W, 4, cfg=cfg))
        conv2d(f"{m} 16->64 cfg=35 no workspace", desc(16, H, W, 64, cfg=35), ws=None)
        conv2d(f"{m} 16->64 cfg=36 small workspace", desc(16, H, W, 64, cfg=36), ws=4096)
        conv2d(f"{m} 16->64 cfg=36 affine", desc(16, H, W, 64, cfg=36), affine=True)
        for split in (0, 1, 2, 3):
            for (ci, co, st) in [(256, 32, 1), (256, 64, 1), (256, 128, 1), (256, 32, 2), (16, 32, 1)]:
                d = desc(ci, H, W, co, stride=st, split_k=split, act=PRELU)
                conv2d(f"{m} {ci}->{co} s{st} split_k={split} ws ample", d, residual=True)
                conv2d(f"{m} {ci}->{co} s{st} split_k={split} ws absent", d, ws=None)
                conv2d(f"{m} {ci}->{co} s{st} split_k={split} ws one image", d, ws=one_image(d, max(split, 2)), residual=True)
                conv2d(f"{m} {ci}->{co} s{st} split_k={split} ws one image + 4", d, ws=one_image(d, max(split, 2)) + 4)
        conv2d(f"{m} 256->32 affine split_k=2 ws one image", desc(256, H, W, 32, split_k=2), ws=one_image(desc(256, H, W, 32), 2), affine=True)
        for ks in (1, 3):
            conv2d(f"{m} 16->32 k{ks} per-image filters", desc(16, H, W, 32, ksize=ks), w_per_image=True)
        d = desc(256, H, W, 32, ksize=1, split_k=2)
        conv2d(f"{m} 256->32 k1 per-image filters split_k=2 ws one image", d, ws=one_image(d, 2), w_per_image=True)
        conv2d(f"{m} 16->32 per-image filters cfg=35", desc(16, H, W, 32, cfg=35), w_per_image=True)
        conv2d(f"{m} 3->64 image layer", desc(3, H, W, 64, act=RELU))
        conv2d(f"{m} 3->64 image layer gray", desc(3, H, W, 64, act=RELU, flags=GRAY_INPUT))
        conv2d(f"{m} 3->64 gray cfg=0", desc(3, H, W, 64, cfg=0, flags=GRAY_INPUT))
        conv2d(f"{m} 3->64 cfg=0", desc(3, H, W, 64, cfg=0))
        conv2d(f"{m} 3->64 residual", desc(3, H, W, 64), residual=True)
        conv2d(f"{m} 7->32 image layer", desc(7, H, W, 32, act=LEAKY, act_slope=0.2))
        for dil in (1, 2):
            conv2d(f"{m} 256->64 d{dil} automatic stream-K", desc(256, H, W, 64, dil=dil, act=RELU), ws=32 * MB, residual=True)
        conv2d(f"{m} 256->64 split_k=1 stream-K workspace", desc(256, H, W, 64, split_k=1), ws=32 * MB)
        conv2d(f"{m} 256->64 cfg=34 split_k=1", desc(256, H, W, 64, cfg=34, split_k=1), ws=32 * MB)

    # ---- the Winograd entry points
    for (H, W) in MAPS:
        m = f"{H}x{W}"
        for dil in (1, 2):
            for cfg in range(-1, 17):
                wino(f"{m} 16->128 d{dil} cfg={cfg}", desc(16, H, W, 128, dil=dil, cfg=cfg, act=RELU))
                wino(f"{m} 16->64 d{dil} cfg={cfg}", desc(16, H, W, 64, dil=dil, cfg=cfg, pad_mode=REFLECT))
            for split in (0, 1, 2, 3):
                for ci in (16, 256):
                    d = desc(ci, H, W, 64, dil=dil, split_k=split, act=PRELU)
                    wino(f"{m} {ci}->64 d{dil} split_k={split} ws ample", d, residual=True)
                    wino(f"{m} {ci}->64 d{dil} split_k={split} ws absent", d, ws=None)
                    wino(f"{m} {ci}->64 d{dil} split_k={split} ws one image", d, ws=one_image(d, max(split, 2)), residual=True)
                    wino(f"{m} {ci}->64 d{dil} split_k={split} ws one image - 1", d, ws=one_image(d, max(split, 2)) - 1)
        wino(f"{m} 16->64 in_up=2", desc(16, H, W, 64, in_up=2, pad_mode=REFLECT))
        wino(f"{m} 16->64 in_sub=2", desc(16, H, W, 64, in_sub=2))
        for split in (1, 2):
            d = desc(16, H, W, 64, split_k=split, act=RELU)
            wino(f"{m} 16->64 split_k={split}", d, entry="pool")
            wino(f"{m} 16->64 split_k={split} y NULL", d, entry="pool", y_null=True)
            wino(f"{m} 16->64 split_k={split} ws one image", d, ws=one_image(d, 2), entry="pool")
            wino(f"{m} 16+8->64 split_k={split}", desc(16, H, W, 64, split_k=split, act=LEAKY, act_slope=0.2), entry="dual", d2=desc(8, H, W, 64))
            wino(f"{m} up2(16)+8->64 split_k={split}", desc(16, H, W, 64, in_up=2, split_k=split), entry="dual", d2=desc(8, 2 * H, 2 * W, 64))
            wino(f"{m} up2(16)+8->64 split_k={split} reflect ws one image", desc(16, H, W, 64, in_up=2, split_k=split, pad_mode=REFLECT),
                 ws=one_image(desc(16, H, W, 64, in_up=2), 2), entry="dual", d2=desc(8, 2 * H, 2 * W, 64, pad_mode=REFLECT))
        wino(f"{m} 16+8->64 sizes differ", desc(16, H, W, 64), entry="dual", d2=desc(8, H + 1, W, 64))
        for flags, name in ((DEFER_REDUCE, "defer reduce"), (BATCH_PLAN, "batch plan"), (DEFER_REDUCE | BATCH_PLAN, "defer + batch plan")):
            for split in (0, 2):
                wino(f"{m} 256->64 split_k={split} {name}", desc(256, H, W, 64, split_k=split, flags=flags, act=RELU))
            d = desc(256, H, W, 64, split_k=2, flags=flags)
            wino(f"{m} 256->64 split_k=2 {name} ws one image", d, ws=one_image(d, 2))
            wino(f"{m} 256->64 split_k=2 {name} residual", d, residual=True)
        a, b, c = desc(16, H, W, 64, cfg=8, act=RELU), desc(256, H, W, 64, cfg=9, split_k=2), desc(16, W, H, 64, cfg=10, split_k=2, flags=DEFER_REDUCE)
        group(f"{m} two items merged", [a, b])
        group(f"{m} three items merged", [a, b, c])
        group(f"{m} two items, one of another shape", [a, desc(16, H, W, 128, cfg=0)])
        group(f"{m} three items, automatic plans", [desc(16, H, W, 64), desc(256, H, W, 64), desc(16, W, H, 128)])
        group(f"{m} two items, one in several passes", [a, b], ws_each=one_image(b, 2))
        group(f"{m} one item", [b])
    torch.cuda.synchronize()


if __name__ == "__main__":
    if len(sys.argv) == 4 and sys.argv[1] == "--compare":
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    main()
