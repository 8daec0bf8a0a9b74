"""SHA-256 digests of every output of the entry points whose kernels sit on csrc/reduce.h and csrc/feature_norm.hip, for comparing
two commits bit for bit: corr_prepare_with_mean, corr_prepare_bf16, the contextual prepare (own mean, given mean, no centring; the
norms included) and its normalise backward, channel_l2norm(_multi), warp_cn_bwd, instnorm_stats / instnorm_apply, both contextual
losses forward and backward (dvc_cx_rows / _rows_tq / _finish), fused_correlation backward (dvc_corr_softmax_bwd), cvn_head_bwd
and flow_warp backward.  The shapes are the edges of the normalise kernels: P below one tile and not a multiple of 4 (63), a
multiple of 4 and 32 but ragged in 64 (240), a multiple of 4 behind a pointer offset by one float (the scalar path), C = 66 (uneven
groups of 16, tail loop), C = 8 (fewer channels than groups), four tensors in one l2norm launch with one shorter than a workgroup.
Every input carries a plane of exact zeros and a plane of negative zeros.  Fixed seeds, one process; only dvc_amd.ops, the two
autograd modules and the C ABI behind dvc_amd.contextual are used, so the file runs unchanged on either commit.

    python tools/reduction_digests.py > A.txt                 (one line per tensor: 16 hex digits, two spaces, the label)
    python tools/reduction_digests.py --compare A.txt B.txt   (both columns side by side, `same` / `DIFFERS` per row)
"""
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (B, C, P, offset the input by one float)
PREPARE = [(2, 256, 63, False), (1, 256, 240, False), (1, 256, 240, True), (2, 66, 63, False), (1, 8, 100, False), (1, 8, 100, True)]
# (B, C, H, W) of the contextual losses (P = H * W)
CONTEXTUAL = [(2, 256, 7, 9), (1, 256, 12, 20), (2, 66, 7, 9), (1, 8, 10, 10)]
# (N, C, H, W): block sizes 256, 512 and 1024 of the InstanceNorm statistics, a plane that is no multiple of 4
INSTNORM = [(2, 3, 5, 7), (1, 3, 96, 96), (1, 3, 192, 192)]


def compare(path_a, path_b):
    rows_a, rows_b = ([ln.rstrip("\n").split("  ", 1) for ln in open(p) if ln.strip()] for p in (path_a, path_b))
    assert [r[1] for r in rows_a] == [r[1] for r in rows_b], "the two runs list different tensors"
    equal = sum(a[0] == b[0] for a, b in zip(rows_a, rows_b))
    print(f"{len(rows_a)} rows, {equal} equal.\n\nparent            branch                   result")
    for (da, label), (db, _) in zip(rows_a, rows_b):
        print(f"{da}  {db}  {'same   ' if da == db else 'DIFFERS'}  {label}")
    return 0 if equal == len(rows_a) else 1


def main():
    sys.path.insert(0, os.path.join(ROOT, "deep-exemplar-based-video-colorization_amd"))
    sys.path.insert(0, ROOT)
    import torch
    from dvc_amd import _lib, contextual, corr_autograd, flow_warp, ops
    from dvc_amd.ops import _p, _stream

    lib = _lib.load()

    def emit(label, t):
        raw = t.detach().contiguous().cpu().numpy().tobytes()
        print(f"{hashlib.sha256(raw).hexdigest()[:16]}  {label}", flush=True)

    def features(seed, shape, offset=False):
        """Random [B][C][...] map on the device with channel 0 all zeros, channel 1 all negative zeros and a position whose
        every channel is zero; `offset`: a contiguous view one float behind a 16-byte aligned address."""
        g = torch.Generator().manual_seed(seed)
        t = torch.randn(shape, generator=g)
        t[:, 0] = 0.0
        t[:, 1] = -0.0
        t.flatten(2)[:, :, 3] = 0.0
        if not offset:
            return t.cuda()
        buf = torch.empty(t.numel() + 4, device="cuda")
        v = buf[1:1 + t.numel()].view(shape)
        v.copy_(t)
        assert v.data_ptr() % 16 == 4 and v.is_contiguous()
        return v

    for (B, C, P, off) in PREPARE:
        tag = f"B={B} C={C} P={P} offset={int(off)}"
        t = features(B + C + P, (B, C, P), off)
        out, mean = ops.corr_prepare_with_mean(t)
        emit(f"corr_prepare {tag} out", out)
        emit(f"corr_prepare {tag} mean", mean)
        g = features(7 + C + P, (B, C, P))
        emit(f"warp_cn_bwd {tag} dt", ops.warp_cn_bwd(t, mean, g))
        if C == 256:
            f32, b16 = ops.corr_prepare_bf16(t)
            emit(f"corr_prepare_bf16 {tag} f32", f32)
            emit(f"corr_prepare_bf16 {tag} bf16", b16)
        x4 = t.view(B, C, 1, P)
        emit(f"channel_l2norm {tag}", ops.channel_l2norm(x4))
        # the contextual prepare as dvc_amd.contextual calls it: own mean, given mean + norms, no centring (+ norms)
        st = _stream()
        f32 = dict(device="cuda", dtype=torch.float32)
        for mode in ("own mean", "given mean", "no centring"):
            o, m, n = torch.empty((B, C, P), **f32), torch.zeros(B * C, **f32), torch.zeros((B, P), **f32)
            if mode == "own mean":
                rc = lib.dvc_cx_prepare(_p(t), None, 1, B, C, P, float(ops.EPS64), _p(m), None, _p(o), st)
            elif mode == "given mean":
                rc = lib.dvc_cx_prepare(_p(t), _p(mean), 1, B, C, P, float(ops.EPS64), None, _p(n), _p(o), st)
            else:
                rc = lib.dvc_cx_prepare(_p(t), None, 0, B, C, P, float(ops.EPS64), None, _p(n), _p(o), st)
            _lib.check(rc, "dvc_cx_prepare")
            for name, v in (("out", o), ("mean", m), ("norm", n)):
                emit(f"cx_prepare {mode} {tag} {name}", v)
            if mode != "own mean":
                dx = torch.empty((B, C, P), **f32)
                _lib.check(lib.dvc_cx_normalize_bwd(_p(o), _p(n), _p(g), B, C, P, float(ops.EPS64), _p(dx), st), "dvc_cx_normalize_bwd")
                emit(f"cx_normalize_bwd {mode} {tag} dx", dx)

    # four tensors in one launch, the smallest shorter than one workgroup (32 positions); then each alone
    xs = [features(40 + i, (2, C, H, W)) for i, (C, H, W) in enumerate([(128, 12, 20), (256, 6, 10), (66, 3, 8), (8, 1, 12)])]
    for i, y in enumerate(ops.channel_l2norm_multi(xs)):
        emit(f"channel_l2norm_multi tensor {i} {tuple(xs[i].shape)}", y)
    for i, x in enumerate(xs):
        emit(f"channel_l2norm alone tensor {i} {tuple(x.shape)}", ops.channel_l2norm(x))

    for (N, C, H, W) in INSTNORM:
        x = features(N + H, (N, C, H, W))
        tag = f"N={N} C={C} {H}x{W}"
        for name, v in zip(("scale", "shift"), ops.instnorm_stats(x)):
            emit(f"instnorm_stats {tag} {name}", v)
        slope = torch.full((1,), 0.25, device="cuda")
        sc = torch.empty(N * C, device="cuda")
        emit(f"instnorm_apply {tag} y", ops.instnorm_apply(x, slope_t=slope, scale_out=sc))
        emit(f"instnorm_apply {tag} scale", sc)

    default_lib = ops.gemm_lib()
    ops.set_gemm_lib(True)          # (the engine's products take channel counts that are multiples of 4 only)
    for (B, C, H, W) in CONTEXTUAL:
        X, Y = features(C + H, (B, C, H, W)), features(C + W, (B, C, H, W))
        gout = torch.linspace(0.5, 1.5, B).cuda()
        for centre in (True, False):
            for tag, cls in (("fwd", contextual.ContextualLoss_forward), ("bwd", contextual.ContextualLoss)):
                x = X.clone().requires_grad_(True)
                loss = cls()(x, Y, h=0.2, feature_centering=centre)
                (loss * gout).sum().backward()
                label = f"contextual {tag} B={B} C={C} {H}x{W} centre={int(centre)}"
                emit(label + " loss", loss)
                emit(label + " dX", x.grad)
    ops.set_gemm_lib(default_lib)

    for (h, w, B, wta) in [(7, 9, 2, 1), (12, 20, 1, 0.5)]:
        P = h * w
        th, ph = (ops.corr_prepare(features(s + P, (B, 256, P))) for s in (1, 2))
        g = torch.Generator().manual_seed(P)
        blab = (torch.randn(B, 3, P, generator=g) * 30).cuda()
        gy, gs = torch.randn(B, 3, h, w, generator=g).cuda(), torch.randn(B, 1, h, w, generator=g).cuda()
        a, b = th.clone().requires_grad_(True), ph.clone().requires_grad_(True)
        y, sim, amax = corr_autograd.fused_correlation(a, b, blab, 0.01, h, w, WTA_scale_weight=wta)
        ((y * gy).sum() + (sim * gs).sum()).backward()
        for name, t in (("y", y), ("sim", sim), ("argmax", amax), ("d theta", a.grad), ("d phi", b.grad)):
            emit(f"correlation {h}x{w} B={B} wta={wta} {name}", t)

    N, C, H, W = 2, 6, 15, 20       # two 256-position workgroups per image, the second ragged
    g = torch.Generator().manual_seed(5)
    ab, gab = (torch.rand(N, 2, H, W, generator=g) * 200 - 100).cuda(), torch.randn(N, 2, H, W, generator=g).cuda()
    R = features(6, (N, C, H, W))
    for name, t in zip(("dZ", "dW", "db"), ops.cvn_head_bwd(ab, gab, torch.randn(2, C, generator=g).cuda(), R)):
        emit(f"cvn_head_bwd N={N} C={C} {H}x{W} {name}", t)

    for (B, C, H, W) in [(2, 3, 9, 14), (1, 2, 40, 50)]:
        x = features(H, (B, C, H, W)).requires_grad_(True)
        flow = (torch.randn(B, 2, H, W, generator=g) * 3).cuda().requires_grad_(True)
        G = features(W, (B, C, H, W))
        (flow_warp.flow_warp(x, flow) * G).sum().backward()
        emit(f"flow_warp bwd B={B} C={C} {H}x{W} dx", x.grad)
        emit(f"flow_warp bwd B={B} C={C} {H}x{W} dflow", flow.grad)
    torch.cuda.synchronize()


if __name__ == "__main__":
    if len(sys.argv) == 4 and sys.argv[1] == "--compare":
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    main()
