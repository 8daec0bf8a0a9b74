"""SHA-256 digests of everything the training side's block loops produce (dvc_amd.corr_autograd, dvc_amd.contextual), for
comparing two commits bit for bit: the loss and dX of both contextual losses; y, sim, argmax, d theta and d phi of the fused
correlation — at the parametrised sizes of tests/test_gpu_contextual.py and tests/test_gpu_corr_backward.py (54 x 96, B = 2
included) and at small maps cut into several ragged row blocks (ROW_BLOCK = 64, one with BLOCK_BYTES of a single image), in
both GEMM modes, the correlation with WTA_scale_weight 1 and 0.5.  Fixed seeds, one process; only the public entry points,
ops.set_gemm_lib and the ROW_BLOCK / BLOCK_BYTES globals are used, so the file runs unchanged on either commit.

    python tools/training_side_digests.py > A.txt              (one line per tensor: 16 hex digits, two spaces, the label)
    python tools/training_side_digests.py --compare A.txt B.txt  (both columns side by side, `same` / `DIFFERS` per row)
"""
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (C, H, W, B, h, centre, ROW_BLOCK)
CONTEXTUAL = [(512, 13, 24, 2, 0.1, True, None), (512, 27, 48, 1, 0.1, True, None), (256, 27, 48, 2, 0.1, True, None),
              (64, 24, 40, 1, 0.2, False, None), (128, 7, 9, 3, 0.1, True, None),
              (64, 10, 15, 2, 0.1, True, 64), (64, 10, 15, 2, 0.2, False, 64), (64, 9, 14, 3, 0.1, True, 64), (66, 7, 9, 2, 0.1, True, 64)]
# (h, w, B, T, ROW_BLOCK, BLOCK_BYTES)
CORRELATION = [(12, 20, 2, 0.01, None, None), (10, 16, 2, 0.01, None, None), (27, 48, 1, 0.01, None, None), (12, 20, 1, 0.005, None, None),
               (9, 7, 2, 0.05, None, None), (10, 16, 1, 0.01, None, None), (54, 96, 2, 0.01, None, None), (27, 48, 2, 0.01, None, None),
               (12, 20, 1, 1e-7, None, None),
               (12, 20, 2, 0.01, 64, None), (12, 20, 2, 0.01, 64, 4 * 64 * 240), (9, 7, 2, 0.05, 64, None)]


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
    from dvc_amd import contextual, corr_autograd, ops
    from oracle import contextual_oracle as CO

    def emit(label, t):
        raw = t.detach().contiguous().cpu().numpy().tobytes()
        print(f"{hashlib.sha256(raw).hexdigest()[:16]}  {label}", flush=True)

    def with_globals(mod, **values):
        """Set the module's block-size globals (None: the default), return what restores them."""
        before = {k: getattr(mod, k) for k in values}
        for k, v in values.items():
            if v is not None:
                setattr(mod, k, v)
        return before

    def unit(t):
        t = t - t.mean(-1, keepdim=True)
        return t / t.norm(dim=1, keepdim=True)

    default_lib = ops.gemm_lib()
    for lib_gemm in (True, False):
        ops.set_gemm_lib(lib_gemm)
        mode = "vendor-gemm" if lib_gemm else "engine-gemm"
        for (C, H, W, B, h, centre, row_block) in CONTEXTUAL:
            if C % 4 and not lib_gemm:
                continue            # (the engine takes channel counts that are multiples of 4 only)
            before = with_globals(contextual, ROW_BLOCK=row_block)
            X, Y = CO.synth_features(1000 + C + H, B, C, H, W)
            gout = torch.linspace(0.5, 1.5, B).cuda()
            for tag, cls in (("fwd", contextual.ContextualLoss_forward), ("bwd", contextual.ContextualLoss)):
                x = X.cuda().requires_grad_(True)
                loss = cls()(x, Y.cuda(), h=h, feature_centering=centre)
                (loss * gout).sum().backward()
                label = f"{mode} contextual {tag} C={C} {H}x{W} B={B} h={h} centre={int(centre)} ROW_BLOCK={row_block}"
                emit(label + " loss", loss)
                emit(label + " dX", x.grad)
            with_globals(contextual, **before)
        for (h, w, B, T, row_block, block_bytes) in CORRELATION:
            before = with_globals(corr_autograd, ROW_BLOCK=row_block, BLOCK_BYTES=block_bytes)
            g = torch.Generator().manual_seed(100 * h + w)
            P = h * w
            th, ph = unit(torch.randn(B, 256, P, generator=g)).cuda(), unit(torch.randn(B, 256, P, generator=g)).cuda()
            blab = ops.avgpool4x4((torch.randn(B, 3, 4 * h, 4 * w, generator=g) * 30).cuda()).view(B, 3, P)
            gy, gs = torch.randn(B, 3, h, w, generator=g).cuda(), torch.randn(B, 1, h, w, generator=g).cuda()
            for wta in (1, 0.5):
                a, b = th.clone().requires_grad_(True), ph.clone().requires_grad_(True)
                y, sim, amax = corr_autograd.fused_correlation(a, b, blab, T, h, w, WTA_scale_weight=wta)
                ((y * gy).sum() + (sim * gs).sum()).backward()
                label = f"{mode} correlation {h}x{w} B={B} T={T} wta={wta} ROW_BLOCK={row_block} BLOCK_BYTES={block_bytes}"
                for name, t in (("y", y), ("sim", sim), ("argmax", amax), ("d theta", a.grad), ("d phi", b.grad)):
                    emit(f"{label} {name}", t)
            with_globals(corr_autograd, **before)
    ops.set_gemm_lib(default_lib)
    torch.cuda.synchronize()


if __name__ == "__main__":
    if len(sys.argv) == 4 and sys.argv[1] == "--compare":
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    main()
