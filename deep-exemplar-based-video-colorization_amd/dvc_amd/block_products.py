"""The products of the training side's row-block loops, behind one interface.

The fused correlation's backward (corr_autograd) and the contextual losses (contextual) never keep an N x N affinity: for a
block of R rows of the "rows" operand L [B, C, Nl] against the "columns" operand M [B, C, Nm] they compute

    S = L_blk^T M                  scores()
    dS from S                      the caller's HIP kernel, writing where ds_targets() says
    d M += L_blk dS                grad_cols_accumulate()      (the correlation only)
    d L_blk = M dS^T               grad_rows()

`block_products(...)` picks the implementation once per autograd call: by backend() when one was selected (set_backend /
use_backend: "vendor", "engine", "native" or "split3"), else, as ever, by ops.gemm_lib():
  * vendor (the default): ops.bmm on views — no staging copies, no padded last block, dS row-major only; buffers per
    (images, rows), so a ragged last block has its own;
  * native: the same views through ops.bgemm, this library's own strided fp32 MFMA GEMM (csrc/bgemm.hip) — no vendor library,
    any C; selected by name only;
  * split3: native's loop with ops.bgemm(engine="split3") — the bf16 matrix pipes on three bf16 terms per fp32 operand
    (csrc/bgemm_split3.hip), held to the fp32 kernel's error bound; selected by name only;
  * engine (DVC_GEMM_LIB=0): ops.conv2d with per-image filters, ksize 1, on buffers of R rows allocated once per call.  The
    block's columns of L are staged K-major (and row-major for d M) with zero rows behind a ragged block, S and dS are
    [nb, R, hm, wm] "images", the caller's kernel also writes dS^T as [nb, Nm, R/32, 32] (an image of R "pixels"), and M^T is
    copied once per image slice.  Per-image filter slices must be 16-byte aligned, else `chunk` becomes 1.
Use: images(sl_b) once per image slice; per block scores(i0, rows) first — the other three refer to that block.
"""
import contextlib
import functools

import torch

from . import ops

_BACKENDS = (None, "vendor", "engine", "native", "split3")
_backend = None


def backend():
    """The selected backend: "vendor", "engine", "native", "split3", or None = ops.gemm_lib() decides between vendor and engine."""
    return _backend


def set_backend(name):
    global _backend
    if name not in _BACKENDS:
        raise ValueError(f"dvc_amd.block_products: unknown backend {name!r}; one of {_BACKENDS}")
    _backend = name


@contextlib.contextmanager
def use_backend(name):
    """`with use_backend("native"): ...` — the selection inside the block, the earlier one after it (also on an exception)."""
    prev = backend()
    set_backend(name)
    try:
        yield
    finally:
        set_backend(prev)


def block_products(L, M, map_hw, R, chunk, want_rows=False, want_cols=False):
    """L [B, C, Nl], M [B, C, Nm] with Nm = hm * wm, map_hw = (hm, wm); R: rows per block (a multiple of 64); chunk: the most
    images the caller allows per slice (`.chunk` afterwards: what the backend takes); want_rows / want_cols: whether grad_rows /
    grad_cols_accumulate will be called."""
    name = backend() or ("vendor" if ops.gemm_lib() else "engine")
    cls = {"vendor": _Vendor, "engine": _Engine, "native": _Native, "split3": _Split3}[name]
    return cls(L, M, map_hw, R, chunk, want_rows, want_cols)


class _Products:
    dST = None

    def __init__(self, L, M, map_hw, R, chunk, want_rows, want_cols):
        self.L, self.M, self.map_hw, self.R, self.want_rows, self.want_cols = L, M, map_hw, R, want_rows, want_cols
        self.f32 = dict(device=L.device, dtype=torch.float32)
        self.chunk = chunk
        self.bufs = self._alloc(*M.shape[1:])

    def images(self, sl_b):
        self.sl_b, self.nb = sl_b, sl_b.stop - sl_b.start

    def ds_targets(self):
        """(dS, dST) for the caller's kernel, with the leading dimension scores() gave; either may be None."""
        return self.dS, self.dST


class _Views(_Products):
    """The products on views of L, M and dS; `product` is ops.bmm (_Vendor), ops.bgemm (_Native) or its split3 engine (_Split3)."""
    product = None

    def _alloc(self, C, Nm):
        return {}

    def scores(self, i0, rows):
        """(S, ld): S[b, i, :] = sum_c L[b, c, i0 + i] M[b, c, :]; images are ld rows apart."""
        self.i0, self.rows = i0, rows
        nb, (C, Nm) = self.nb, self.M.shape[1:]
        if (nb, rows) not in self.bufs:
            self.bufs[(nb, rows)] = (torch.empty((nb, rows, Nm), **self.f32),
                                     torch.empty((nb, rows, Nm), **self.f32) if self.want_rows else None,
                                     torch.empty((nb, C, rows), **self.f32) if self.want_rows else None)
        self.S, self.dS, self.staged = self.bufs[(nb, rows)]
        self.blk = self.L[self.sl_b, :, i0:i0 + rows]                    # [nb, C, rows] view
        self.product(self.blk.transpose(1, 2), self.M[self.sl_b], out=self.S)
        return self.S, rows

    def grad_cols_accumulate(self, out):
        """out[sl_b, c, j] += sum_i L[b, c, i0 + i] dS[b, i, j]"""
        self.product(self.blk, self.dS, out=out[self.sl_b], accumulate=True)

    def grad_rows(self, out):
        """out[sl_b, c, i0 + i] = sum_j M[b, c, j] dS[b, i, j]   (a block that is all of `out`: straight into it, no copy)"""
        whole = (self.nb, self.rows) == (out.shape[0], out.shape[2])
        self.product(self.M[self.sl_b], self.dS.transpose(1, 2), out=out if whole else self.staged)
        if not whole:
            out[self.sl_b, :, self.i0:self.i0 + self.rows] = self.staged


class _Vendor(_Views):
    product = staticmethod(ops.bmm)


class _Native(_Views):
    product = staticmethod(ops.bgemm)


class _Split3(_Views):
    product = staticmethod(functools.partial(ops.bgemm, engine="split3"))


class _Engine(_Products):
    def _alloc(self, C, Nm):
        R, hw, f32 = self.R, self.map_hw, self.f32
        if (Nm * C) % 4 or (C * R) % 4:          # per-image filter slices must be 16-byte aligned: else one image per call
            self.chunk = 1
        chunk = self.chunk
        return (torch.empty((chunk, R, *hw), **f32),                                          # S
                torch.empty((chunk, R, *hw), **f32) if self.want_cols else None,              # dS
                torch.empty((chunk, Nm, R // 32, 32), **f32) if self.want_rows else None,     # dS^T
                torch.zeros((chunk, C, 1, R), **f32),                                         # the block's columns of L, K-major ...
                torch.zeros((chunk, R, 1, C), **f32) if self.want_cols else None)             # ... and row-major

    def images(self, sl_b):
        super().images(sl_b)
        nb, (C, Nm) = self.nb, self.M.shape[1:]
        self.S, self.dS, self.dST, self.blk, self.blk_t = (t if t is None else t[:nb] for t in self.bufs)
        self.m_img = self.M[sl_b].view(nb, C, *self.map_hw)
        if self.want_rows:                                                  # K-major per-image filters of d L = M dS^T
            self.m_t = self.M[sl_b].transpose(1, 2).contiguous().view(nb, Nm, 1, C)

    def scores(self, i0, rows):
        self.i0, self.rows = i0, rows
        cols = self.L[self.sl_b, :, i0:i0 + rows]
        if rows < self.R:                                                   # zero rows behind a ragged block
            self.blk[..., rows:].zero_()
            if self.want_cols:
                self.blk_t[:, rows:].zero_()
        self.blk[:, :, 0, :rows].copy_(cols)
        if self.want_cols:
            self.blk_t[:, :rows, 0, :].copy_(cols.transpose(1, 2))
        ops.conv2d(self.m_img, self.blk, None, ksize=1, pad=0, out=self.S)
        return self.S, self.R

    def grad_cols_accumulate(self, out):
        if self.rows < self.R:
            self.dS.view(self.nb, self.R, -1)[:, self.rows:].zero_()
        out_img = out[self.sl_b].view(self.m_img.shape)                     # accumulated in place through the skip input
        ops.conv2d(self.dS, self.blk_t, None, ksize=1, pad=0, residual=out_img, out=out_img)

    def grad_rows(self, out):
        g = ops.conv2d(self.dST, self.m_t, None, ksize=1, pad=0)            # [nb, C, R/32, 32]
        out[self.sl_b, :, self.i0:self.i0 + self.rows] = g.view(self.nb, -1, self.R)[:, :, :self.rows]
