"""Test infrastructure: float64 restatements of the bandwidth-bound kernels between the GEMMs of the contextual losses
(csrc/contextual.hip, dvc_cx_normalize_bwd of csrc/feature_norm.hip) and of the fused correlation's backward (csrc/corr_bwd.hip),
on the CPU, with the per-element error bounds their float32 arithmetic allows.  Product code never imports it.

Everything starts from a GIVEN float32 block S (or F): the GEMM that produced it is somebody else's rounding.  A float32 input is
exact in float64, so an arg-max taken here is the arg-max the kernel sees.  Ties are resolved explicitly (`lowest_argmax`), never
left to torch.max, and the gradients are routed by `gather` at those indices.

Notation (header of contextual.hip): d = 1 - S, a_i = min_j d_ij + 1e-5, z = (1 - d / a_i) / h, w = exp(z), l_i = sum_j w_ij,
A = w / l_i, r_i = A_{i j*}, E_i = sum_j A_ij d_ij.  Tensors carry any number of leading batch dimensions: S [..., rows, N].

Error model, u = 2^-24 (half an ulp of float32, relative):
  q = d / a carries the roundings of d, of a and of the division; 1 - q one more and / h one more:
      dz <= u (3 q + 2 |1 - q| + 1) / h                                                      `dz_bound`
    (a = fl(fl(1 - m) + 1e-5f) is good to u when the row maximum m >= 1/2, where 1 - m is exact, and to 2 u otherwise: the count
    for q is then 4, which the + 1 covers for q <= 1, that is at the columns that carry the sums; measured: the docstring of
    test_gpu_cx_kernels.py)
  the device exponential is good to 1 ulp = 2 u, a following division or product adds u each:
      dw <= w (dz + 4 u) + 2^-126                                                            `w_bound`   (2^-126: a flushed denormal)
      dA <= A (dz + 6 u) + 2^-126        (a and l GIVEN as float32: their roundings are in the 3 q and the 6 u)   `A_bound`
  a 256-thread row sum of N terms is ceil(N / 256) serial additions, six butterfly steps and two tree steps per value:
      d(sum_j x_j) <= sum_j dx_j + (ceil(N / 256) + 10) u |sum|                              `NR`
"""
import math

import torch

U = 2.0 ** -24
TINY = 2.0 ** -126


def NR(N):
    """Roundings of a 256-thread row sum over N terms (see the module docstring), times u."""
    return ((N + 255) // 256 + 10) * U


def lowest_argmax(t, dim):
    """Index of the maximum of t along dim; the LOWEST index on exact ties."""
    n = t.shape[dim]
    shape = [1] * t.dim()
    shape[dim] = n
    idx = torch.arange(n).view(shape).expand_as(t)
    m = t.max(dim, keepdim=True)[0]
    return torch.where(t == m, idx, torch.full_like(idx, n)).min(dim)[0]


def onehot(idx, n):
    return torch.arange(n) == idx.unsqueeze(-1)


def weights(S, a, h):
    """w = exp((1 - (1 - S) / a_i) / h) in float64."""
    return torch.exp((1 - (1 - S.double()) / a.double().unsqueeze(-1)) / h)


def affinity(S, a, l, h):
    return weights(S, a, h) / l.double().unsqueeze(-1)


# ------------------------------------------------------------------------------------------------ inputs
def features(seed, B, C, Nx, Ny, centre=True):
    """oracle.contextual_oracle.synth_features cut to Nx / Ny positions: (X [B, C, 1, Nx], Y [B, C, 1, Ny]) float32 as the modules
    take them, and their centred, normalised float64 forms Xn [B, C, Nx], Yn [B, C, Ny] (ContextualLoss.py:48-61)."""
    from oracle import contextual_oracle as O
    X, Y = O.synth_features(seed, B, C, 1, max(Nx, Ny))
    X, Y = X[..., :Nx].contiguous(), Y[..., :Ny].contiguous()
    x, y = X.double(), Y.double()
    if centre:
        mu = y.mean(-1, keepdim=True)
        x, y = x - mu, y - mu
    return X, Y, O.feature_normalize(x).view(B, C, Nx), O.feature_normalize(y).view(B, C, Ny)


def scores(seed, B, C, Nx, Ny, centre=True):
    """S [B, Nx, Ny] = the float32 rounding of Xn^T Yn: the block a GEMM would hand the kernels."""
    _, _, Xn, Yn = features(seed, B, C, Nx, Ny, centre)
    return torch.matmul(Xn.transpose(1, 2), Yn).float()


# ------------------------------------------------------------------------------------------------ forward pieces
def rows_stats(S, h):
    """dvc_cx_rows: (a, jstar, l, r, e) per row of S."""
    S = S.double()
    jstar = lowest_argmax(S, -1)
    a = (1 - S.gather(-1, jstar.unsqueeze(-1)).squeeze(-1)) + 1e-5
    w = weights(S, a, h)
    l = w.sum(-1)
    r = w.gather(-1, jstar.unsqueeze(-1)).squeeze(-1) / l
    e = (w * (1 - S)).sum(-1) / l
    return a, jstar, l, r, e


def col_max(S, a, l, h, row0=0, cmax_in=None, cargi_in=None):
    """dvc_cx_colmax: running maximum of A over the rows of this block and the row (row0 + i) it sits in.  The lower row wins ties
    inside the block; a carried-in value wins ties against every row of the block (its row is in an earlier block)."""
    A = affinity(S, a, l, h)
    cargi = lowest_argmax(A, -2)
    cmax = A.gather(-2, cargi.unsqueeze(-2)).squeeze(-2)
    cargi = cargi + row0
    if cmax_in is not None:
        keep = cmax_in.double() >= cmax
        cmax, cargi = torch.where(keep, cmax_in.double(), cmax), torch.where(keep, cargi_in.long(), cargi)
    return cmax, cargi


def rows_tq(S, a, l, cargi, row0, h):
    """dvc_cx_rows_tq: T_i = sum of A_ik over the columns k whose maximum sits in row row0 + i, Q_i = the same weighted by d_ik."""
    A = affinity(S, a, l, h)
    rows = S.shape[-2]
    own = cargi.unsqueeze(-2) == (row0 + torch.arange(rows)).unsqueeze(-1)
    return (A * own).sum(-1), (A * own * (1 - S.double())).sum(-1)


def finish(v):
    """dvc_cx_finish: loss = -log mean(v), gscale = d loss / d v_k = -1 / (n mean(v)), per image (last dimension)."""
    mean = v.double().mean(-1)
    return -torch.log(mean), -1.0 / (v.shape[-1] * mean)


# ------------------------------------------------------------------------------------------------ the losses as functions of S
def loss(S, h, mode):
    """The contextual losses restated on S [..., Nx, Ny] (any float dtype, differentiable): mode 0 = ContextualLoss_forward,
    -log mean_i A[i, jstar_i]; mode 1 = ContextualLoss, -log mean_k A[cargi_k, k].  a_i is d gathered at jstar_i, the maxima
    are A gathered at the explicit lowest-index arg-max: on a tie the whole gradient goes to the lowest index."""
    d = 1 - S
    jstar = lowest_argmax(S.detach(), -1).unsqueeze(-1)
    a = d.gather(-1, jstar) + 1e-5
    w = torch.exp((1 - d / a) / h)
    A = w / w.sum(-1, keepdim=True)
    if mode == 0:
        v = A.gather(-1, jstar).squeeze(-1)
    else:
        cargi = lowest_argmax(A.detach(), -2).unsqueeze(-2)
        v = A.gather(-2, cargi).squeeze(-2)
    return -torch.log(v.mean(-1))


def ds(S, h, mode, gout=1.0):
    """dvc_cx_ds: d (sum_b gout_b loss_b) / d S by float64 autograd through `loss` — not a copy of the kernel's formula."""
    S64 = S.double().clone().requires_grad_(True)
    L = loss(S64, h, mode)
    (L * torch.as_tensor(gout, dtype=torch.float64)).sum().backward()
    return S64.grad


def normalize_bwd(xn, norm, dxn, eps):
    """dvc_cx_normalize_bwd: backward of xn = x / (n + eps), n = ||x||_C, from the saved xn [B, C, P] and n [B, P]:
    dx = dxn / (n + eps) - xn (xn . dxn) / n, the second term absent where n == 0."""
    xn, n, dxn = xn.double(), norm.double().unsqueeze(1), dxn.double()
    dot = (xn * dxn).sum(1, keepdim=True)
    k = torch.where(n > 0, dot / n.clamp_min(1e-300), torch.zeros_like(dot))
    return dxn / (n + eps) - xn * k


# ------------------------------------------------------------------------------------------------ bounds, contextual
def dz_bound(S, a, h):
    q = (1 - S.double()) / a.double().unsqueeze(-1)
    return U * (3 * q + 2 * (1 - q).abs() + 1) / h


def w_bound(S, a, h):
    return weights(S, a, h) * (dz_bound(S, a, h) + 4 * U) + TINY


def A_bound(S, a, l, h):
    return affinity(S, a, l, h) * (dz_bound(S, a, h) + 6 * U) + TINY


def rows_bounds(S, h):
    """Bounds of l, r, e of dvc_cx_rows against rows_stats(S, h):
        dl <= sum_j dw_j + NR l
        dr <= r (dw* / w* + dl / l + u)                                          (w* recomputed at the maximum, one division)
        de <= [sum_j d_j (dw_j + u w_j) + NR sum_j w_j d_j] / l + e (dl / l + u)     (d_j rounded once, the fmaf once: in NR)"""
    a, jstar, l, r, e = rows_stats(S, h)
    N = S.shape[-1]
    w, dw, d = weights(S, a, h), w_bound(S, a, h), 1 - S.double()
    dl = dw.sum(-1) + NR(N) * l
    js = jstar.unsqueeze(-1)
    dr = r * (dw.gather(-1, js).squeeze(-1) / w.gather(-1, js).squeeze(-1) + dl / l + U)
    num = (w * d).sum(-1)
    de = ((d * (dw + U * w)).sum(-1) + NR(N) * num) / l + e * (dl / l + U)
    return dl, dr, de


def tq_bounds(S, a, l, cargi, row0, h):
    """dT <= sum_owned dA + NR T;  dQ <= sum_owned d (dA + u A) + NR Q."""
    A, dA, d = affinity(S, a, l, h), A_bound(S, a, l, h), 1 - S.double()
    own = cargi.unsqueeze(-2) == (row0 + torch.arange(S.shape[-2])).unsqueeze(-1)
    t, q = rows_tq(S, a, l, cargi, row0, h)
    N = S.shape[-1]
    return (dA * own).sum(-1) + NR(N) * t, (d * (dA + U * A) * own).sum(-1) + NR(N) * q


def ds_bound(S, h, mode, g, a, jstar, l, r, e, cargi=None, T=None, Q=None, row0=0):
    """Bound of dvc_cx_ds on a block of rows against `ds`, the row statistics GIVEN as the float32 roundings of a, l, r, e (and
    T, Q): v = dz / (h a) - [k = j*] sdd / (h a^2), g = gscale * gout (two roundings), delta = the 0 / 1 indicator.
      mode 0: dz = g r (delta - A)        d(dz)  <= |g| r (dA + 6 u |delta - A|)           (g: 2, r: 1, the difference, two products)
              sdd = g r ((a - 1e-5) - E)   d(sdd) <= |g| r (3 u a + u E + 6 u |dmin - E|)   (dmin recovered from a: 3 u a absolute)
      mode 1: dz = g A (delta - T)        d(dz)  <= |g| (dA |delta - T| + A (5 u |delta - T| + u T))
              sdd = g (Q - T E)           d(sdd) <= |g| (u Q + 3 u T E + 4 u |Q - T E|)
      d(v) <= (d(dz) + 3 u |dz|) / (h a) + [k = j*] (d(sdd) + 5 u |sdd|) / (h a^2) + u |v| + 2^-126
    (3 u: a, the product h a, the division; 5 u: a twice, two products, the division; u |v|: the final subtraction.)"""
    N = S.shape[-1]
    A, dA = affinity(S, a, l, h), A_bound(S, a, l, h)
    star = onehot(jstar, N).double()
    g = torch.as_tensor(g, dtype=torch.float64).reshape(-1, 1, 1).abs() if S.dim() == 3 else abs(float(g))
    au, ru, eu = a.unsqueeze(-1), r.unsqueeze(-1), e.unsqueeze(-1)
    if mode == 0:
        dz = g * ru * (star - A)
        ddz = g * ru * (dA + 6 * U * (star - A).abs())
        dmin = au - 1e-5
        sdd = g * ru * (dmin - eu)
        dsdd = g * ru * (3 * U * au + U * eu + 6 * U * (dmin - eu).abs())
    else:
        own = (cargi.unsqueeze(-2) == (row0 + torch.arange(S.shape[-2])).unsqueeze(-1)).double()
        Tu, Qu = T.unsqueeze(-1), Q.unsqueeze(-1)
        dz = g * A * (own - Tu)
        ddz = g * (dA * (own - Tu).abs() + A * (5 * U * (own - Tu).abs() + U * Tu))
        sdd = g * (Qu - Tu * eu)
        dsdd = g * (U * Qu + 3 * U * Tu * eu + 4 * U * (Qu - Tu * eu).abs())
    ha = h * au
    v = dz / ha - star * sdd / (ha * au)
    return (ddz + 3 * U * dz.abs()) / ha + star * (dsdd + 5 * U * sdd.abs()) / (ha * au) + U * v.abs() + TINY


def normalize_bwd_bound(xn, norm, dxn, eps):
    """dot = xn . dxn carries ceil(C / 16) + 16 roundings (an fmaf chain per channel group, then the 16 groups);
    dx = dxn * inv - xn * k with inv = 1 / (n + eps) (two roundings), k = dot / n (one):
        d(dx) <= 3 u |dxn| / (n + eps) + |xn| (d(dot) / n + 2 u |k|) + u |dx|"""
    C = xn.shape[1]
    xn, n, dxn = xn.double(), norm.double().unsqueeze(1), dxn.double()
    ddot = ((C + 15) // 16 + 16) * U * (xn * dxn).abs().sum(1, keepdim=True)
    pos = n > 0
    nn = n.clamp_min(1e-300)
    k = torch.where(pos, (xn * dxn).sum(1, keepdim=True) / nn, torch.zeros_like(n))
    dk = torch.where(pos, ddot / nn + 2 * U * k.abs(), torch.zeros_like(n))
    return 3 * U * dxn.abs() / (n + eps) + xn.abs() * dk + U * normalize_bwd(xn, norm, dxn, eps).abs() + TINY


# ------------------------------------------------------------------------------------------------ correlation backward
def _corr_pieces(F, T, wta):
    """z = fl32(f' / T) formed in float32 — IEEE product and division: the kernel's bits — then float64: (z, keep-mask, T)."""
    assert F.dtype == torch.float32
    T32 = torch.tensor(T, dtype=torch.float32)
    raw = F.max(-1, keepdim=True)[0]
    keep = F == raw
    fw = F if wta == 1 else torch.where(keep, F, F * torch.tensor(wta, dtype=torch.float32))
    return (fw / T32).double(), keep, float(T32)


def softmax_fwd_y(F, blab, T, wta):
    """The forward's colour y [B, 3, rows] = p . B_lab that the backward kernel reads, from the same z."""
    z, _, _ = _corr_pieces(F, T, wta)
    return torch.matmul(torch.softmax(z, -1), blab.double().transpose(1, 2)).transpose(1, 2)


def softmax_bwd(F, blab, gy, y, gsim, argmax, T, wta, with_bound=False):
    """dvc_corr_softmax_bwd (header of corr_bwd.hip): F [B, rows, P] float32, blab [B, 3, P], gy, y [B, 3, rows], gsim [B, rows]
    or None with argmax [B, rows]:
        p = softmax_j z,  dS = p (g . B_j - g . y_i) / T,  times the constant 1e-4 off the RAW row maximum when wta != 1,
        plus gsim_i at the arg-max column, unscaled.
    with_bound: also the per-element bound
        d(exp) <= ex (u |z - m| + 2 u) + 2^-126;  dl <= sum + NR l;  p relative: ep = u |z - m| + 2 u + dl / l + u
        c = g . B_j - g . y_i:  dc <= 3 u (sum_k |g_k B_kj| + sum_k |g_k y_ki|) + u |c|
        d(dS) <= [p (dc + |c| (ep + 2 u)) + 2^-126 |c| / l] / T, (* 1e-4 + 2 u |dS| where scaled), + u |dS| where gsim lands."""
    z, keep, Tf = _corr_pieces(F, T, wta)
    P = F.shape[-1]
    zm = z - z.max(-1, keepdim=True)[0]
    ex = torch.exp(zm)
    l = ex.sum(-1, keepdim=True)
    p = ex / l
    gy, y, blab = gy.double(), y.double(), blab.double()
    G = torch.einsum("bki,bkj->bij", gy, blab)
    delta = (gy * y).sum(1).unsqueeze(-1)
    c = G - delta
    v = p * c / Tf
    scaled = ~keep if wta != 1 else torch.zeros_like(keep)
    v = torch.where(scaled, v * 1e-4, v)
    hit = onehot(argmax.long(), P) if gsim is not None else None
    if gsim is not None:
        v = v + gsim.double().unsqueeze(-1) * hit
    if not with_bound:
        return v
    dex = ex * (U * zm.abs() + 2 * U) + TINY
    dl = dex.sum(-1, keepdim=True) + NR(P) * l
    ep = U * zm.abs() + 3 * U + dl / l
    dc = 3 * U * (torch.einsum("bki,bkj->bij", gy.abs(), blab.abs()) + (gy * y).abs().sum(1).unsqueeze(-1)) + U * c.abs()
    dv = (p * (dc + c.abs() * (ep + 2 * U)) + TINY * c.abs() / l) / Tf
    dv = torch.where(scaled, dv * 1e-4 + 2 * U * v.abs(), dv)
    if gsim is not None:
        dv = dv + U * v.abs() * hit
    return v, dv + TINY


def ulp32(x):
    """Spacing of float32 at |x| (x: float64 tensor of normal magnitude)."""
    return torch.tensor([2.0 ** (math.frexp(abs(float(t)))[1] - 24) for t in x.flatten()], dtype=torch.float64).view(x.shape)
