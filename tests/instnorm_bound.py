"""Shared by tests/test_cabi_and_host.py (CPU) and tests/test_gpu_glue_edges.py (GPU): the inputs of the InstanceNorm
mean / sigma sweep, the float64 reference and the error bound of the kernels' form y = fma(x, sc, sh).

csrc/norm_pool.hip computes the statistics of a plane in float64 and applies them as x * sc + sh with sc = fl(rstd),
sh = fl(-mean * rstd), both rounded to float32 once.  With u = 2^-24 (half an ulp, relative):
    |x * (sc - rstd)|        <= u * |x| * rstd              (rounding of sc)
    |sh + mean * rstd|       <= u * |mean| * rstd            (rounding of sh;  |mean| <= max|x|)
    |fl(y') - y'|            <= u * |y'|                     (the one rounding of the fused multiply-add)
so |y_kernel - y| <= u * (2 * max|x| * rstd + max|y|) + O(u^2) <= 2^-23 * (max|x| * rstd + max|y| + 1) per plane: the `+ 1`
absorbs the second-order terms and the float64 statistics' own error.  ATen's (x - mean) * rstd has no term in
max|x| * rstd, which is why the error of this form grows with |mean| / sigma and ATen's does not.
"""
import numpy as np

EPS = 1e-5
RATIOS = (1, 10, 100, 1000)
SHAPE = (26, 48)


def sweep_plane(R):
    """The [26][48] float32 plane of ratio R: sigma = 1, mean = R (standard normal draws + R, rounded to float32)."""
    rng = np.random.default_rng(1000 + R)
    return (rng.standard_normal(SHAPE) + float(R)).astype(np.float32)


def reference(x, eps=EPS):
    """(y, rstd, mean) of InstanceNorm2d (biased variance, no affine) on the float32 plane x, in float64."""
    x = x.astype(np.float64)
    mean = x.mean()
    rstd = 1.0 / np.sqrt(((x - mean) ** 2).mean() + eps)
    return (x - mean) * rstd, rstd, mean


def bound(x, eps=EPS):
    y, rstd, _ = reference(x, eps)
    return 2.0 ** -23 * (np.abs(x.astype(np.float64)).max() * rstd + np.abs(y).max() + 1.0)


def emulate_fma(x, eps=EPS):
    """fma(x, sc, sh) as a correct implementation evaluates it: exact product and sum (float64 holds the 48-bit product of two
    float32 values exactly; the sum's own float64 rounding is 2^-29 of an fp32 ulp) of the float32-rounded sc and sh, rounded
    to float32 once."""
    _, rstd, mean = reference(x, eps)
    sc = np.float32(rstd)
    sh = np.float32(-mean * rstd)
    return (x.astype(np.float64) * np.float64(sc) + np.float64(sh)).astype(np.float32)
