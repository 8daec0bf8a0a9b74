"""numpy restatement of csrc/bgemm_split3.hip's arithmetic: the exact split of an fp32 value into three bf16 terms, and the
eight-product sum in float64 (exact products, exact sums: what the kernel computes before any fp32 rounding), plus the exact
integer and one-hot cases that tests/test_bgemm_split3_host.py checks against this restatement and
tests/test_gpu_bgemm_split3.py against the kernel."""
import functools

import numpy as np

U = 2.0 ** -24
BF16_MAX = np.float32(float.fromhex("0x1.fep127"))


def bf16_rn(x):
    """float32 -> the nearest bf16 (ties to even), as float32.  Finite input whose rounding stays finite."""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    r = (u + 0x7fff + ((u >> 16) & 1)) & 0xffff0000
    return r.astype(np.uint32).view(np.float32)


def is_bf16(t):
    return (np.ascontiguousarray(t, dtype=np.float32).view(np.uint32) & 0xffff) == 0


def split3(x):
    """x1 = bf16(clamp(x, +-BF16_MAX)), x2 = bf16(x - x1), x3 = bf16(x - x1 - x2); the subtractions in float32, as on the device."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    x1 = bf16_rn(np.clip(x, -BF16_MAX, BF16_MAX))
    r1 = x - x1
    x2 = bf16_rn(r1)
    r2 = r1 - x2
    return x1, x2, bf16_rn(r2)


def kept_products(A, B):
    """[.., M, K] x [.., K, N] in float64: a1 b1 + (a3 b2 + a2 b3 + a3 b1 + a2 b2 + a1 b3 + a2 b1 + a1 b2), the kernel's eight
    terms and its grouping."""
    a1, a2, a3 = (t.astype(np.float64) for t in split3(A))
    b1, b2, b3 = (t.astype(np.float64) for t in split3(B))
    low = a3 @ b2 + a2 @ b3 + a3 @ b1 + a2 @ b2 + a1 @ b3 + a2 @ b1 + a1 @ b2
    return a1 @ b1 + low


def dropped(a, b):
    """What the kernel drops, a3 b3, elementwise in float64 (exact: a product of two 8-bit significands)."""
    a3, b3 = split3(a)[2].astype(np.float64), split3(b)[2].astype(np.float64)
    return a3 * b3


def dropped_with_the_cross_terms(a, b):
    """a2 b3 + a3 b2 + a3 b3: what a six-product kernel would drop (the reason the kernel computes eight)."""
    _, a2, a3 = (t.astype(np.float64) for t in split3(a))
    _, b2, b3 = (t.astype(np.float64) for t in split3(b))
    return a2 * b3 + a3 * b2 + a3 * b3


@functools.lru_cache(maxsize=None)
def split_inputs():
    """10^6 random fp32 values, exponents uniform over [-100, 127], random signs and significands; then +-FLT_MAX, +-0, every
    power of two from 2^-100 to 2^127, and the values with all 24 significand bits set at those exponents."""
    rng = np.random.default_rng(20240)
    n = 10 ** 6
    bits = (rng.integers(0, 2, n, dtype=np.uint64) << 31) | (rng.integers(27, 255, n, dtype=np.uint64) << 23) \
        | rng.integers(0, 1 << 23, n, dtype=np.uint64)
    rand = bits.astype(np.uint32).view(np.float32)
    fmax = np.finfo(np.float32).max
    e = np.arange(-100, 128)
    pow2 = np.ldexp(np.float32(1), e).astype(np.float32)
    ones = (np.ldexp(np.float64(2 - 2.0 ** -23), e)).astype(np.float32)
    x = np.concatenate([rand, [fmax, -fmax, 0.0, -0.0], pow2, -pow2, ones, -ones]).astype(np.float32)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def integer_cases():
    """{name: (A [M, K], B [K, N], C [M, N])} float32, C = A B exactly (from an int64 product, or the selected elements).
      two_planes   A, B integers in +-(2^11 - 1), K = 4: two terms each — needs a1 b1, a1 b2, a2 b1, a2 b2
      a_three      A in +-(2^19 - 1) (three terms), B in +-7, K = 2 — needs a3 b1
      b_three      the roles swapped — needs a1 b3
      a2b3         A = +-2^j (2^10 + 1, -2^10) (two terms), B = +-(2^20 + 2^10 + 1, 2^20 + 2^10) (three), K = 2 — needs a2 b3
      a3b2         the roles swapped — needs a3 b2
      b_one_hot_K  B = one-hot columns of 1.0, A random full-precision fp32: C[m][n] = A[m][sel[n]]   (K = 17, 70)
      a_one_hot_K  A = one-hot rows: C[m][n] = B[sel[m]][n]
    M, N in {33, 130} (one tile with tails, two tiles with tails), both ways round."""
    rng = np.random.default_rng(7)
    cases = {}

    def ints(lim, *shape):
        return rng.integers(-lim, lim + 1, shape).astype(np.int64)

    for M, N in ((33, 130), (130, 33)):
        for name, la, lb, K in (("two_planes", 2 ** 11 - 1, 2 ** 11 - 1, 4), ("a_three", 2 ** 19 - 1, 7, 2),
                                ("b_three", 7, 2 ** 19 - 1, 2)):
            A, B = ints(la, M, K), ints(lb, K, N)
            A[0, :], B[:, 0] = la, -lb                                      # the extremes meet at C[0][0]
            C = A @ B
            assert np.abs(C).max() <= 2 ** 24
            cases[f"{name}_{M}x{N}"] = (A.astype(np.float32), B.astype(np.float32), C.astype(np.float32))
        # two terms against three with the large products cancelling over K = 2:
        # (2^10 + 1)(2^20 + 2^10 + 1) - 2^10 (2^20 + 2^10) = 2^20 + 2^11 + 1, whose last 1 is (the second term) x (the third)
        two = np.array([2 ** 10 + 1, -2 ** 10], np.int64)
        three = np.array([2 ** 20 + 2 ** 10 + 1, 2 ** 20 + 2 ** 10], np.int64)
        s = (rng.choice([-1, 1], M) * 2 ** rng.integers(0, 3, M)).astype(np.int64)
        t = rng.choice([-1, 1], N).astype(np.int64)
        for name, A, B in (("a2b3", s[:, None] * two[None, :], three[:, None] * t[None, :]),
                           ("a3b2", s[:, None] * three[None, :], two[:, None] * t[None, :])):
            C = A @ B
            assert np.abs(C).max() < 2 ** 24 and (np.abs(C) % 2 == 1).any()
            cases[f"{name}_{M}x{N}"] = (A.astype(np.float32), B.astype(np.float32), C.astype(np.float32))
        for K in (17, 70):
            A = rng.standard_normal((M, K)).astype(np.float32)
            sel = rng.integers(0, K, N)
            sel[:2] = (K - 1, 0)
            B = np.zeros((K, N), np.float32)
            B[sel, np.arange(N)] = 1.0
            cases[f"b_one_hot_{K}_{M}x{N}"] = (A, B, A[:, sel].copy())
            Bm = rng.standard_normal((K, N)).astype(np.float32)
            sel = rng.integers(0, K, M)
            sel[:2] = (K - 1, 0)
            Am = np.zeros((M, K), np.float32)
            Am[np.arange(M), sel] = 1.0
            cases[f"a_one_hot_{K}_{M}x{N}"] = (Am, Bm, Bm[sel, :].copy())
    for t in cases.values():
        for a in t:
            a.setflags(write=False)
    return cases
