"""The shared device arithmetic (orbfe_common.hpp, orbfe_cvmat.hpp, orbfe_jacobi4.hpp, orbfe_jacobi_wave.hpp), helper by helper, bit for bit.

Every kernel of the project inherits its bit-exact claim from these helpers, and the scene suites feed them a few thousand keypoints
and a few hundred matrices: a contraction that comes back with a flag, a sqrt lowering one ulp off, a DPP step that loses the minimum
of one lane are rare per input and would leave those suites green.  tests/arith_blocks/arith_blocks.hip (test-only, the product's
compiler flags, the product's headers as they are) runs one helper per kernel and stores raw bits; the inputs are exhaustive where
the domain allows it and adversarial where it does not.

Every comparison is on bit patterns; there are no tolerances.  One rule goes with that: where an INPUT makes an arithmetic step
produce a NaN, which sign and payload the NaN carries is the processor's choice (x86 and gfx950 differ), so both sides of such a
comparison give every NaN one pattern (host_forms.bits_one_nan) -- the contract's own rule for stored NaNs.  one_nan itself is
compared raw.

References: the oracle's scalar routines through their array forms (atan2, sincos, reflect101), numpy's IEEE operations on the CPU
(sqrt, division, conversions), tests/cvmat_model.py (products, inverse, determinant, norm, unit, the Jacobi) and explicit float64
restatements in index order written out below.  small_div is checked on the device in integer arithmetic.

The CPU tests show that the array forms equal the scalar forms, that the case lists hold what they are there for, that a contracted
evaluation (one fused multiply-add in place of a product and a sum, emulated in exact rationals) WOULD change the bits of the det3
and arctangent cases, and that the three test harnesses compile with the product's flags.
"""
import ctypes as C
import os
import re
from fractions import Fraction

import numpy as np
import pytest

from oracle import oracle as O
from tests import cvmat_model as M
from tests import host_forms as H
from tests import test_cvmat_model as K

HERE = os.path.dirname(os.path.abspath(__file__))
F32, F64, U32, U64, I32 = np.float32, np.float64, np.uint32, np.uint64, np.int32
(OP_ATAN2, OP_SINCOS, OP_SMALL_DIV, OP_REFLECT101, OP_ROW_SUM, OP_WAVE_SUM, OP_WAVE_MIN_DPP, OP_WAVE_MIN, OP_SCAN, OP_DSQRT, OP_DDIV, OP_FDIV,
 OP_SQRT_RN, OP_D2F, OP_D2I, OP_MAT3, OP_JACOBI_3_4, OP_JACOBI_9_16, OP_NULL4) = range(1, 20)
MAT3_IN = np.dtype([("a", F32, 9), ("b", F32, 9), ("v", F32, 3), ("T", F32, 12), ("x", F32, 3), ("plus", F32, 3), ("pad", F32),
                    ("alpha", F64), ("nom", F64), ("den", F64)])
MAT3_OUT = np.dtype([("ab", F32, 9), ("ab_alpha", F32, 9), ("inv", F32, 9), ("unit", F32, 3), ("stored", F32, 9), ("av", F32, 3), ("rwc_plus", F32, 3),
                     ("rwc", F32, 3), ("row_dot", F32, 3), ("reduce", F32), ("ratio", F32), ("fin", U32, 9), ("pad", U32, 2),
                     ("det", F64), ("norm", F64), ("dot", F64), ("sum_sq", F64)])
assert MAT3_IN.itemsize == 184 and MAT3_OUT.itemsize == 288
OT_THREADS = 512                                    # the block size of block_excl_scan's only caller, octree_generic_kernel


def jacobi_out(n):
    return np.dtype([("At", F32, (n, M.AS)), ("Vt", F32, (n, M.VS)), ("pad", F32, ((n * (M.AS + M.VS)) % 2,)), ("W", F64, n)])


NULL4_OUT = np.dtype([("v", F32, 4), ("Vt", F32, (4, 4)), ("W", F64, 4)])
assert jacobi_out(3).itemsize == 328 and jacobi_out(9).itemsize == 976 and NULL4_OUT.itemsize == 112


def _lib():
    path = os.path.join(HERE, "arith_blocks", "libarith_blocks.so")
    if not os.path.exists(path):
        raise RuntimeError("tests/arith_blocks/libarith_blocks.so is missing: __graft_entry__.build() compiles it")
    L = C.CDLL(path)
    L.arith_blocks_run.restype = C.c_int
    L.arith_blocks_run.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    return L


def _run(op, n, inputs, out_dtype, out_count):
    """`inputs`: arrays laid one after the other (planar)."""
    a = np.concatenate([np.ascontiguousarray(x).reshape(-1).view(np.uint8) for x in inputs])
    out = np.zeros(out_count, out_dtype)
    assert _lib().arith_blocks_run(op, n, a.ctypes.data, out.ctypes.data) == 0
    return out


def _assert_same_bits(got, want, what, inputs=()):
    """Equal as bit patterns; the first mismatches are named with their inputs."""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    u = {1: np.uint8, 4: U32, 8: U64}[got.dtype.itemsize]
    bad = np.flatnonzero(got.view(u).reshape(-1) != want.view(u).reshape(-1))
    print("%s: %d values, %d mismatches" % (what, got.size, len(bad)))
    if len(bad):
        first = [(int(i), [np.asarray(x).reshape(-1)[i].item() for x in inputs if np.asarray(x).size == got.size],
                  hex(int(got.view(u).reshape(-1)[i])), hex(int(want.view(u).reshape(-1)[i]))) for i in bad[:5]]
        raise AssertionError("%s: %d of %d differ; (index, inputs, device, reference) %s" % (what, len(bad), got.size, first))


def _one_nan(a):
    a = np.array(a)
    return np.frombuffer(H.bits_one_nan(a).tobytes(), a.dtype).reshape(a.shape)


# ================================================================ cases (shared by the CPU and the GPU tests)

def atan_bound():
    """The largest |m10| (and |m01|) IC_Angle can form: 255 times the sum of u over the positive half of every row of the patch."""
    umax = O.Extractor().umax().astype(np.int64)
    per_row = umax * (umax + 1) // 2                            # 1 + 2 + ... + umax[v]
    return int(255 * (per_row[0] + 2 * per_row[1:].sum()))       # row 0 once, rows +-v


def atan_grid():
    r = np.arange(-1024, 1025, dtype=F32)
    y, x = np.meshgrid(r, r, indexing="ij")
    return y.reshape(-1).copy(), x.reshape(-1).copy()


def atan_seeded(count=1 << 22):
    B = atan_bound()
    v = np.random.default_rng(11).integers(-B, B + 1, size=(2, count))
    return v[0].astype(F32), v[1].astype(F32)


def atan_rays():
    B = atan_bound()
    m = np.unique(np.concatenate([np.round(np.geomspace(1, B, 4096)), [1, 2, B]])).astype(np.int64)
    m = np.concatenate([m, np.random.default_rng(12).integers(1, B + 1, 4096 - len(m))])       # 4096 magnitudes in all, log-spaced and B itself among them
    pairs = [(0 * m[:1], 0 * m[:1])]
    for sy in (1, -1):
        for sx in (1, -1):
            pairs += [(sy * m, sx * m), (sy * m, sx * (m - 1)), (sy * (m - 1), sx * m)]
        pairs += [(0 * m, sy * m), (sy * m, 0 * m)]
    return np.concatenate([p[0] for p in pairs]).astype(F32), np.concatenate([p[1] for p in pairs]).astype(F32)


FACTOR_PI = F32(np.pi / F64(F32(180.0)))                        # (float)(CV_PI / 180.f)
SINCOS_TOP = F32(360.0) * FACTOR_PI                             # fl(360 * factor_pi): no angle of fast_atan2_deg gives more
SINCOS_BINADES = [0.125, 0.25, 0.5, 1.0, 2.0, 4.0]


def _floats_between(lo, hi, step=1):
    """Every `step`-th float32 from lo to hi, both included when the step meets them."""
    a, b = int(np.array(lo, F32).view(U32)), int(np.array(hi, F32).view(U32))
    return np.arange(a, b + 1, step, dtype=np.int64).astype(U32).view(F32)


def sincos_binade(lo):
    hi = min(np.nextafter(F32(2 * lo), F32(0)), SINCOS_TOP)
    return _floats_between(F32(lo), hi)


def sincos_small():
    return _floats_between(F32(2.0 ** -20), F32(0.125), 64)


def sincos_special():
    neg = -np.random.default_rng(13).random(1 << 16, F32)       # the routine is valid from -1
    sp = np.array([0x00000000, 0x80000000, 0x00800000, 0x00000001, 0x00400123], U32).view(F32)   # +0, -0, the smallest normal, denormals
    return np.concatenate([sp, neg, np.array([-1.0], F32)])


def small_div_divisors():
    extra = np.random.default_rng(14).integers(4097, (1 << 21) + 1, 4096)
    extra[:2] = [4097, 1 << 21]
    return np.concatenate([np.arange(1, 4097), extra]).astype(I32)


def reflect_cases():
    ps, ls = [], []
    for ln in range(1, 65):
        p = np.arange(-24, ln + 24)
        ps.append(p); ls.append(np.full(len(p), ln))
    return np.concatenate(ps).astype(I32), np.concatenate(ls).astype(I32)


def wave_vectors():
    """uint32[n][64].  The unique minimum in each lane in turn (small values, then everything >= 2^31); the minimum twice, in two
    different rows of 16 lanes (every pair of rows); sums of negative values and sums that wrap; 4096 seeded vectors."""
    rng = np.random.default_rng(15)
    out = []
    for base in (1000, 1 << 31):
        v = rng.integers(base + 1000, 1 << 32, size=(64, 64), dtype=np.uint64)
        v[np.arange(64), np.arange(64)] = base + rng.integers(0, 1000, 64).astype(np.uint64)
        out.append(v)
    dup = []
    for r1 in range(4):
        for r2 in range(r1 + 1, 4):
            for _ in range(8):
                base = (r1 & 1) << 31                               # half of them with everything >= 2^31
                v = rng.integers(base + 1000, 1 << 32, size=64, dtype=np.uint64)
                v[16 * r1 + rng.integers(0, 16)] = v[16 * r2 + rng.integers(0, 16)] = base + 77
                dup.append(v)
    out.append(np.array(dup))
    out.append(np.stack([np.full(64, 0xFFFFFFFF), np.full(64, 0x80000000), np.full(64, 0x7FFFFFFF), np.arange(64) + 0xFFFFFF00,
                         0x7FFFFFFF - np.arange(64), np.where(np.arange(64) % 2, 0x80000000, 0x7FFFFFFF)]).astype(np.uint64))
    out.append((-rng.integers(1, 1 << 31, size=(64, 64))).astype(np.int64).astype(np.uint64) & np.uint64(0xFFFFFFFF))   # negative ints
    out.append(rng.integers(0, 1 << 32, size=(4096, 64), dtype=np.uint64))
    return np.concatenate(out).astype(U32)


def wave_reference(op, v):
    v64 = v.astype(np.uint64)
    if op == OP_ROW_SUM:
        rows = v64.reshape(-1, 4, 16).sum(axis=2) & np.uint64(0xFFFFFFFF)          # int32 arithmetic modulo 2^32
        return np.repeat(rows, 16, axis=1).astype(U32)
    if op == OP_WAVE_SUM:
        return np.repeat((v64.sum(axis=1) & np.uint64(0xFFFFFFFF))[:, None], 64, axis=1).astype(U32)
    return np.repeat(v.min(axis=1)[:, None], 64, axis=1)


SCAN_CASES = [(n, alias, lds) for n in (0, 1, OT_THREADS - 1, OT_THREADS, OT_THREADS + 1, 5 * OT_THREADS + 3) for alias in (0, 1) for lds in (0, 1)]


def scan_source(n):
    return np.random.default_rng(16 + n).integers(-(1 << 18), 1 << 18, n).astype(I32)     # 2563 * 2^18 < 2^31: no signed overflow


def _finite64(rng, count):
    b = rng.integers(0, 1 << 64, count, dtype=np.uint64)
    b[(b >> np.uint64(52)) & np.uint64(0x7FF) == 0x7FF] &= np.uint64(0xBFFFFFFFFFFFFFFF)   # Inf / NaN: clear an exponent bit
    b[:count // 16] &= np.uint64(0x800FFFFFFFFFFFFF)                                        # a sixteenth denormal
    return b.view(F64)


def _finite32(rng, count):
    b = rng.integers(0, 1 << 32, count, dtype=np.uint64).astype(U32)
    b[(b >> 23) & 0xFF == 0xFF] &= U32(0xBFFFFFFF)
    b[:count // 16] &= U32(0x807FFFFF)
    return b.view(F32)


def _short_mantissa64(rng, count, bits, lo=-300, hi=300):
    """Doubles with a `bits`-bit significand: the product of two (and a square) with bits <= 26 is exact."""
    return np.ldexp(rng.integers(1 << (bits - 1), 1 << bits, count).astype(F64), rng.integers(lo, hi, count))


def ieee_cases(op, seeded=1 << 22, hard=1 << 16):
    """The inputs of one primitive: `seeded` finite bit patterns (a sixteenth of them denormal) and the hard cases: exact squares /
    products with their neighbours one ulp either side, arguments in the denormal range and quotients that land in it.  (No root of a
    representable number lands in the denormal range: sqrt(2^-1074) = 2^-537.  The denormal ARGUMENTS stand for that item.)"""
    rng = np.random.default_rng(20 + op)
    up64 = lambda v: np.nextafter(v, F64(np.inf))
    dn64 = lambda v: np.nextafter(v, F64(-np.inf))
    up32 = lambda v: np.nextafter(v, F32(np.inf))
    dn32 = lambda v: np.nextafter(v, F32(-np.inf))
    if op == OP_DSQRT:
        sq = np.square(_short_mantissa64(rng, hard, 26))
        den = (rng.integers(1, 1 << 52, hard, dtype=np.uint64)).view(F64)
        return (np.concatenate([_finite64(rng, seeded), sq, up64(sq), dn64(sq), den, np.array([0.0, -0.0, 5e-324, np.finfo(F64).tiny, np.finfo(F64).max])]),)
    if op == OP_DDIV:
        y, z = _short_mantissa64(rng, hard, 26, -200, 200), _short_mantissa64(rng, hard, 26, -200, 200)
        p = y * z
        small, big = _short_mantissa64(rng, hard, 53, -1062, -1042), _short_mantissa64(rng, hard, 53, -32, 8)      # 2^-1010 .. 2^-990 over 2^20 .. 2^60: quotients around 2^-1070 .. 2^-1010
        sa, sb = np.array([0.0, -0.0, 1.0, 0.0, 5e-324, 1.0, np.finfo(F64).max]), np.array([1.0, 3.0, 0.0, 0.0, 2.0, 3.0, 0.5])
        return (np.concatenate([_finite64(rng, seeded), p, up64(p), dn64(p), small, sa]), np.concatenate([_finite64(rng, seeded), z, z, z, big, sb]))
    if op == OP_FDIV:
        y = np.ldexp(rng.integers(1 << 11, 1 << 12, hard).astype(F32), rng.integers(-40, 40, hard)).astype(F32)
        z = np.ldexp(rng.integers(1 << 11, 1 << 12, hard).astype(F32), rng.integers(-40, 40, hard)).astype(F32)
        p = (y * z).astype(F32)
        small = np.ldexp(rng.integers(1 << 23, 1 << 24, hard).astype(F32), rng.integers(-145, -120, hard)).astype(F32)   # quotients around 2^-150 .. 2^-100
        big = np.ldexp(rng.integers(1 << 23, 1 << 24, hard).astype(F32), rng.integers(-23, 10, hard)).astype(F32)
        sa, sb = np.array([0.0, -0.0, 1.0, 0.0, 1e-45, 1.0], F32), np.array([1.0, 3.0, 0.0, 0.0, 2.0, 3.0], F32)
        return (np.concatenate([_finite32(rng, seeded), p, up32(p), dn32(p), small, sa]), np.concatenate([_finite32(rng, seeded), z, z, z, big, sb]))
    if op == OP_SQRT_RN:
        y = np.ldexp(rng.integers(1 << 11, 1 << 12, hard).astype(F32), rng.integers(-50, 50, hard)).astype(F32)
        sq = (y * y).astype(F32)
        den = rng.integers(1, 1 << 23, hard).astype(U32).view(F32)
        return (np.concatenate([_finite32(rng, seeded), sq, up32(sq), dn32(sq), den, np.array([0.0, -0.0, 1e-45, np.finfo(F32).tiny, np.finfo(F32).max], F32)]),)
    if op == OP_D2F:
        # half the seeded patterns span the double range (overflow to Inf, underflow to 0); the other half are a float plus low bits, one in
        # eight an exact tie, one in eight in the float denormal range
        f = _finite32(rng, seeded // 2).astype(F64).view(np.uint64)
        low = rng.integers(0, 1 << 29, seeded // 2, dtype=np.uint64)
        low[::8] = 1 << 28
        mid = (f | low).view(F64)
        mid[1::8] = np.ldexp(rng.random(len(mid[1::8])) + 1, rng.integers(-152, -125, len(mid[1::8])))
        edge = np.array([np.finfo(F32).max, np.nextafter(F64(np.finfo(F32).max), np.inf), float.fromhex("0x1.ffffffp127"), float.fromhex("0x1.fffffefffffffp127"),
                         2.0 ** -150, np.nextafter(F64(2.0 ** -150), 1.0), 2.0 ** -149, 1.5 * 2.0 ** -149, 0.0, -0.0, 5e-324])
        return (np.concatenate([_finite64(rng, seeded // 2), mid, edge, -edge]),)
    assert op == OP_D2I
    wide = rng.uniform(-2147483648.0, 2147483648.0, seeded)
    wide = wide[(wide > -2147483649.0) & (wide < 2147483648.0)]
    frac = rng.integers(-(1 << 20), 1 << 20, hard) + rng.choice([0.0, 0.5, -0.5, 0.999999, -0.999999, 2.0 ** -30], hard)
    edge = np.array([0.0, -0.0, 0.9999999999999999, -0.9999999999999999, 2147483647.0, 2147483647.9999995, -2147483648.0, -2147483648.9999995, 5e-324, -5e-324])
    return (np.concatenate([wide, frac, rng.uniform(-1, 1, hard), edge]),)


def ieee_reference(op, args):
    with np.errstate(all="ignore"):
        if op == OP_DSQRT: return np.sqrt(args[0])
        if op == OP_DDIV: return args[0] / args[1]
        if op == OP_FDIV: return (args[0] / args[1]).astype(F32)
        if op == OP_SQRT_RN: return np.sqrt(args[0])                    # numpy's float32 sqrt is the correctly rounded one (sqrtss)
        if op == OP_D2F: return args[0].astype(F32)
        return np.trunc(args[0]).astype(np.int64).astype(I32)           # (int): toward zero


def mat3_cases():
    """Mat3In records: small_inputs(), then seeded_small_inputs() of tests/test_cvmat_model.py (4096 full-mantissa, the exactly singular,
    the nearly singular, the STORED patterns).  v, T, x, plus3 and the two doubles are drawn from the same matrices and a seed."""
    S = K.small_inputs()
    a2, b2, p2, al2 = K.seeded_small_inputs()
    a = np.concatenate([np.stack([s[0] for s in S]), a2])
    b = np.concatenate([np.stack([s[1] for s in S]), b2])
    plus = np.concatenate([np.stack([s[2] for s in S]), p2])
    alpha = np.concatenate([[s[3] for s in S], al2])
    n = len(a)
    rng = np.random.default_rng(17)
    c = np.zeros(n, MAT3_IN)
    c["a"], c["b"], c["alpha"] = a.reshape(n, 9), b.reshape(n, 9), alpha
    c["v"] = a[:, 0]                                                    # the row the host form's Unit and Norm3 take
    c["T"] = np.concatenate([b, plus[:, :, :1]], axis=2).reshape(n, 12)
    c["T"][-6:, :9] = a[-6:].reshape(6, 9)                              # the STORED patterns reach the Tcw products too
    c["x"], c["plus"] = plus[:, 1], plus[:, 2]
    c["nom"], c["den"] = rng.normal(size=n), rng.normal(size=n)
    c["den"][:8] = [0.0, -0.0, 0.0, 1e300, 1e-300, 3.0, 1e38, 2.0 ** 127]
    c["nom"][:8] = [0.0, 1.0, -1.0, 1e-300, 1e300, 1.0, 1e-7, 2.0 ** -22]       # 0 / 0, +-Inf, underflow, overflow, a third, float denormals
    return c


def mat3_reference(c):
    """MAT3_OUT records: the model where it has the step, else a float64 restatement in index order with one rounding."""
    n = len(c)
    a, b, v, T, x, plus = (c[k].astype(F32) for k in ("a", "b", "v", "T", "x", "plus"))
    A, Bm = a.reshape(n, 3, 3), b.reshape(n, 3, 3)
    r = np.zeros(n, MAT3_OUT)
    d = lambda t: t.astype(F64)
    with np.errstate(all="ignore"):
        r["ab"] = M.mat(A, Bm).reshape(n, 9)
        r["ab_alpha"] = M.mat(A, Bm, alpha=c["alpha"]).reshape(n, 9)
        r["inv"] = M.inv3(A).reshape(n, 9)
        r["det"] = M.det3(A)
        r["norm"] = M.norm(v)
        r["unit"] = np.stack([M.unit(t) for t in v])
        r["stored"] = M.stored(a)
        for i in range(3):
            s = np.zeros(n, F64)
            for k in range(3):
                s = s + d(a[:, 3 * i + k]) * d(v[:, k])
            r["av"][:, i] = s.astype(F32)
            s = np.zeros(n, F64)
            for k in range(3):
                s = s + d(T[:, 4 * k + i]) * d(x[:, k])
            r["rwc"][:, i] = s.astype(F32)
            r["rwc_plus"][:, i] = (s + d(plus[:, i])).astype(F32)
            s = np.zeros(n, F64)
            for k in range(3):
                s = s + d(T[:, 4 * i + k]) * d(x[:, k])
            r["row_dot"][:, i] = (s + d(T[:, 4 * i + 3])).astype(F32)
        r["reduce"] = (a[:, 0] + a[:, 1]) + a[:, 2]
        r["ratio"] = (c["nom"] / c["den"]).astype(F32)
        r["fin"] = np.isfinite(a)
        s, q = np.zeros(n, F64), np.zeros(n, F64)
        for k in range(9):
            s = s + d(a[:, k]) * d(b[:, k])
            q = q + d(a[:, k] * a[:, k])
        r["dot"], r["sum_sq"] = s, q
    assert r["reduce"].dtype == F32
    return r


def jacobi_cases(n, m):
    """float32[B][m][n]: every matrix of jacobi_inputs() of that shape, ZERO_COLUMN at 3 x 3, and the seeded ones."""
    known = [A for A in K.jacobi_inputs() if A.shape == (m, n)]
    assert len(known) >= 9 and (n != 3 or any(np.array_equal(A, K.ZERO_COLUMN) for A in known))
    return np.concatenate([np.stack(known), K.seeded_jacobi_inputs(n, m)])


def transposed(As):
    """At float32[B][n][16] of matrices float32[B][m][n]."""
    B, m, n = As.shape
    At = np.zeros((B, n, M.AS), F32)
    At[:, :, :m] = As.transpose(0, 2, 1)
    return At


# ================================================================ CPU: the references and the case lists

def test_array_forms_of_the_oracle_equal_the_scalar_forms():
    L, rng = O.lib(), np.random.default_rng(1)
    y, x = (rng.integers(-4000, 4000, 10000).astype(F32) for _ in range(2))
    y[:3], x[:3] = [0, 0, -0.0], [0, -5, 0]
    got = O.fast_atan2_n(y, x)
    _assert_same_bits(got, np.array([L.orc_fast_atan2(float(a), float(b)) for a, b in zip(y, x)], F32), "atan2 array form")
    rad = np.concatenate([rng.uniform(-1, 8, 9998), [0.0, -0.0]]).astype(F32)
    s, c = O.sincos_det_n(rad)
    ws, wc = C.c_float(), C.c_float()
    want = []
    for r in rad:
        L.orc_sincos_det(float(r), C.byref(ws), C.byref(wc))
        want.append((ws.value, wc.value))
    _assert_same_bits(np.stack([s, c], 1), np.array(want, F32), "sincos array form")
    p, ln = rng.integers(-200, 400, 10000).astype(I32), rng.integers(1, 200, 10000).astype(I32)
    _assert_same_bits(O.border_reflect101_n(p, ln), np.array([L.orc_border_reflect101(int(a), int(b)) for a, b in zip(p, ln)], I32), "reflect101 array form")


def test_the_atan_bound_is_what_ic_angle_can_form_and_casts_exactly():
    B = atan_bound()
    u = O.Extractor().umax()
    assert len(u) == 16 and B == 255 * sum(abs(x) for v in range(-15, 16) for x in range(0, u[abs(v)] + 1))
    assert 0 < B < 1 << 24
    y, x = atan_rays()
    assert len(y) == 1 + 4096 * 16 and np.abs(y).max() == B and np.abs(x).max() == B and (y == 0).any() and (np.abs(x) == np.abs(y)).any()
    y, x = atan_seeded(1 << 12)
    assert np.abs(y).max() <= B and np.abs(y).max() > B // 2


def test_the_sincos_domain_is_every_float_of_every_binade_up_to_a_full_turn():
    assert FACTOR_PI.view(U32) == 0x3C8EFA35 and 6.28 < SINCOS_TOP < 6.2832
    total = 0
    for lo in SINCOS_BINADES:
        r = sincos_binade(lo)
        assert r[0] == F32(lo) and len(r) <= 1 << 23 and (np.diff(r.view(U32).astype(np.int64)) == 1).all()
        total += len(r)
    assert sincos_binade(4.0)[-1] == SINCOS_TOP and total == int(SINCOS_TOP.view(U32)) - int(F32(0.125).view(U32)) + 1
    s = sincos_small()
    assert s[0] == F32(2.0 ** -20) and s[-1] <= F32(0.125) and len(s) == 17 * (1 << 23) // 64 + 1
    sp = sincos_special()
    assert (sp < 0).sum() >= 1 << 16 and sp.min() == -1


def test_the_case_lists_hold_what_they_are_there_for():
    b = small_div_divisors()
    assert len(b) == 8192 and (b[:4096] == np.arange(1, 4097)).all() and b[4096:].min() == 4097 and b.max() == 1 << 21
    p, ln = reflect_cases()
    assert len(p) == sum(x + 48 for x in range(1, 65)) and p.min() == -24 and (p - ln).max() == 23
    v = wave_vectors()
    arg = v[:128].argmin(axis=1)
    assert (arg == np.tile(np.arange(64), 2)).all() and v[64:128].min() >= 1 << 31                 # the unique minimum, lane by lane
    dup = v[128:176]
    rows = sorted({tuple(np.flatnonzero(x == x.min()) // 16) for x in dup})
    assert rows == [(i, j) for i in range(4) for j in range(i + 1, 4)]                               # the minimum twice, every pair of rows
    assert (v.astype(np.int64).sum(axis=1) >= 1 << 32).any() and (v.view(I32) < 0).all(axis=1).any() and len(v) >= 4096
    for op in (OP_DSQRT, OP_DDIV, OP_FDIV, OP_SQRT_RN, OP_D2F, OP_D2I):
        args = ieee_cases(op)
        assert all(np.isfinite(a).all() and len(a) >= (1 << 22) - (1 << 12) and len(a) == len(args[0]) for a in args)
        if op != OP_D2I:
            tiny = np.finfo(args[0].dtype).tiny
            assert ((np.abs(args[0]) < tiny) & (args[0] != 0)).sum() >= 1 << 16                      # denormal arguments
        with np.errstate(all="ignore"):
            if op in (OP_DDIV, OP_FDIV):
                qq = ieee_reference(op, args)
                assert ((np.abs(qq) < np.finfo(qq.dtype).tiny) & (qq != 0)).sum() >= 1 << 15        # quotients in the denormal range
                exact = (args[0].astype(np.longdouble) == qq.astype(np.longdouble) * args[1].astype(np.longdouble)).sum()
                assert exact >= 1 << 16                                                              # y * z / z
    c = mat3_cases()
    with np.errstate(all="ignore"):
        det = M.det3(c["a"].reshape(-1, 3, 3))
    assert len(c) == 6 + 4096 + 4 * 512 + 6 and (det[6 + 4096:6 + 4096 + 1024] == 0).all()
    near = det[6 + 4096 + 1024:6 + 4096 + 1536]
    assert (near != 0).mean() > 0.9 and np.abs(near).max() < 1e-4
    cancel = np.abs(det[6 + 4096 + 1536:6 + 4096 + 2048])
    assert np.median(cancel) < 1e-6 and (cancel != 0).mean() > 0.9                                   # what cancellation leaves of terms of order 1
    assert np.isnan(c["a"][-6:]).any() and np.isinf(c["a"][-6:]).any()
    for n, m in K.SIZES:
        A = jacobi_cases(n, m)
        assert np.isnan(A).any(axis=(1, 2)).sum() == 1 and np.isinf(A).any(axis=(1, 2)).sum() == 1 and len(A) >= K.SEEDED + 9
        S = A[-K.SEEDED:]
        twins = sum(any((a[:, i] == a[:, j]).all() for i in range(n) for j in range(i + 1, n)) for a in S[:K.SEEDED // 4])
        assert twins == K.SEEDED // 4
        assert (S[K.SEEDED // 4:3 * K.SEEDED // 8] == 0).all(axis=1).any(axis=1).all() and (S[3 * K.SEEDED // 8:K.SEEDED // 2, n - 1:] == 0).all()


def test_the_mat3_restatements_agree_with_the_model_where_it_has_the_step():
    """mul3_vec, rwc_times and row_dot_plus are cv::Mat products: the restatement in mat3_reference gives the bits of M.mat."""
    c = mat3_cases()
    r = mat3_reference(c)
    n = len(c)
    with np.errstate(all="ignore"):
        A, v, T, x = c["a"].reshape(n, 3, 3), c["v"].reshape(n, 3, 1), c["T"].reshape(n, 3, 4), c["x"].reshape(n, 3, 1)
        _assert_same_bits(_one_nan(r["av"]), _one_nan(M.mat(A, v)[:, :, 0]), "mul3_vec restated")
        Rwc = T[:, :, :3].transpose(0, 2, 1)
        _assert_same_bits(_one_nan(r["rwc"]), _one_nan(M.mat(Rwc, x)[:, :, 0]), "rwc_times restated")
        _assert_same_bits(_one_nan(r["rwc_plus"]), _one_nan(M.mat(Rwc, x, plus=c["plus"].reshape(n, 3, 1))[:, :, 0]), "rwc_times + plus restated")
        _assert_same_bits(_one_nan(r["row_dot"]), _one_nan(M.mat(T[:, :, :3], x, plus=T[:, :, 3:])[:, :, 0]), "row_dot_plus restated")


# ================================================================ CPU: the cases can fail

def _rd64(fr):
    return Fraction(float(fr))                      # int / int true division is correctly rounded


def _rd32(fr):
    """A rational rounded to the nearest float32 (ties to even; normal range), as a rational."""
    if fr == 0:
        return fr
    e = 0
    while abs(fr) / Fraction(2) ** e >= 1 << 24: e += 1
    while abs(fr) / Fraction(2) ** e < 1 << 23: e -= 1
    assert e > -149
    return round(fr / Fraction(2) ** e) * Fraction(2) ** e      # round(): ties to even


def det3_contracted(m):
    """det3 as a compiler may contract it: x * y - z * w as fma(x, y, -(z * w)) (no change by itself: a product of two floats is exact in
    double), and the outer sum, whose products have a double factor, as two nested fmas."""
    f = [Fraction(float(v)) for v in np.asarray(m, F32).reshape(9)]
    m00, m01, m02, m10, m11, m12, m20, m21, m22 = f
    fma = lambda a, b, c: _rd64(a * b + c)
    t1, t2, t3 = fma(m11, m22, -_rd64(m12 * m21)), fma(m10, m22, -_rd64(m12 * m20)), fma(m10, m21, -_rd64(m11 * m20))
    return float(fma(m02, t3, fma(-m01, t2, _rd64(m00 * t1))))


def atan_contracted(y, x):
    """fast_atan2_deg with the Horner steps (and 90 - p * c) as fused multiply-adds."""
    p1, p3, p5, p7 = (Fraction(float(np.array(b, U32).view(F32))) for b in (0x4265226F, 0xC19556EE, 0x410E9FBF, 0xC0228AD9))
    eps = Fraction(float(F32(2.220446049250313e-16)))
    fx, fy = Fraction(float(x)), Fraction(float(y))
    ax, ay = abs(fx), abs(fy)
    fma = lambda a, b, c: _rd32(a * b + c)
    lo, hi = (ay, ax) if ax >= ay else (ax, ay)
    c = _rd32(lo / _rd32(hi + eps))
    c2 = _rd32(c * c)
    poly = fma(fma(fma(p7, c2, p5), c2, p3), c2, p1)
    a = _rd32(poly * c) if ax >= ay else fma(-poly, c, Fraction(90))
    if fx < 0: a = _rd32(180 - a)
    if fy < 0: a = _rd32(360 - a)
    return F32(float(a))


def test_a_contracted_det3_changes_the_bits_of_at_least_a_tenth_of_the_seeded_cases():
    a = K.seeded_small_inputs()[0][:2000]
    with np.errstate(all="ignore"):
        want = M.det3(a)
    diff = sum(F64(det3_contracted(m)).view(U64) != w.view(U64) for m, w in zip(a, want))
    print("contracted det3 differs on %d of %d" % (diff, len(a)))
    assert diff >= len(a) // 10


def test_a_contracted_det3_changes_the_inverse_of_at_least_a_tenth_of_the_cancelling_cases():
    """A float of inv3 hides a last-bit change of d (one in 2^29 shows) unless d is what cancellation left: then the change is large."""
    a = K.seeded_small_inputs()[0][4096 + 1536:4096 + 2048]
    m = a.astype(F64)
    m00, m01, m02, m10, m11, m12, m20, m21, m22 = [m[:, r, c] for r in range(3) for c in range(3)]

    def inverse(d):                                 # the cofactors are differences of exact products: a contraction changes only d
        with np.errstate(all="ignore"):
            d = F64(1.0) / d
            t = [(m11 * m22 - m12 * m21) * d, (m02 * m21 - m01 * m22) * d, (m01 * m12 - m02 * m11) * d, (m12 * m20 - m10 * m22) * d, (m00 * m22 - m02 * m20) * d,
                 (m02 * m10 - m00 * m12) * d, (m10 * m21 - m11 * m20) * d, (m01 * m20 - m00 * m21) * d, (m00 * m11 - m01 * m10) * d]
        return np.stack(t, axis=-1).astype(F32)

    with np.errstate(all="ignore"):
        d = M.det3(a)
        _assert_same_bits(_one_nan(inverse(d)[d != 0].reshape(-1, 3, 3)), _one_nan(M.inv3(a)[d != 0]), "the inverse restated")
    diff = (inverse(d).view(U32) != inverse(np.array([det3_contracted(x) for x in a])).view(U32)).any(axis=1).sum()
    print("contracted inv3 differs on %d of %d" % (diff, len(a)))
    assert diff >= len(a) // 10


def test_a_contracted_arctangent_changes_the_bits_of_at_least_a_hundredth_of_the_seeded_pairs():
    y, x = atan_seeded(2000)
    want = O.fast_atan2_n(y, x)
    plain = sum(atan_contracted(a, b).view(U32) != w.view(U32) for a, b, w in zip(y, x, want))
    print("contracted atan differs on %d of %d" % (plain, len(y)))
    assert plain >= len(y) // 100


# ================================================================ CPU: the harnesses compile with the product's flags

def _flags(makefile):
    text = open(os.path.join(os.path.dirname(HERE), makefile)).read().replace("\\\n", " ")
    lines = re.findall(r"^FLAGS\s*=(.*)$", text, re.M)
    assert len(lines) == 1, makefile
    return lines[0].split()


def test_the_harnesses_compile_with_the_flags_of_the_product():
    product = _flags("orbslam2_amd/csrc/Makefile")
    assert "-ffp-contract=off" in product and "-fhip-fp32-correctly-rounded-divide-sqrt" in product and "$(EXTRA)" in product
    for harness in ("arith_blocks", "pose_blocks", "sim3_blocks"):
        assert _flags("tests/%s/Makefile" % harness) == product, harness


# ================================================================ GPU

@pytest.mark.gpu
@pytest.mark.parametrize("cases", [atan_grid, atan_seeded, atan_rays])
def test_gpu_fast_atan2_deg_equals_the_oracle(cases):
    y, x = cases()
    got = _run(OP_ATAN2, len(y), (y, x), F32, len(y))
    _assert_same_bits(got, O.fast_atan2_n(y, x), "fast_atan2_deg " + cases.__name__, (y, x))


def _sincos(rad, what):
    got = _run(OP_SINCOS, len(rad), (rad,), F32, 2 * len(rad))
    s, c = O.sincos_det_n(rad)
    _assert_same_bits(got[:len(rad)], s, "sincos_det sin " + what, (rad,))
    _assert_same_bits(got[len(rad):], c, "sincos_det cos " + what, (rad,))


@pytest.mark.gpu
@pytest.mark.parametrize("lo", SINCOS_BINADES)
def test_gpu_sincos_det_equals_the_oracle_on_every_float_of_a_binade(lo):
    _sincos(sincos_binade(lo), "binade of %g" % lo)


@pytest.mark.gpu
def test_gpu_sincos_det_equals_the_oracle_below_an_eighth_and_on_the_special_arguments():
    _sincos(sincos_small(), "every 64th float below 0.125")
    _sincos(sincos_special(), "zeros, denormals, negative arguments")


@pytest.mark.gpu
def test_gpu_small_div_is_the_floor_quotient_on_its_whole_domain():
    b = small_div_divisors()
    out = _run(OP_SMALL_DIV, len(b), (b,), U64, 2)
    first = None if out[1] == np.uint64(0xFFFFFFFFFFFFFFFF) else (int(out[1]) >> 32, int(out[1]) & 0xFFFFFFFF)
    print("small_div: %d divisors x 2^21 dividends, %d mismatches, first (a, b) %s" % (len(b), int(out[0]), first))
    assert int(out[0]) == 0 and first is None, (int(out[0]), first)


@pytest.mark.gpu
def test_gpu_reflect101_equals_the_oracle():
    p, ln = reflect_cases()
    _assert_same_bits(_run(OP_REFLECT101, len(p), (p, ln), I32, len(p)), O.border_reflect101_n(p, ln), "reflect101", (p, ln))


@pytest.mark.gpu
@pytest.mark.parametrize("op,name", [(OP_ROW_SUM, "row_sum_i32"), (OP_WAVE_SUM, "wave_sum_i32"), (OP_WAVE_MIN_DPP, "wave_min_u32_dpp"), (OP_WAVE_MIN, "wave_min_u32")])
def test_gpu_dpp_reductions(op, name):
    v = wave_vectors()
    got = _run(op, len(v), (v,), U32, v.size).reshape(v.shape)
    _assert_same_bits(got, wave_reference(op, v), name, (v,))


@pytest.mark.gpu
@pytest.mark.parametrize("n,alias,lds", SCAN_CASES)
def test_gpu_block_excl_scan(n, alias, lds):
    src = scan_source(n)
    out = _run(OP_SCAN, n, (np.array([OT_THREADS, alias, lds], I32), src), I32, 1 + n)
    want = np.concatenate([[0], np.cumsum(src.astype(np.int64))])
    _assert_same_bits(out, np.concatenate([want[-1:], want[:-1]]).astype(I32), "block_excl_scan n=%d alias=%d lds=%d (total, then dst)" % (n, alias, lds))


@pytest.mark.gpu
@pytest.mark.parametrize("op,name,out", [(OP_DSQRT, "double sqrt", F64), (OP_DDIV, "double division", F64), (OP_FDIV, "__fdiv_rn", F32), (OP_SQRT_RN, "sqrt_rn", F32),
                                         (OP_D2F, "double to float", F32), (OP_D2I, "(int) of a double", I32)])
def test_gpu_ieee_primitives_equal_numpy_on_the_cpu(op, name, out):
    args = ieee_cases(op)
    got = _run(op, len(args[0]), args, out, len(args[0]))
    _assert_same_bits(_one_nan(got), _one_nan(ieee_reference(op, args)), name, args)


@pytest.mark.gpu
def test_gpu_3x3_steps_equal_the_model_and_the_float64_restatements():
    c = mat3_cases()
    got, want = _run(OP_MAT3, len(c), (c,), MAT3_OUT, len(c)), mat3_reference(c)
    bad = []
    for k in MAT3_OUT.names:
        try:
            if k == "stored":
                _assert_same_bits(got[k], want[k], "3 x 3 one_nan (raw)")
            elif k != "pad":
                _assert_same_bits(_one_nan(got[k]), _one_nan(want[k]), "3 x 3 " + k)
        except AssertionError as e:
            bad.append(str(e))
    assert not bad, "\n".join(bad)


def _jacobi_wave(op, n, m, rows):
    """The m x n cases through jacobi_wave<n, rows>.  The model runs on the same `rows` rows, the zero rows included: they change no bit
    of a finite matrix (tests/test_cvmat_model.py), but a NaN rotation turns them into NaN (NaN * 0), on the device as in the model."""
    As = jacobi_cases(n, m)
    At = transposed(As)
    got = _run(op, len(At), (At,), jacobi_out(n), len(At))
    with np.errstate(all="ignore"):
        wAt, wVt, wW, _ = M.jacobi(At, n, rows)
        short = M.jacobi(At[:64], n, m)
    for k, w in enumerate((wAt[:, :, :m], wVt, wW)):                    # the known answers are finite: the host form's m rows give the same bits
        _assert_same_bits(w[:9], (short[k][:, :, :m] if k == 0 else short[k])[:9], "the model on %d and on %d rows" % (rows, m))  # (a zero row may turn -0)
    bad = []
    for k, w in (("At", wAt), ("Vt", wVt), ("W", wW)):
        try:
            _assert_same_bits(_one_nan(got[k]), _one_nan(w), "jacobi_wave %d x %d %s" % (m, n, k))
        except AssertionError as e:
            bad.append(str(e))
    assert not bad, "\n".join(bad)


@pytest.mark.gpu
def test_gpu_jacobi_wave_3_4_equals_the_model():
    _jacobi_wave(OP_JACOBI_3_4, 3, 3, 4)


@pytest.mark.gpu
@pytest.mark.parametrize("m", [9, 16])
def test_gpu_jacobi_wave_9_16_equals_the_model(m):
    _jacobi_wave(OP_JACOBI_9_16, 9, m, 16)


@pytest.mark.gpu
def test_gpu_null_vector_4x4_equals_the_model():
    As = jacobi_cases(4, 4)
    At = transposed(As)
    got = _run(OP_NULL4, len(At), (At[:, :, :4],), NULL4_OUT, len(At))
    with np.errstate(all="ignore"):
        _, wVt, wW, _ = M.jacobi(At, 4, 4)
        one = np.stack([M.null_vector(A)[0] for A in As[:16]])
    _assert_same_bits(_one_nan(wVt[:16, 3, :4]), _one_nan(one), "the batched model and M.null_vector")
    bad = []
    for k, w in (("v", wVt[:, 3, :4]), ("Vt", wVt[:, :, :4]), ("W", wW)):
        try:
            _assert_same_bits(_one_nan(got[k]), _one_nan(w), "null_vector 4 x 4 " + k)
        except AssertionError as e:
            bad.append(str(e))
    assert not bad, "\n".join(bad)
