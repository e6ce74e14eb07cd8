"""References for the operand-prep, int32 row transfer and report kernels (prep.hip, the
formatter of report.hip), NumPy and Python integers only — nothing here calls libdmlp.
tests/test_operand_contract_model.py pins them against torch's bfloat16 cast and the CPU
implementations; the GPU contract tests compare kernels with them bit for bit.

  bf16 hi/lo   cf = fp32(c); hi = bf16(cf); lo = bf16(fp32(c - fp64(hi)))   (round to nearest even)
  image        uint16 [tile][rt][kt][hl][lane][8], lane = r + 16 kg: attributes kt 32 + kg 8 + j of
               point tile 64 + rt 16 + r (hl: 0 hi, 1 lo; the fp16 image has no hl axis)
  render       c = x - mu in fp64; |c|^2 = (s0 + s2) + (s1 + s3), s[a & 3] += c c (every step
               rounded), rounded to fp32; hi = fp16(fp32(c)); |c| >= 65504 or not finite: flagged, 0
  report       "Query <qid> checksum: <cs>\\n"
"""
from __future__ import annotations

import math

import numpy as np

BF16_MAX_ABS = 1.0e15      # prep.hip kMaxAbs
FP16_MAX_ABS = 65504.0     # host_prep.cpp kMaxAbs, k_render


# ------------------------------------------------------------------ bf16
def bf16_rne(f32):
    """bf16 bits (uint16) of float32 values, round to nearest even on the uint32 bits.  NaN
    payloads are not modelled (no kernel converts one: NaN is flagged and rendered as 0)."""
    u = np.ascontiguousarray(f32, np.float32).view(np.uint32).astype(np.uint64)
    return ((u + 0x7fff + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def bf16_trunc(f32):
    """The wrong conversion (for the model tests): the low 16 bits dropped."""
    return (np.ascontiguousarray(f32, np.float32).view(np.uint32) >> 16).astype(np.uint16)


def bf16_to_f64(bits):
    return (np.asarray(bits, np.uint16).astype(np.uint32) << 16).view(np.float32).astype(np.float64)


def split_bf16(c):
    """(hi, lo) uint16 of float64 c (|c| < 1e15)."""
    c = np.asarray(c, np.float64)
    hi = bf16_rne(c.astype(np.float32))
    lo = bf16_rne((c - bf16_to_f64(hi)).astype(np.float32))
    return hi, lo


def centred(X, mu, lim):
    """(c, bad): c = X - mu with every element that is not |c| < lim (too large, inf, NaN) set to
    +0.0, bad = 1 if there was one."""
    with np.errstate(invalid="ignore", over="ignore"):
        c = np.asarray(X, np.float64) - np.asarray(mu, np.float64)
        flag = ~(np.abs(c) < lim)
    c = np.where(flag, 0.0, c)
    return c, int(flag.any())


def _padded(c, rows, W):
    out = np.zeros((rows, W), np.float64)
    out[:c.shape[0], :c.shape[1]] = c
    return out


def hilo_image(X, mu, KT):
    """dmlp_prep_data: (image uint16 [n_tiles * 64 * KT * 64], c [N, A] as the kernel centres it,
    bad)."""
    N, A = X.shape
    nt = (N + 63) // 64
    c, bad = centred(X, mu, BF16_MAX_ABS)
    hi, lo = split_bf16(_padded(c, nt * 64, KT * 32))
    h = np.stack([hi, lo]).reshape(2, nt, 4, 16, KT, 4, 8)        # hl, t, rt, r, kt, kg, j
    return np.ascontiguousarray(h.transpose(1, 2, 4, 0, 5, 3, 6)).reshape(-1), c, bad


def query_frags(Qx, mu, KT):
    """dmlp_prep_queries: (qhi, qlo uint16 [Q, KT * 32], c, bad)."""
    Q, A = Qx.shape
    c, bad = centred(Qx, mu, BF16_MAX_ABS)
    hi, lo = split_bf16(_padded(c, Q, KT * 32))
    return hi, lo, c, bad


def norms_exact(c):
    """|c|^2 of every row: the correctly rounded (math.fsum) sum of the fp64 products."""
    return np.array([math.fsum((r * r).tolist()) for r in np.asarray(c, np.float64)], np.float64)


def within_one_ulp32(got, want64):
    """got (float32) is fp32(want64) or one of its two fp32 neighbours."""
    w = np.asarray(want64, np.float64).astype(np.float32)
    got = np.asarray(got, np.float32)
    lo, hi = np.nextafter(w, np.float32(-np.inf)), np.nextafter(w, np.float32(np.inf))
    return (got == w) | (got == lo) | (got == hi)


# ------------------------------------------------------------------ fp16 image and its copy
def hi_image(rows16, KT):
    """rows [n_tiles * 64, KT * 32] (any 2-byte dtype) -> the hi-only tile image, flat:
    chunk (16 bytes) of point p, attributes kt 32 + kg 8 .. + 7 at chunk index
    ((t 4 + rt) KT + kt) 64 + kg 16 + r  (host_prep.cpp prep_data_range)."""
    n, W = rows16.shape
    assert n % 64 == 0 and W == KT * 32
    h = rows16.reshape(n // 64, 4, 16, KT, 4, 8)                   # t, rt, r, kt, kg, j
    return np.ascontiguousarray(h.transpose(0, 1, 3, 4, 2, 5)).reshape(-1)


def rowmajor(chunks, KT):
    """chunks [n_tiles * 64 * 4 KT, ...] of the tile image -> point-major [p * 4 KT + f]
    (prep.hip k_x1_rowmajor: chunk f of point p sits at tile 256 KT + ((p & 63) >> 4) KT 64 +
    (f >> 2) 64 + 16 (f & 3) + (p & 15))."""
    nf = 4 * KT
    n = chunks.shape[0]
    assert n % (64 * nf) == 0
    i = np.arange(n)
    p, f = i // nf, i % nf
    idx = (p >> 6) * (nf * 64) + ((((p & 63) >> 4) * KT + (f >> 2)) * 64) + 16 * (f & 3) + (p & 15)
    return chunks[idx]


# ------------------------------------------------------------------ k_render / host_prep.cpp
def f16_bits(c):
    with np.errstate(over="ignore"):
        return np.asarray(c, np.float64).astype(np.float32).astype(np.float16).view(np.uint16)


def norm4(c, single=False):
    """fp32 |c|^2 of every row as k_render sums it (single: one accumulator, a wrong order)."""
    c = np.asarray(c, np.float64)
    s = np.zeros((c.shape[0], 4), np.float64)
    for a in range(c.shape[1]):
        j = 0 if single else a & 3
        s[:, j] = s[:, j] + c[:, a] * c[:, a]
    return ((s[:, 0] + s[:, 2]) + (s[:, 1] + s[:, 3])).astype(np.float32)


def i32_rows(m):
    """the fp64 rows of lossless int32 rows: the correctly rounded m / 1e6"""
    return np.asarray(m, np.int32).astype(np.float64) / 1.0e6


def render_model(rows, mu, KT, mode, n_pad=None, single=False):
    """rows [nvalid, A] fp64 (of int32 rows: i32_rows(m)) -> dict
      mode 0: img (uint16 tile image of n_pad rows, n_pad a multiple of 64 >= nvalid), xq =
              xinit [n_pad] (-inf padding), xrow (uint16 [n_pad, KT 32]), up (fp32 [nvalid], the
              rounded-up norms whose max goes to *nmax), bad
      mode 1: img = qhi (uint16 [nvalid, KT 32]), xq = qn, bad."""
    n, A = rows.shape
    W = KT * 32
    c, bad = centred(rows, mu, FP16_MAX_ABS)
    ssf = norm4(c, single)
    if mode == 1:
        return {"img": f16_bits(_padded(c, n, W)), "xq": ssf, "bad": bad}
    n_pad = (n + 63) // 64 * 64 if n_pad is None else n_pad
    h = f16_bits(_padded(c, n_pad, W))
    xq = np.full(n_pad, -np.inf, np.float32)
    xq[:n] = np.float32(-0.5) * ssf
    one = np.float32(1.0) + np.float32(1.0e-6)
    up = ssf * one + np.float32(1.0e-30)
    assert up.dtype == np.float32
    return {"img": hi_image(h, KT), "xq": xq, "xrow": h, "up": up, "bad": bad}


def nmax_bits(up):
    return int(np.asarray(up, np.float32).max().view(np.uint32)) if len(up) else 0


# ------------------------------------------------------------------ report
def report_lines(cs, qid_base=0):
    return [b"Query %d checksum: %d\n" % (qid_base + i, int(c)) for i, c in enumerate(cs)]


def report_ref(cs, qid_base=0) -> bytes:
    return b"".join(report_lines(cs, qid_base))


def line_offsets_ref(cs, qid_base=0, base=0):
    """int64 [nq + 1]: the byte offset of every line and the end of the text"""
    ln = np.array([len(b) for b in report_lines(cs, qid_base)], np.int64)
    return base + np.concatenate([[0], np.cumsum(ln)]).astype(np.int64)


# ------------------------------------------------------------------ adversarial values
def bf16_edges():
    """Centred values where a bf16 hi/lo split goes wrong: ties of hi at the bf16 LSB (to even
    both ways), ties of lo, a tie of lo decided by bits below fp32(c), hi rounding up into the
    next binade, fp32-subnormal residuals and values, -0.0, |c| just under 1e15."""
    v = []
    for e in (0, -3, 20):
        for k in range(8):
            v += [math.ldexp(1.0 + (2 * k + 1) * 2.0 ** -8, e),             # hi ties
                  -math.ldexp(1.0 + (2 * k + 1) * 2.0 ** -8, e),
                  math.ldexp(1.0 + 2.0 ** -10 * (1.0 + (2 * k + 1) * 2.0 ** -8), e)]   # lo ties
    v += [1.0 + 2.0 ** -10 + 2.0 ** -18 + 2.0 ** -40,      # lo tie broken below fp32(c)
          1.0 + 2.0 ** -10 + 2.0 ** -18 - 2.0 ** -40,
          -(1.0 + 2.0 ** -10 + 3 * 2.0 ** -18 + 2.0 ** -45),
          2.0 - 2.0 ** -9, 2.0 - 2.0 ** -20, -(4.0 - 2.0 ** -8), 1024.0 - 2.0 ** -30,   # next binade
          2.0 ** -120 * (1 + 2.0 ** -10), 2.0 ** -125 * (1 + 3 * 2.0 ** -12),  # subnormal residual
          -2.0 ** -122 * (1 + 2.0 ** -9 + 2.0 ** -11),
          2.0 ** -130, 1.5 * 2.0 ** -140, 2.0 ** -149, 2.0 ** -150, 3 * 2.0 ** -151,
          2.0 ** -134, 3 * 2.0 ** -134, -2.0 ** -133, 2.0 ** -126, 2.0 ** -126 * (1 - 2.0 ** -9),
          -0.0, 0.0,
          float(np.nextafter(1.0e15, 0.0)), -float(np.nextafter(1.0e15, 0.0)), 9.99e14, -9.99e14]
    return np.array(v, np.float64)


BF16_FLAGS = (1.0e15, -1.0e15, math.inf, -math.inf, math.nan)


def fp16_edges():
    """The set of tests/test_host_prep.py test_cpu_prep_fp16_rounding_edges (ties at the mantissa
    LSB, fp16 subnormals and their ties, signed zeros) and the ends of the fp16 range."""
    rng = np.random.default_rng(1)
    return np.concatenate([
        rng.uniform(-65000, 65000, 300),
        rng.uniform(-1e-4, 1e-4, 300),
        (np.arange(-200, 200) + 0.5) * 2.0 ** -10,
        (np.arange(1947, 2047) + 0.5) * 2.0 ** 5,                     # ties in the top binade
        np.ldexp(rng.integers(1, 2 ** 12, 300).astype(np.float64), -24),
        [0.0, -0.0, 65503.0, -65503.0, 2.0 ** -14, 2.0 ** -25, 3 * 2.0 ** -26, 2.0 ** -24,
         65503.99, -65503.99, 65488.0, 65472.0 + 16.0 - 2.0 ** -20]])


FP16_FLAGS = (65504.0, -65504.0, 1.0e6, math.inf, math.nan)


def order_row(A):
    """Centred values whose fp32 |c|^2 depends on the order of the fp64 sum: c0^2 + c4^2 =
    1 + 2^-24 sits on an fp32 tie, every other term is 2^-54, a quarter of the accumulator's last
    bit.  Four partial sums collect them (the result rounds up to 1 + 2^-23); one accumulator
    drops each of them (the tie rounds to 1.0)."""
    c = np.full(A, 2.0 ** -27)
    c[0] = 1.0
    if A > 4:
        c[4] = 2.0 ** -12
    return c


def render_rows(n, A, seed=0, i32=False):
    """(rows fp64 [n, A], mu, int32 rows or None) for the fp16 render: the fp16 edge set and, A > 4,
    order_row in rows 1 and n - 2 (mu 0 or 0.5, so that those rows centre exactly); or int32 rows drawn
    over the whole int32 range and a six-decimal mu in [-1000, 1000)."""
    rng = np.random.default_rng(seed + A)
    if i32:
        m = i32_values(n * A, seed + A).reshape(n, A)
        return i32_rows(m), np.round(rng.uniform(-1000.0, 1000.0, A), 6), m
    e = fp16_edges()
    mu = np.where(np.arange(A) % 2 == 0, 0.0, 0.5)
    i, a = np.meshgrid(np.arange(n), np.arange(A), indexing="ij")
    X = e[(i * A + a + seed) % len(e)] + mu[None, :]
    if A > 4 and n > 2:
        X[1] = X[n - 2] = order_row(A) + mu
    return np.ascontiguousarray(X), mu, None

I32_EDGES = np.array([0, 1, -1, 999999, -999999, 1000000, -1000000, 2147483647, -2147483647,
                      -2147483648], np.int64).astype(np.int32)


def i32_values(n, seed=0):
    """I32_EDGES, then values drawn over the whole int32 range"""
    rng = np.random.default_rng(seed)
    r = rng.integers(-(1 << 31), 1 << 31, max(0, n - len(I32_EDGES)), dtype=np.int64)
    return np.concatenate([I32_EDGES, r.astype(np.int32)])[:n]


def checksum_values(seed=0, n_random=64):
    """uint64: for every digit count d the ends 10^(d-1) and 10^d - 1, the group boundaries of a
    9-digit splitter, values whose middle (or low) nine-digit group is all zeros, random."""
    v = [0, 10 ** 9, 10 ** 9 + 1, 10 ** 9 - 1, 10 ** 18, 10 ** 18 - 1, 10 ** 18 + 1, 2 ** 64 - 1,
         2 ** 63, 2 ** 32]
    for d in range(1, 21):
        v += [10 ** (d - 1), min(10 ** d - 1, 2 ** 64 - 1)]
    v += [7 * 10 ** 18 + 5, 12 * 10 ** 18 + 123456789, 18 * 10 ** 18 + 10 ** 9 * 0 + 1,
          3 * 10 ** 18 + 100000000, 5 * 10 ** 9, 5 * 10 ** 9 + 7, 123 * 10 ** 9 + 10,
          10 ** 19, 10 ** 19 + 10 ** 9, 4 * 10 ** 18 + 999999999 * 10 ** 9]
    rng = np.random.default_rng(seed)
    v += [int(x) for x in rng.integers(0, 1 << 63, n_random, dtype=np.int64)]
    v += [int(x) + (1 << 63) for x in rng.integers(0, 1 << 63, n_random, dtype=np.int64)]
    assert all(0 <= x < 1 << 64 for x in v)
    return np.array(v, np.uint64)


def checksums(nq, seed=0):
    """nq checksums cycling through checksum_values in a shuffled order"""
    base = checksum_values(seed)
    rng = np.random.default_rng(seed + nq)
    reps = (nq + len(base) - 1) // len(base)
    out = np.concatenate([base[rng.permutation(len(base))] for _ in range(reps)])
    return np.ascontiguousarray(out[:nq])


def prep_rows(n, A, mu, seed=0):
    """n rows for the bf16 prep: row i % 4 == 0 uniform six-decimal values in [0, 1000), the
    others mu + a bf16 edge value (exactly that centred value where mu[a] = 0)."""
    rng = np.random.default_rng(seed * 1000 + n * 31 + A)
    X = np.round(rng.uniform(0.0, 1000.0, (n, A)), 6)
    e = bf16_edges()
    i, a = np.meshgrid(np.arange(n), np.arange(A), indexing="ij")
    ev = e[(i * 37 + a * 11 + seed) % len(e)] + np.asarray(mu)[None, :]
    X = np.where((i % 4) != 0, ev, X)
    return np.ascontiguousarray(X)


def prep_mu(A):
    """A centre with exact zeros (columns 0, A - 1 and every third) and six-decimal values"""
    mu = np.round(np.random.default_rng(A).uniform(400.0, 600.0, A), 6)
    mu[::3] = 0.0
    mu[A - 1] = 0.0
    return mu
