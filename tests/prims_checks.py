"""Checks of the gfx950 primitives the subgraph and dense-layer kernels are written against (igmc_amd/csrc/g2_prims.h,
g2_image.h), one at a time through ``igmc_debug_g2_prims`` (g2_probe.h) -- shared by tests/test_emu_prims.py (the CPU stand-ins)
and tests/test_gpu_prims.py (the device forms on an MI355X).

Each primitive has two forms, and a whole model step sees them through four layers, a head and a backward pass at one weight
scale and at tolerances relative to a tensor's peak; here every one is held to a restatement of its own:

* ``g2_pk_bf16`` / ``g2_split2``: a round-to-nearest-even conversion restated on the bit patterns -- bit equality of the three
  packed words, and ``hi + mid + lo == x`` EXACTLY in float64, for ``2^-100 <= |x| < 2^127`` (below, a residual is an f32
  subnormal; above, a term may overflow);
* ``g2_expand4`` / ``g2_bytemask`` / ``g2_mask_frag``: a per-byte restatement, bit equality (on both backends: each stand-in is
  thereby equal to its device form);
* ``g2_mfma_bf16``: the float64 sum of the exact products plus c -- exact where every order of summation is exact in f32, and
  within the first-order bound of any order of 33 f32 additions otherwise;
* ``g2_tanh`` and the two instructions its device form is made of: float64.

What is recorded but not asserted (f32 subnormals, the convert instruction above the overflow threshold, bf16 subnormal
operands of the matrix core) goes to the parity log (``parity_checks.record_observed``); profiles/prims_observed.txt keeps what
both backends showed."""
import ctypes

import numpy as np

import parity_checks as PC

SPLIT, TANH, EXP, RCP, MFMA, MASK = range(6)
IN_WORDS = {SPLIT: 2, TANH: 1, EXP: 1, RCP: 1, MFMA: 12, MASK: 4}
OUT_WORDS = {SPLIT: 3, TANH: 1, EXP: 1, RCP: 1, MFMA: 4, MASK: 8}
PAD, SENTINEL = 64, 0xC0DEC0DE          # words behind the results that no lane may write
U = 2.0 ** -24                          # unit roundoff of float32
RELM_CODE, KEEP_BITS = 0x0F, (4, 5)     # common.h: IGMC_RELM_CODE, IGMC_RELM_KF / IGMC_RELM_KT


def probe(be, op, words, n):
    """``igmc_debug_g2_prims(op)`` over n items -> the result words [n, OUT_WORDS[op]] (uint32)."""
    words = np.ascontiguousarray(words, np.uint32).reshape(-1)
    assert words.size == n * IN_WORDS[op]
    d_in = be.dev(words.view(np.int32))
    d_out = be.dev(np.full(n * OUT_WORDS[op] + PAD, SENTINEL, np.uint32).view(np.int32))
    be.lib.call('igmc_debug_g2_prims', ctypes.c_int(op), ctypes.c_void_p(be.ptr(d_in)), ctypes.c_int64(n),
                ctypes.c_void_p(be.ptr(d_out)), None)
    be.sync()
    out = be.host(d_out).view(np.uint32)
    assert (out[n * OUT_WORDS[op]:] == SENTINEL).all(), 'a word behind the results was written'
    return out[:n * OUT_WORDS[op]].reshape(n, OUT_WORDS[op])


def f32(bits):
    return np.ascontiguousarray(bits, np.uint32).view(np.float32)


def bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def probe_f32(be, op, x):
    x = np.ascontiguousarray(x, np.float32).reshape(-1)
    return f32(probe(be, op, bits(x), x.size).reshape(-1))


def check_refusals(be):
    """Null pointers, a negative size, unknown ops and part of a wave for the matrix core are refused."""
    buf = be.dev(np.zeros(64 * 12, np.int32))
    p = ctypes.c_void_p(be.ptr(buf))
    call = lambda op, i, n, o: be.lib.cdll.igmc_debug_g2_prims(ctypes.c_int(op), i, ctypes.c_int64(n), o, None)
    assert call(TANH, None, 4, p) != 0 and call(TANH, p, 4, None) != 0
    assert call(TANH, p, -1, p) != 0
    assert call(-1, p, 4, p) != 0 and call(6, p, 4, p) != 0
    assert call(MFMA, p, 63, p) != 0
    assert call(TANH, p, 0, p) == 0
    be.sync()


# ====================================================================== bf16 conversion and the three-term split
def bf16_rne(u):
    """Round-to-nearest-even f32 -> bf16 on the bit patterns of finite values (a carry out of the mantissa moves the exponent)."""
    u = np.asarray(u, np.uint32).astype(np.uint64)
    return (((u + np.uint64(0x7FFF) + ((u >> np.uint64(16)) & np.uint64(1))) >> np.uint64(16)) & np.uint64(0xFFFF)).astype(np.uint32)


def bf16_f32(h):
    return f32(np.asarray(h, np.uint32) << np.uint32(16))


def split_terms(u):
    """The three bf16 terms (16-bit patterns) of the f32 values with bit patterns ``u``: each residual is exact in f32."""
    x = f32(u)
    with np.errstate(all='ignore'):
        h = bf16_rne(u)
        r = x - bf16_f32(h)
        m = bf16_rne(bits(r))
        s = r - bf16_f32(m)
        lo = bf16_rne(bits(s))
    return h, m, lo


def split_inputs():
    rng = np.random.default_rng(101)
    hi16 = np.arange(1 << 16, dtype=np.uint32) << np.uint32(16)
    exps = np.arange(1, 255, dtype=np.uint32) << np.uint32(23)
    sign = np.uint32(0x80000000)
    parts = [
        rng.integers(0, 1 << 32, 200000, dtype=np.uint64).astype(np.uint32),          # random bit patterns
        hi16 | np.uint32(0x8000),                                                     # every tie, both parities of bit 16
        hi16 | np.uint32(0x7FFF), hi16 | np.uint32(0x8001),                           # ... and their neighbours
        np.array([0, 0x80000000, 0x7F7F0000, 0x7F7EFFFF, 0x7F7F0001, 0xFF7F0000, 0xFF7EFFFF, 0xFF7F0001,
                  0x7F7F7FFF, 0x7F7F8000, 0x7F7FFFFF, 0x7F800000, 0xFF800000, 0x7FC00000, 0xFFC00001, 0x7F800001], np.uint32),
        exps, exps | sign,                                                            # powers of two
        exps | np.uint32(0x7F8000), exps | np.uint32(0x7FFFFF), exps | np.uint32(0x7FC123),      # round up into the next binade
        exps | sign | np.uint32(0x7F8000), exps | sign | np.uint32(0x7FFFFF),
        exps | np.uint32(0x007FFF), exps | np.uint32(0x00FF80), exps | np.uint32(0x00807F),      # second term rounds up / ties
        rng.integers(1, 1 << 23, 4096, dtype=np.uint64).astype(np.uint32),            # f32 subnormals
        rng.integers(1, 1 << 23, 4096, dtype=np.uint64).astype(np.uint32) | sign,
    ]
    u = np.concatenate(parts)
    if u.size % 2:
        u = np.append(u, np.uint32(0x3F800000))
    u = u[rng.permutation(u.size)]            # the two values of a pair have nothing to do with each other
    return u


def check_split(be):
    """``g2_split2`` against the bit-level restatement; -> what was observed outside the asserted range."""
    u = split_inputs()
    n = u.size // 2
    got = probe(be, SPLIT, u, n)              # words {term(x) | term(y) << 16}
    t = np.empty((3, u.size), np.uint32)
    t[:, 0::2] = (got & np.uint32(0xFFFF)).T
    t[:, 1::2] = (got >> np.uint32(16)).T
    want = np.stack(split_terms(u))
    with np.errstate(invalid='ignore'):
        xd = f32(u).astype(np.float64)
    ax = np.abs(xd)
    finite = (u & np.uint32(0x7F800000)) != np.uint32(0x7F800000)
    held = finite & (ax >= 2.0 ** -100) & (ax < 2.0 ** 127)
    assert held.sum() > 300000
    assert (u[held] & np.uint32(0xFFFF) == 0x8000).sum() > 50000 and (ax[held] == 2.0 ** 126).any()
    bad = held & (t != want).any(0)
    assert not bad.any(), '%d of %d values: terms differ from round-to-nearest-even (first x = 0x%08X: got %s want %s)' % (
        int(bad.sum()), int(held.sum()), int(u[bad][0]), ['0x%04X' % v for v in t[:, bad][:, 0]], ['0x%04X' % v for v in want[:, bad][:, 0]])
    with np.errstate(invalid='ignore'):
        total = bf16_f32(t[0]).astype(np.float64) + bf16_f32(t[1]).astype(np.float64) + bf16_f32(t[2]).astype(np.float64)
    inexact = held & (total != xd)
    assert not inexact.any(), '%d values: hi + mid + lo != x (first x = 0x%08X)' % (int(inexact.sum()), int(u[inexact][0]))
    # outside the range: no finite input below the overflow threshold of the conversion yields a non-finite term
    below_overflow = finite & ((u & np.uint32(0x7FFFFFFF)) < np.uint32(0x7F7F8000))
    nonfinite_term = ((t & np.uint32(0x7F80)) == np.uint32(0x7F80)).any(0)
    assert not (below_overflow & nonfinite_term).any(), 'a finite input below the overflow threshold gave a non-finite term: 0x%08X' % int(
        u[below_overflow & nonfinite_term][0])
    differs = (t != want).any(0)
    classes = {'f32_subnormal': finite & (ax > 0) & (ax < 2.0 ** -126), 'tiny_normal': finite & (ax >= 2.0 ** -126) & (ax < 2.0 ** -100),
               'from_2p127': finite & (ax >= 2.0 ** 127) & below_overflow, 'overflow': finite & ~below_overflow,
               'inf': ~finite & ((u & np.uint32(0x7FFFFF)) == 0), 'nan': ~finite & ((u & np.uint32(0x7FFFFF)) != 0)}
    seen = {}
    for k, sel in classes.items():
        assert sel.any(), k
        seen[k + '_n'] = int(sel.sum())
        seen[k + '_differ_from_rne'] = int((sel & differs).sum())
        seen[k + '_nonfinite_terms'] = int((sel & nonfinite_term).sum())
        seen[k + '_inexact'] = int((sel & finite & (total != xd)).sum())
    PC.record_observed('prims_split', backend=be.name, held=int(held.sum()), **seen)
    print('split (%s): %d values bit-equal and exact; outside the range: %s' % (be.name, int(held.sum()), seen))
    return seen


# ====================================================================== byte masks
def mask_inputs():
    rows = []
    rng = np.random.default_rng(102)
    extra = rng.integers(0, 1 << 32, 64, dtype=np.uint64).astype(np.uint32)
    for flags in (0, 1):
        for kb in KEEP_BITS:
            for r1 in (1, 2, 3, 4, 5, 9):                    # 9: a relation code the block never holds
                for pos in range(4):
                    v = np.arange(256, dtype=np.uint32)
                    w = np.zeros(256, np.uint32)
                    for q in range(4):                       # the other positions cycle through different bytes
                        byte = v if q == pos else (v * np.uint32(7 + 2 * q) + np.uint32(13 * q + 5 * pos + 3 * r1 + kb)) & np.uint32(0xFF)
                        w |= byte << np.uint32(8 * q)
                    rows.append(np.stack([w, np.full(256, r1, np.uint32), np.full(256, kb, np.uint32), np.full(256, flags, np.uint32)], 1))
                rows.append(np.stack([extra, np.full(64, r1, np.uint32), np.full(64, kb, np.uint32), np.full(64, flags, np.uint32)], 1))
    return np.concatenate(rows)


def byte_matches(byte, r1, keepbit, flags):
    """One block byte (common.h: bits 0..3 = relation + 1, bits 4 / 5 = keep flags) against relation code r1."""
    code = byte & RELM_CODE
    if flags and not (byte >> keepbit) & 1:
        code = 0
    return code == r1


def mask_expected(w, r1, kb, flags):
    m = [byte_matches((w >> (8 * q)) & 0xFF, r1, kb, flags) for q in range(4)]
    rot = ((w >> 8) | (w << 24)) & 0xFFFFFFFF
    m1 = [byte_matches((rot >> (8 * q)) & 0xFF, r1, kb, flags) for q in range(4)]
    pair = lambda a, b: (0x3F80 if a else 0) | (0x3F800000 if b else 0)          # bf16 1.0 where the byte matches
    bm = lambda mm: sum(0xFF << (8 * q) for q in range(4) if mm[q])
    return [pair(m[0], m[1]), pair(m[2], m[3]), bm(m), bm(m1), pair(m[0], m[1]), pair(m[2], m[3]), pair(m1[0], m1[1]), pair(m1[2], m1[3])]


def check_masks(be):
    inp = mask_inputs()
    got = probe(be, MASK, inp, len(inp))
    want = np.array([mask_expected(int(w), int(r1), int(kb), int(fl)) for w, r1, kb, fl in inp], np.uint32)
    assert (want[:, 2] == 0).any() and all((want[:, 2] >> (8 * q) & 0xFF == 0xFF).any() for q in range(4))
    for flags in (0, 1):                      # the flags do change what is kept, and the two keep bits differ
        sel = inp[:, 3] == flags
        assert (want[sel, 2] != 0).any()
    k4, k5 = (inp[:, 3] == 1) & (inp[:, 2] == 4), (inp[:, 3] == 1) & (inp[:, 2] == 5)
    assert not np.array_equal(want[k4, 2], want[k5, 2])
    bad = (got != want).any(1)
    names = ('expand4.o01', 'expand4.o23', 'bytemask', 'bytemask(rotated)', 'frag[0]', 'frag[1]', 'frag[2]', 'frag[3]')
    if bad.any():
        i = int(np.flatnonzero(bad)[0])
        col = int(np.flatnonzero(got[i] != want[i])[0])
        raise AssertionError('%d of %d mask cases differ; first: word 0x%08X r1 %d keep bit %d FLAGS %d: %s = 0x%08X, want 0x%08X' % (
            int(bad.sum()), len(inp), int(inp[i, 0]), int(inp[i, 1]), int(inp[i, 2]), int(inp[i, 3]), names[col], int(got[i, col]),
            int(want[i, col])))
    return len(inp)


# ====================================================================== the matrix-core step
def mfma_reference(a, b, c):
    """a, b [waves, 64 lanes, 8] float64 values of the bf16 operands, c [waves, 64, 4] -> (D, sum |a b| + |c|) as the lanes hold
    them.  Lane (li, kq) of A holds row li, of B column li, both for the same eight k; lane (li, kq) of D holds rows
    4 kq .. 4 kq + 3 of column li."""
    W = a.shape[0]
    A = a.reshape(W, 4, 16, 8).transpose(0, 2, 1, 3).reshape(W, 16, 32)          # [w, row, k]
    B = b.reshape(W, 4, 16, 8).transpose(0, 2, 1, 3).reshape(W, 16, 32)          # [w, col, k]
    P = np.einsum('wik,wjk->wij', A, B)
    S = np.einsum('wik,wjk->wij', np.abs(A), np.abs(B))
    lane = np.arange(64)
    rows = 4 * (lane >> 4)[:, None] + np.arange(4)[None, :]                      # [lane, reg]
    cols = np.broadcast_to((lane & 15)[:, None], (64, 4))
    return P[:, rows, cols] + c, S[:, rows, cols] + np.abs(c)


def to_bf16_bits(x):
    """float values -> bf16 bit patterns (round to nearest even)"""
    return bf16_rne(bits(np.asarray(x, np.float32)))


def pack_mfma(a16, b16, c):
    """bf16 patterns [W, 64, 8] x 2 and f32 c [W, 64, 4] -> the probe's 12 words per lane"""
    pk = lambda h: (h[..., 0::2] | (h[..., 1::2] << np.uint32(16))).astype(np.uint32)
    return np.concatenate([pk(a16), pk(b16), bits(c).reshape(c.shape)], -1)


def run_mfma(be, a16, b16, c):
    W = a16.shape[0]
    got = f32(probe(be, MFMA, pack_mfma(a16, b16, c), W * 64).reshape(-1)).reshape(W, 64, 4).astype(np.float64)
    ref, S = mfma_reference(bf16_f32(a16).astype(np.float64), bf16_f32(b16).astype(np.float64), c.astype(np.float64))
    return got, ref, S


def check_mfma_exact(be):
    """Sums that are representable in f32 whatever the order of the 33 additions must come out exact."""
    rng = np.random.default_rng(103)
    W = 16
    # (1) A in {0, 1}, B and c small integers
    a = (rng.random((W, 64, 8)) < 0.5).astype(np.float32)
    b = rng.integers(-8, 9, (W, 64, 8)).astype(np.float32)
    c = rng.integers(-64, 65, (W, 64, 4)).astype(np.float32)
    got, ref, _ = run_mfma(be, to_bf16_bits(a), to_bf16_bits(b), c)
    assert np.ptp(ref) > 0 and np.array_equal(got, ref), 'A in {0, 1}, small integers: %d of %d sums are not exact' % (
        int((got != ref).sum()), ref.size)
    # (2) A in {0, 1}, B the hi / mid / lo terms of one value per column (terms of one sign: every partial sum is a multiple of
    #     the value's last place and no larger than the value): row i sums the terms of the columns' values at three k of its own
    xs = []
    while len(xs) < W * 16:
        u = rng.integers(0x30000000, 0x50000000, 4096, dtype=np.uint64).astype(np.uint32)
        h, m, lo = split_terms(u)
        keep = ((h | m | lo) & np.uint32(0x8000)) == 0              # all three terms positive (or zero)
        xs.extend(u[keep].tolist())
    xu = np.array(xs[:W * 16], np.uint32).reshape(W, 16)
    h, m, lo = split_terms(xu)
    sgn = np.where(rng.random((W, 16)) < 0.5, np.uint32(0x8000), np.uint32(0)).astype(np.uint32)
    A = np.zeros((W, 16, 32), np.float32)
    B16 = to_bf16_bits(rng.integers(-8, 9, (W, 16, 32)).astype(np.float32))          # arbitrary where A is zero
    ks = [3, 17, 30]                                                 # one k per term, in three different lanes' fragments
    A[:, :, ks] = 1.0
    for q, term in zip(ks, (h, m, lo)):
        B16[:, :, q] = term | (sgn * (term != 0))
    lanes = lambda M: M.reshape(W, 16, 4, 8).transpose(0, 2, 1, 3).reshape(W, 64, 8)       # [w, row / col, k] -> [w, lane, e]
    c0 = np.zeros((W, 64, 4), np.float32)
    got, ref, _ = run_mfma(be, lanes(to_bf16_bits(A)), lanes(B16), c0)
    xv = f32(xu).astype(np.float64) * np.where(sgn != 0, -1.0, 1.0)
    assert np.array_equal(ref, np.broadcast_to(xv[:, None, :], (W, 16, 16)).reshape(W, 4, 4, 16).transpose(0, 1, 3, 2).reshape(W, 64, 4)), \
        'the reference does not reproduce the values from their terms'
    assert np.array_equal(got, ref), 'hi + mid + lo through the matrix core: %d of %d sums differ from x' % (int((got != ref).sum()), ref.size)
    # (3) cancellations M, -M, s with s >= 2^-20 M at three k (every order exact), with and without s in c
    A = np.zeros((W, 16, 32), np.float32)
    B = np.zeros((W, 16, 32), np.float32)
    c = np.zeros((W, 64, 4), np.float32)
    big = 2.0 ** rng.integers(-10, 11, (W, 16)).astype(np.float32)
    small = big * 2.0 ** -rng.integers(1, 21, (W, 16)).astype(np.float32)
    k3 = rng.permuted(np.tile(np.arange(32), (W, 1)), axis=1)[:, :3]
    for w in range(W):
        A[w, :, k3[w]] = 1.0
        B[w, :, k3[w, 0]] = big[w]
        B[w, :, k3[w, 1]] = -big[w]
        if w % 2:
            B[w, :, k3[w, 2]] = small[w]
        else:
            c[w] = np.broadcast_to(small[w][None, :], (16, 16)).reshape(4, 4, 16).transpose(0, 2, 1).reshape(64, 4)
    got, ref, _ = run_mfma(be, lanes(to_bf16_bits(A)), lanes(to_bf16_bits(B)), c)
    assert (ref != 0).all() and np.array_equal(got, ref), 'M - M + s: %d of %d sums are not exact' % (int((got != ref).sum()), ref.size)


def check_mfma_random(be):
    """Random bf16 operands over 16 binades: ``|err| <= 33 * 2^-24 * (sum |a b| + |c|)``, the first-order bound of any order of 33
    float32 additions (the products of bf16 values are exact in float32).  -> the largest err / bound."""
    rng = np.random.default_rng(104)
    W = 128
    scale = lambda shape: 2.0 ** rng.integers(-8, 9, shape)
    a16 = to_bf16_bits(rng.standard_normal((W, 64, 8)) * scale((W, 64, 8)))
    b16 = to_bf16_bits(rng.standard_normal((W, 64, 8)) * scale((W, 64, 8)))
    c = (rng.standard_normal((W, 64, 4)) * scale((W, 64, 4))).astype(np.float32)
    got, ref, S = run_mfma(be, a16, b16, c)
    assert np.isfinite(got).all()
    bound = 33 * U * S
    err = np.abs(got - ref)
    worst = float((err / bound).max())
    print('mfma (%s): largest err / bound %.4f' % (be.name, worst))
    PC.record_observed('prims_mfma', backend=be.name, worst_err_over_bound=worst)
    assert (err <= bound).all(), '%d of %d sums beyond 33 * 2^-24 * (sum|a b| + |c|); largest err / bound %.3f' % (
        int((err > bound).sum()), err.size, worst)
    # bf16 subnormal operands (times 2^100: normal products): recorded, not asserted
    a16 = rng.integers(1, 0x80, (4, 64, 8), dtype=np.uint64).astype(np.uint32) | np.where(rng.random((4, 64, 8)) < 0.5, 0x8000, 0).astype(np.uint32)
    b16 = to_bf16_bits(2.0 ** 100 * rng.standard_normal((4, 64, 8)))
    got, ref, S = run_mfma(be, a16, b16, np.zeros((4, 64, 4), np.float32))
    sub = float((np.abs(got - ref) / (33 * U * S)).max())
    PC.record_observed('prims_mfma_subnormal', backend=be.name, worst_err_over_bound=sub, all_zero=bool(not got.any()))
    print('mfma (%s): bf16 subnormal operands: largest err / bound %.4g, all results zero: %s' % (be.name, sub, not got.any()))
    return worst


# ====================================================================== exp, rcp, tanh
def ulp64(ref):
    """One unit in the last place of float32 at the magnitude of the float64 values ``ref`` (normal range)."""
    _, e = np.frexp(np.abs(ref))
    return np.ldexp(1.0, e - 24)


def check_rcp(be):
    """The reciprocal within 1 ulp of float64 ``1 / x`` over the normal inputs whose reciprocal is normal too (``2^-126 <= |x| <=
    2^126``).  Beyond, ``1 / x`` is an f32 subnormal: the result is either flushed to a zero of the right sign (what the MI355X's
    instruction does) or within one subnormal unit (2^-149) of it (the stand-in's division) -- a change of the denormal mode of
    either form fails here."""
    rng = np.random.default_rng(105)
    u = rng.integers(0, 1 << 32, 300000, dtype=np.uint64).astype(np.uint32)
    x = np.concatenate([f32(u), np.linspace(1.0, 2.0, 65537, dtype=np.float32), -np.linspace(1.0, 4.0, 65537, dtype=np.float32),
                        np.float32(2.0) ** np.arange(-126, 127).astype(np.float32), np.array([3.0, -3.0, 1e-30, 1e30], np.float32)])
    x = x[np.isfinite(x)]
    x = x[np.abs(x.astype(np.float64)) >= 2.0 ** -126]
    got = probe_f32(be, RCP, x).astype(np.float64)
    ref = 1.0 / x.astype(np.float64)
    held = np.abs(x.astype(np.float64)) <= 2.0 ** 126
    assert held.sum() > 300000
    e = np.abs(got - ref) / ulp64(ref)
    i = int(np.argmax(np.where(held, e, 0)))
    worst = float(e[i])
    sub = float(np.abs(got - ref)[~held].max() / 2.0 ** -149) if (~held).any() else 0.0
    print('rcp (%s): largest error %.3f ulp at x = %r; subnormal results: largest error %.4g x 2^-149' % (be.name, worst, float(x[i]), sub))
    PC.record_observed('prims_rcp', backend=be.name, worst_ulp=worst, at=float(x[i]), subnormal_results_worst_in_2p149=sub)
    assert (e[held] <= 1.0).all(), 'reciprocal: %d of %d beyond 1 ulp; largest %.3f ulp at x = %r' % (
        int((e[held] > 1.0).sum()), int(held.sum()), worst, float(x[i]))
    gs, rs = got[~held], ref[~held]
    assert gs.size > 1000
    flushed = (gs == 0) & (np.signbit(gs) == np.signbit(rs))
    ok = flushed | (np.abs(gs - rs) <= 2.0 ** -149)
    assert ok.all(), 'reciprocal of |x| > 2^126: %d of %d neither a signed zero nor within 2^-149 (first x = %r -> %r)' % (
        int((~ok).sum()), gs.size, float(x[~held][~ok][0]), float(gs[~ok][0]))
    return worst


def check_exp(be):
    """The exponential within ``1 ulp + |x| 2^-23`` (relative) of float64 over the arguments whose result is a normal f32: the
    second term covers the argument's scaling by log2 e on the device (the product's rounding and the constant's)."""
    rng = np.random.default_rng(106)
    x = np.concatenate([np.linspace(-87.0, 88.0, 400001, dtype=np.float32), np.linspace(-1.0, 1.0, 65537, dtype=np.float32),
                        (rng.standard_normal(65536) * 8).astype(np.float32), np.array([0.0, -0.0, 24.0, -24.0, 2 * 44.35], np.float32)])
    x = x[(x >= -87.0) & (x <= 88.0)]
    got = probe_f32(be, EXP, x).astype(np.float64)
    xd = x.astype(np.float64)
    ref = np.exp(xd)
    bound = ulp64(ref) + np.abs(xd) * 2.0 ** -23 * ref
    err = np.abs(got - ref)
    i = int(np.argmax(err / bound))
    e_ulp = float((err / ulp64(ref)).max())
    worst = float(err[i] / bound[i])
    print('exp (%s): largest err / bound %.3f at x = %r; largest error in ulp %.3f' % (be.name, worst, float(x[i]), e_ulp))
    PC.record_observed('prims_exp', backend=be.name, worst_err_over_bound=worst, at=float(x[i]), worst_ulp=e_ulp)
    assert (err <= bound).all(), 'exponential: %d of %d beyond 1 ulp + |x| 2^-23; largest err / bound %.3f at x = %r' % (
        int((err > bound).sum()), x.size, worst, float(x[i]))
    return worst


TANH_ABS = 8 * U


def tanh_inputs():
    lg = np.logspace(-12, 0, 20001).astype(np.float32)
    ov = np.linspace(44.3, 44.4, 4097, dtype=np.float32)
    big = np.array([10.0, 10.5, 12.5, 20.0, 40.0, 88.0, 1e30, 3e38], np.float32)
    return np.concatenate([np.linspace(-12.0, 12.0, 2000001, dtype=np.float32), lg, -lg, ov, -ov, big, -big,
                           np.array([0.0, -0.0, np.inf, -np.inf, 1e-38, -1e-38, 1e-45, -1e-45], np.float32)])


def check_tanh(be):
    """``g2_tanh`` against float64 ``tanh``.

    The device form is ``1 - 2 rcp(1 + exp(2x))`` in float32 (the emulation build calls ``tanhf``).  Asserted: ``g2_tanh(+-0) == 0``
    exactly; ``|result| <= 1`` for every finite and infinite input; exactly ``+-1`` for ``|x| >= 10`` and ``+-inf``; NaN in, NaN out; and
    ``|g2_tanh(x) - tanh(x)| <= 8 * 2^-24`` over 2 M evenly spaced points of [-12, 12], 1e-12 .. 1 logarithmically in both signs,
    +-44.3 .. +-44.4 (where ``exp(2x)`` overflows), +-88 and +-1e30.

    The bound: with t = tanh x, e = exp(2x), r = 1 / (1 + e) = (1 - t) / 2.  Evaluated in float32 with correctly rounded
    operations the formula is within 3.0 * 2^-24 of tanh (worst near x = -3.55, measured on a CPU: the final subtraction rounds
    at 2^-24 for results in [1/2, 1), 2 r at 2^-24 relative, 1 + e likewise).  One ulp of error in exp is a relative error of
    2^-23 in e and moves the result by 2 r^2 e 2^-23 = (1 - t^2) / 2 * 2^-23 <= 1.0 * 2^-24; the scaling of the argument adds
    (1 - t^2) |x| 2^-23 at most 0.45 * 2^-23 < 1.0 * 2^-24 (x (1 - tanh^2 x) peaks at 0.448, and vanishes as e^-2|x|); one ulp of
    error in rcp is 2^-23 relative in r and moves the result by 2 r 2^-23 <= 2.0 * 2^-24.  3 + 1 + 1 + 2 = 7 < 8.  The bound is
    absolute: below |x| ~ 1e-6 the result is a multiple of 2^-24 and its RELATIVE error exceeds 1 (below 3e-8 it is 0)."""
    x = tanh_inputs()
    got = probe_f32(be, TANH, x)
    assert not np.isnan(got).any(), 'NaN for a finite or infinite argument'
    zero = x == 0
    assert zero.sum() >= 2 and np.signbit(x[zero]).any() and (got[zero] == 0).all(), 'g2_tanh(+-0) is not exactly 0: %s' % got[zero]
    assert (np.abs(got) <= 1.0).all(), '|g2_tanh| exceeds 1: %r at x = %r' % (
        float(got[np.argmax(np.abs(got))]), float(x[np.argmax(np.abs(got))]))
    sat = np.abs(x) >= 10.0
    assert sat.sum() > 100000 and np.isinf(x).sum() == 2
    assert np.array_equal(got[sat], np.sign(x[sat])), 'not exactly +-1 for |x| >= 10: first x = %r -> %r' % (
        float(x[sat][got[sat] != np.sign(x[sat])][0]), float(got[sat][got[sat] != np.sign(x[sat])][0]))
    nan = probe_f32(be, TANH, np.array([np.nan, -np.nan, f32(np.array([0x7F800001], np.uint32))[0]], np.float32))
    assert np.isnan(nan).all(), 'NaN in, %s out' % nan
    ref = np.tanh(x.astype(np.float64))
    err = np.abs(got.astype(np.float64) - ref)
    i = int(np.argmax(err))
    worst = float(err[i] / U)
    small = (np.abs(x) > 0) & (np.abs(x) < 1e-6)
    rel_small = float((err[small] / np.abs(ref[small])).max())
    print('tanh (%s): largest |error| %.3f x 2^-24 at x = %r; largest relative error below 1e-6: %.3g' % (be.name, worst, float(x[i]), rel_small))
    PC.record_observed('prims_tanh', backend=be.name, worst_abs_in_2p24=worst, at=float(x[i]), worst_rel_below_1e6=rel_small)
    assert (err <= TANH_ABS).all(), '%d of %d beyond 8 * 2^-24; largest %.3f x 2^-24 at x = %r' % (
        int((err > TANH_ABS).sum()), x.size, worst, float(x[i]))
    return worst
