"""BLS12-381 field layer on the device: gm_test_field_op for Fr, Fp and Fp2 against
Python integers, and the raw-limb hook gm_test_field_raw_op at the named maxima of
the headroom audit -- Fr has the least lazy-reduction headroom in the library
(R' / r = 2^261 / r ~ 70.66), and Fp2 = Fp[u]/(u^2 + 1) at 14 limbs is a template
pair (non-residue -1, N = 14) no other curve runs.  tests/lazy_model.py unchanged."""
import random

import pytest

import lazy_model as lm
import bls12381_params as bp

pytestmark = pytest.mark.gpu

FR, FP = 0, 1
MUL_LZ, SQR_LZ, MUL, MUL2, MUL2_NEGK, ADD_LZ, SUB_LZ, SUB2X_LZ, SUB_CF_MUL, CNEG_SUB, PMINUS, REDUCE_K, CANON, \
    TO2P, IS_ZERO, TIMES5, FE2_MUL, FE2_SQR, PF2_MUL, PF2_SQR, PF2_MUL_SUB, MUL4_REDC = range(22)


class Field381(lm.Field):
    """lm.Field for curve id 2 (lm.Field itself looks its curve up in pyref.CURVES)."""

    def __init__(self, kind: int):
        self.cname, self.kind, self.c = bp.NAME, kind, bp.C
        self.p = bp.R if kind == FR else bp.P
        self.N = 9 if kind == FR else 14  # field_constants.hpp: GM_BLS12381_F{R,P}_N29
        self.R = 1 << (lm.RADIX * self.N)
        self.Rinv = pow(self.R, -1, self.p)
        self.beta = -1

    @property
    def headroom(self):
        return self.R // self.p


def _run(ctx, F, fam, K, chain, rows, width=1):
    n = len(rows)
    nops = len(rows[0]) // width
    arrays = [b"".join(F.enc(r[k * width + c]) for r in rows for c in range(width)) for k in range(nops)]
    out = ctx.test_field_raw_op(2, F.kind, fam * 100 + K, chain, arrays, n, n * width * 4 * F.N)
    L = F.limbs(out)
    assert len(L) == n * width
    return [lm.Field.val(l) for l in L], L


def test_headroom_constants():
    assert Field381(FR).headroom == 70 and Field381(FP).headroom == 41291124


@pytest.mark.parametrize("kind", [0, 1, 2])
def test_field_ops(gm_ctx, kind):
    """mul, add, sub, neg, inv, sqr of gm_test_field_op on edge and random values."""
    p = bp.R if kind == 0 else bp.P
    rng = random.Random(3810 + kind)
    edge = [0, 1, 2, p - 1, p - 2, (p - 1) // 2, (p + 1) // 2, 1 << (p.bit_length() - 1), (1 << (p.bit_length() - 1)) - 1]
    width = 2 if kind == 2 else 1
    xs = [tuple(rng.choice(edge) for _ in range(width)) for _ in range(40)] + \
         [tuple(rng.randrange(p) for _ in range(width)) for _ in range(88)]
    ys = list(xs)
    rng.shuffle(ys)
    nb = 32 if kind == 0 else 48
    R64 = 1 << (8 * nb)
    enc = lambda rows: b"".join((v * R64 % p).to_bytes(nb, "little") for r in rows for v in r)
    dec = lambda b: [int.from_bytes(b[i:i + nb], "little") * pow(R64, -1, p) % p for i in range(0, len(b), nb)]
    F2 = __import__("pyref").F2(bp.C)
    if kind == 2:
        ops = {0: F2.mul, 1: F2.add, 2: F2.sub, 3: lambda a, b: F2.neg(a),
               4: lambda a, b: F2.inv(a) if any(a) else (0, 0), 5: lambda a, b: F2.mul(a, a)}
    else:
        ops = {0: lambda a, b: (a[0] * b[0] % p,), 1: lambda a, b: ((a[0] + b[0]) % p,),
               2: lambda a, b: ((a[0] - b[0]) % p,), 3: lambda a, b: (-a[0] % p,),
               4: lambda a, b: (pow(a[0], p - 2, p),), 5: lambda a, b: (a[0] * a[0] % p,)}
    for op, f in ops.items():
        got = dec(gm_ctx.test_field_op(2, kind, op, enc(xs), enc(ys)))
        exp = [v for a, b in zip(xs, ys) for v in f(a, b)]
        assert got == exp, (kind, op)


# The bounds the Fr kernels state (ntt.hip NTT_BOUND, in multiples of p): the
# operand that meets a canonical twiddle (< p) in a lazy product.
FR_BOUNDS = [
    ("DIF round: fe_sub_cf<5>(s0, s1)", 9),
    ("DIF / DIT w_4 round outputs", 8),
    ("growing DIF round B = 8: fe_sub_cf<17>(s0, s1)", 33),
    ("growing DIF w_4 round B = 16 outputs -> inter-pass twiddle (canonical, < p)", 64),
    ("fe_sub_cf<2B + 1> at B = 16", 65),
    ("growing DIT round: fe_sub_cf<3>(e2, v3)", 19),
    ("growing DIT store: outputs x post factor", 20),
]


@pytest.mark.parametrize("chain", [0, 2])
def test_fr_named_maxima(gm_ctx, chain):
    """Every claimed bound K of an Fr product operand is a row: K <= R' / r (the
    condition a 128 p^2 product -- a lazily reduced twiddle -- would fail), and the
    product (K p - 1)(p - 1) comes out below 2p, congruent and normalised."""
    F = Field381(FR)
    p = F.p
    rows, tags = [], []
    for what, K in FR_BOUNDS:
        assert K <= F.headroom, (what, K)
        assert (K * p - 1) * (p - 1) < F.R * p, what
        rows.append((K * p - 1, p - 1))
        tags.append(what)
    assert not 128 <= F.headroom  # what a < 2p inter-pass twiddle after < 64p would need
    vals, limbs = _run(gm_ctx, F, MUL_LZ, 0, chain, rows)
    for (a, b), v, l, what in zip(rows, vals, limbs, tags):
        assert v % p == F.redc(a * b) % p and v < 2 * p and F.normalised(l), (what, chain)
    # the same operands through the carry-free difference the rounds use:
    # fe_sub_cf<17>(a, b) * t with a < 32p - ..., value below a + 17p
    a, b, t = 16 * p - 1, 0, p - 1
    vals, limbs = _run(gm_ctx, F, SUB_CF_MUL, 17, chain, [(a, b, t)])
    assert vals[0] % p == F.redc((a - b + 17 * p) * t) % p and vals[0] < 2 * p and F.normalised(limbs[0])
    # reductions that bring the stores back: < 4p -> < 2p (the DIT store of this field)
    vals, limbs = _run(gm_ctx, F, REDUCE_K, 2, 0, [(4 * p - 1,), (2 * p,), (2 * p - 1,), (0,)])
    assert vals == [2 * p - 1, 0, 2 * p - 1, 0] and all(v < 1 << 256 for v in vals)


@pytest.mark.parametrize("chain", [0, 1, 2])
def test_fp_named_maxima(gm_ctx, chain):
    """The G1 add's products at the top of their ranges (curve.hpp): 100 p^2,
    76 p^2 through the unsigned two-product reduction; R' / p ~ 2^25, so every
    result is below p + 100 p / 2^25 < 1.01 p."""
    F = Field381(FP)
    p = F.p
    m = lambda k: k * p - 1

    def one(fam, K, ops, integer, width=1, comp=0):
        vals, limbs = _run(gm_ctx, F, fam, K, chain, [ops], width)
        assert vals[comp] % p == F.redc(integer) % p and 100 * vals[comp] < 101 * p and F.normalised(limbs[comp]), \
            (chain, fam, K)

    one(MUL_LZ, 0, (m(10), m(10)), m(10) ** 2)
    one(SQR_LZ, 0, (m(10),), m(10) ** 2)
    one(MUL2_NEGK, 5, (m(6), m(11), 0, m(2)), m(6) * m(11) + 5 * p * m(2))
    one(MUL2, 0, (m(6), m(11), 5 * p, m(2)), m(6) * m(11) + 5 * p * m(2))
    one(MUL2_NEGK, 3, (m(4), m(4), m(2), m(2)), m(4) * m(4) + (3 * p - m(2)) * m(2))


def _check_fp2(F, tag, rows, vals, limbs, expect, bound):
    p = F.p
    for i, r in enumerate(rows):
        e = expect(r)
        for c in (0, 1):
            v, l = vals[2 * i + c], limbs[2 * i + c]
            t = tag + (c, [x // p for x in r])
            assert v % p == F.redc(e[c]) % p, t
            assert 100 * v < bound * p, t
            assert F.normalised(l), t


@pytest.mark.parametrize("chain", [0, 1])
def test_pf2_lane_pairs(gm_ctx, chain):
    """Lane-pair Fp2 products and squarings at (non-residue -1, 14 limbs): pf2_mul
    takes a0 b0 + (5p - a1) b1 in one unsigned reduction, inputs < 4p per component
    at every combination of their multiples of p and at the maxima; pf2_sqr<IN> is
    (a0 + a1)(a0 - a1 + IN p).  36 p^2 / R' and 64 p^2 / R' are below 2^-19: < 1.01p."""
    F = Field381(FP)
    p = F.p
    jm = (4, 4, 4, 4)
    rows = lm.lifted(F, jm, seed=3811, cap=600)
    assert lm.covers_every_j(rows, jm, p)
    top = 4 * p - 1
    rows += [(top, top, top, top), (top, 0, top, top), (0, top, top, top), (top, top, 0, top), (0, 0, 0, 0)]
    vals, limbs = _run(gm_ctx, F, PF2_MUL, 0, chain, rows, width=2)
    _check_fp2(F, (chain, "pf2_mul"), rows, vals, limbs, lambda r: lm.f2_mul(F, r[:2], r[2:]), 101)
    for IN in (1, 2, 4):
        rows = lm.lifted(F, (IN, IN), seed=3812 + IN, per_combo=16) + [(IN * p - 1, IN * p - 1), (IN * p - 1, 0),
                                                                       (0, IN * p - 1)]
        vals, limbs = _run(gm_ctx, F, PF2_SQR, IN, chain, rows, width=2)
        _check_fp2(F, (chain, "pf2_sqr<%d>" % IN), rows, vals, limbs, lambda r: lm.f2_mul(F, r, r), 101)


def test_fe2_one_lane(gm_ctx):
    """fe2_mul_lz (inputs < 6p per component) and fe2_sqr_lz<4>, results < 2p."""
    F = Field381(FP)
    rows = lm.lifted(F, (6, 6, 6, 6), seed=3820, cap=400)
    vals, limbs = _run(gm_ctx, F, FE2_MUL, 0, 0, rows, width=2)
    _check_fp2(F, ("fe2_mul_lz",), rows, vals, limbs, lambda r: lm.f2_mul(F, r[:2], r[2:]), 200)
    rows = lm.lifted(F, (4, 4), seed=3821, per_combo=16)
    vals, limbs = _run(gm_ctx, F, FE2_SQR, 4, 0, rows, width=2)
    _check_fp2(F, ("fe2_sqr_lz<4>",), rows, vals, limbs, lambda r: lm.f2_mul(F, r, r), 200)
