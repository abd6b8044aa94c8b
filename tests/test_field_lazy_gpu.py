"""Element-wise parity of the lazily reduced field layer (field.hpp, pair_fp2.hpp)
against Python integers, through the raw-limb hook gm_test_field_raw_op: the
test picks the representative v + j p of every operand and reads every limb of
the result.  Per row: the value (an integer identity, or the residue of a
Montgomery product A B / R'), the range the comment at the function or its call
site promises, and the limbs (normalised unless documented otherwise).

A row is (family, K, bounds on the operands in multiples of p, expected value,
exclusive upper bound in units of p / 100, where the bound is written)."""
import pytest

import lazy_model as lm

CURVES = ["bn254", "bls12377"]
FR, FP = 0, 1

MUL_LZ, SQR_LZ, MUL, MUL2, MUL2_NEGK, ADD_LZ, SUB_LZ, SUB2X_LZ, SUB_CF_MUL, CNEG_SUB, PMINUS, REDUCE_K, CANON, \
    TO2P, IS_ZERO, TIMES5, FE2_MUL, FE2_SQR, PF2_MUL, PF2_SQR, PF2_MUL_SUB, MUL4_REDC = range(22)


def _run(ctx, F, fam, K, chain, rows, width=1):
    """rows: tuples of integers, one per operand -> (values, limbs) per element;
    width 2: operands are Fp2 components (two integers per operand array)."""
    n = len(rows)
    nops = len(rows[0]) // width
    arrays = [b"".join(F.enc(r[k * width + c]) for r in rows for c in range(width)) for k in range(nops)]
    out = ctx.test_field_raw_op(F.cname, F.kind, fam * 100 + K, chain, arrays, n, n * width * 4 * F.N)
    L = F.limbs(out)
    assert len(L) == n * width
    return [lm.Field.val(l) for l in L], L


def _to2p(F, x, M):
    for k in (8, 4, 2):
        if M > k and x >= k * F.p:
            x -= k * F.p
    return x


# ---------------------------------------------------------------------------
# products: value is a residue, range < ab / R' + p and the documented figure
# ---------------------------------------------------------------------------
# (name, family, K, operand bounds (multiples of p), integer that is reduced,
#  documented bound in p / 100, where)
def _product_rows(F):
    p = F.p
    rows = [
        # curve.hpp:124-125 "every product below has inputs with ab <= 100 p^2 (largest: P^2 with P < 10p)";
        # field.hpp:375-378 "with ab < R' p its output is already < 2p"
        ("mul 100p^2", MUL_LZ, 0, (10, 10), lambda a, b: a * b, 200, "field.hpp:375, curve.hpp:125"),
        ("sqr Pd<10p", SQR_LZ, 0, (10,), lambda a: a * a, 200, "curve.hpp:158"),
        # ntt.hip:320 "every product input < 33 p^2 < R' p" (operand < 33p, canonical twiddle)
        ("mul 33p x tw", MUL_LZ, 0, (33, 1), lambda a, b: a * b, 200, "ntt.hip:320"),
        # ntt.hip:649 "inputs < 20p: (20p) p < R' p, output canonical"
        ("mul reduce 20p x p", MUL, 0, (20, 1), lambda a, b: a * b, 100, "ntt.hip:649"),
        ("mul reduce canonical", MUL, 0, (1, 1), lambda a, b: a * b, 100, "field.hpp:265"),
    ]
    if F.kind == FP:
        rows += [
            # curve.hpp:164-166 "R (< 6p) (Q - X3 + 9p < 11p) + (5p - Y1) PPP (< 2p) ... < 76 p^2 / R' + p < 1.5p"
            ("mul2 76p^2 x2 given", MUL2, 0, (6, 11, 5, 2), lambda a, b, c, d: a * b + c * d, 150, "curve.hpp:166"),
            ("mul2 negk5 76p^2", MUL2_NEGK, 5, (6, 11, 4, 2), lambda a, b, c, d: a * b + (5 * p - c) * d, 150,
             "curve.hpp:166"),
            # curve.hpp:305-306 "R (< 4p) (Q - X3 + 2p < 4p) + (3p - S1) PPP ... < 22 p^2 / R' + p < 1.2p"
            ("mul2 negk3 22p^2", MUL2_NEGK, 3, (4, 4, 2, 2), lambda a, b, c, d: a * b + (3 * p - c) * d, 120,
             "curve.hpp:306"),
        ]
        if F.N <= 10:
            # curve.hpp:167-171 Q - X3 + 9p carry-free (Q < 2p, X3 < 8p), times R < 6p
            rows.append(("sub_cf9 x R", SUB_CF_MUL, 9, (2, 8, 6), lambda a, b, c: (a - b + 9 * p) * c, 200,
                         "curve.hpp:171"))
        if F.cname == "bn254":
            # field.hpp:709-710 "(a0 + a1)(b0 + b1) < 144 p^2 < R' p for BN254"
            rows.append(("mul 144p^2", MUL_LZ, 0, (12, 12), lambda a, b: a * b, 200, "field.hpp:710"))
    else:
        # ntt.hip:319-320: fe_sub_cf<K>(a, b) with a, b < (K - 1) p, times a canonical twiddle
        for K in (3, 5, 9, 17):
            rows.append(("sub_cf%d x tw" % K, SUB_CF_MUL, K, (K - 1, K - 1, 1),
                         lambda a, b, c, K=K: (a - b + K * p) * c, 200, "ntt.hip:333-380"))
    return rows


@pytest.mark.gpu
@pytest.mark.parametrize("chain", [0, 1, 2])
@pytest.mark.parametrize("kind", [FR, FP])
@pytest.mark.parametrize("cname", CURVES)
def test_products(gm_ctx, cname, kind, chain):
    F = lm.Field(cname, kind)
    p = F.p
    for name, fam, K, jm, integer, bound, where in _product_rows(F):
        rows = lm.lifted(F, jm, seed=fam * 100 + K, cap=700)
        assert lm.covers_every_j(rows, jm, p)
        vals, limbs = _run(gm_ctx, F, fam, K, chain, rows)
        for r, v, l in zip(rows, vals, limbs):
            t = integer(*r)
            tag = (cname, kind, chain, name, where, [x // p for x in r])
            assert t < F.R * p, tag                       # inside the function's precondition
            assert v % p == F.redc(t), tag                # value
            assert v * F.R < t + F.R * p, tag             # (t + M p) / R', M < R'
            if fam != MUL:
                assert v == F.redc_exact(t), tag          # the one M < R' that divides
            assert 100 * v < bound * p, tag               # the documented range
            assert F.normalised(l), tag                   # limbs
            if fam == MUL:
                assert v == F.redc(t), tag                # canonical


# ---------------------------------------------------------------------------
# integer identities
# ---------------------------------------------------------------------------
def _identity_rows(F):
    p, fr = F.p, F.kind == FR
    rows = [("add_lz", ADD_LZ, 0, (8, 8), lambda a, b: a + b, lambda a, b: a + b + 1, False, "field.hpp:454")]
    # field.hpp:467 "a - b + K p (requires b < K p; the result is < a + K p)"; top limb keeps the excess
    for K in ((2, 4, 8, 16, 32) if fr else (1, 2, 4, 8, 10, 20)):
        rows.append(("sub_lz<%d>" % K, SUB_LZ, K, (max(K, 2), K), lambda a, b, K=K: a - b + K * p,
                     lambda a, b, K=K: a + K * p + 1, True, "field.hpp:467"))
    # field.hpp:494 "a - K p if a >= K p"
    for K in ((1, 2, 4, 8, 16) if fr else (1, 2, 4, 8)):
        rows.append(("reduce_k<%d>" % K, REDUCE_K, K, (2 * K,), lambda a, K=K: a - K * p if a >= K * p else a,
                     lambda a, K=K: max(K * p, a - K * p + 1), False, "field.hpp:494"))
    # field.hpp:575 "canonical representative of a < 2^L p"
    for L in (1, 2, 3, 4):
        rows.append(("canon<%d>" % L, CANON, L, (1 << L,), lambda a: a % p, lambda a: p, False, "field.hpp:575"))
    if not fr:
        rows += [
            # field.hpp:560-562 "a - b - 2c + K p (b + 2c < K p ...) the result is < a + K p"; curve.hpp:163 "< 8p"
            ("sub2x_lz<6>", SUB2X_LZ, 6, (2, 2, 2), lambda a, b, c: a - b - 2 * c + 6 * p, lambda a, b, c: 8 * p, True,
             "field.hpp:560, curve.hpp:163"),
            # field.hpp:480-481 "p - a for a <= p ... in [0, p]"
            ("pminus", PMINUS, 0, (1,), lambda a: p - a, lambda a: p + 1, False, "field.hpp:480"),
            # field.hpp:733 "5 x for x < 2p (< 10p)"; pair_fp2.hpp:62 "< 20p, normalised limbs" for x < 4p
            ("times5", TIMES5, 0, (4,), lambda a: 5 * a, lambda a: 20 * p, False, "field.hpp:733, pair_fp2.hpp:62"),
        ]
        # field.hpp:712 "x < M p -> x < 2p"
        for M in (4, 6, 8, 10, 12):
            rows.append(("to2p<%d>" % M, TO2P, M, (M,), lambda a, M=M: _to2p(F, a, M), lambda a: 2 * p, False,
                         "field.hpp:712"))
    return rows


@pytest.mark.gpu
@pytest.mark.parametrize("kind", [FR, FP])
@pytest.mark.parametrize("cname", CURVES)
def test_integer_identities(gm_ctx, cname, kind):
    F = lm.Field(cname, kind)
    p = F.p
    for name, fam, K, jm, expect, bound, top_excess, where in _identity_rows(F):
        rows = lm.lifted(F, jm, seed=fam * 100 + K, cap=600)
        assert lm.covers_every_j(rows, jm, p)
        if fam == PMINUS:
            rows.append((p,))                              # a = p -> 0
        vals, limbs = _run(gm_ctx, F, fam, K, 0, rows)
        for r, v, l in zip(rows, vals, limbs):
            tag = (cname, kind, name, where, [x // p for x in r])
            assert v == expect(*r), tag
            assert v < bound(*r), tag
            assert F.normalised(l, top_excess), tag
            if fam in (CANON, TO2P, REDUCE_K, PMINUS, TIMES5):
                assert F.normalised(l), tag


@pytest.mark.gpu
@pytest.mark.parametrize("cname", CURVES)
def test_cneg2p_feeds_sub_lz(gm_ctx, cname):
    """fe_cneg2p_cf (field.hpp:548-552: value in (0, 2p], limbs unnormalised) is
    checked through the two consumers it feeds: fe_sub_lz<4> (curve.hpp:147, Y1 <
    4p, "+-S2 - Y1 < 6p") and fe_sub_lz<2> (pair_fp2.hpp:214, "< 4p")."""
    F = lm.Field(cname, FP)
    p = F.p
    for K in (4, 2):
        base = lm.lifted(F, (2, K), seed=900 + K, per_combo=8)
        rows = [(a, b, 0, neg) for a, b in base for neg in (0, 1)]
        assert lm.covers_every_j(rows, (2, K), p)
        vals, limbs = _run(gm_ctx, F, CNEG_SUB, K, 0, rows)
        for (a, b, _, neg), v, l in zip(rows, vals, limbs):
            tag = (cname, K, neg, a // p, b // p)
            assert v == (2 * p - a if neg else a) - b + K * p, tag
            assert v < (K + 2) * p + 1, tag
            assert F.normalised(l, top_excess=True), tag


@pytest.mark.gpu
@pytest.mark.parametrize("K", [4, 6, 10])
@pytest.mark.parametrize("cname", CURVES)
def test_is_zero_lz(gm_ctx, cname, K):
    """fe_is_zero_lz<K> (field.hpp:584-596): 1 exactly on j p, j < K; the top-limb
    filter must let every j p through and the exact test reject its neighbours."""
    F = lm.Field(cname, FP)
    p = F.p
    rows = []
    for j in range(K):
        jp = j * p
        rows.append((jp, 1))
        rows.append((jp + 1, 0))
        if j:
            rows.append((jp - 1, 0))
        # same top limb as j p, different below
        for i in range(F.N - 1):
            x = jp ^ (0x5555 << (lm.RADIX * i))
            if x < K * p:
                rows.append((x, 0))
    rows += [(v + j * p, 1 if v == 0 else 0) for j in range(K) for v in F.values(K)]
    vals, limbs = _run(gm_ctx, F, IS_ZERO, K, 0, [(x,) for x, _ in rows])
    for (x, e), v, l in zip(rows, vals, limbs):
        assert l[0] == e and v == e, (cname, K, x // p, x % p)
    hit = {x // p for x, e in rows if e}
    assert hit == set(range(K))


@pytest.mark.gpu
@pytest.mark.parametrize("cname", CURVES)
def test_limb_guards(gm_ctx, cname):
    """Functions the library guards by limb count answer GM_ERR_INVALID for the
    other field; so do template constants the library does not instantiate."""
    import gnark_mi355x as gm
    F = lm.Field(cname, FP)
    one = [F.enc(1) * 2] * 4
    bad = [(FP, SUB_LZ * 100 + 3, 0), (FR, IS_ZERO * 100 + 4, 0), (FP, PF2_MUL * 100, 2), (FP, CANON * 100 + 5, 0)]
    if F.N > 11:
        bad.append((FP, SUB_CF_MUL * 100 + 9, 0))         # N <= 11 (field.hpp:542)
    if F.N > 9:
        bad += [(FP, MUL4_REDC * 100, 0), (FP, PF2_MUL_SUB * 100, 0)]   # N <= 9 (pair_fp2.hpp:76)
    for kind, op, chain in bad:
        with pytest.raises(gm.GmError):
            gm_ctx.test_field_raw_op(cname, kind, op, chain, one, 1, 8 * F.N)


# ---------------------------------------------------------------------------
# Fp2: one lane (fe2_*_lz) and lane pairs (pf2_*)
# ---------------------------------------------------------------------------
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


@pytest.mark.gpu
@pytest.mark.parametrize("cname", CURVES)
def test_fe2_one_lane(gm_ctx, cname):
    """fe2_mul_lz (field.hpp:739 "result components < 2p.  Inputs: components <
    6p") and fe2_sqr_lz<4> (field.hpp:758, inputs < 4p), both non-residues."""
    F = lm.Field(cname, FP)
    rows = lm.lifted(F, (6, 6, 6, 6), seed=1600, cap=600)
    assert lm.covers_every_j(rows, (6, 6, 6, 6), F.p)
    vals, limbs = _run(gm_ctx, F, FE2_MUL, 0, 0, rows, width=2)
    _check_fp2(F, (cname, "fe2_mul_lz"), rows, vals, limbs, lambda r: lm.f2_mul(F, r[:2], r[2:]), 200)
    rows = lm.lifted(F, (4, 4), seed=1700, per_combo=16)
    vals, limbs = _run(gm_ctx, F, FE2_SQR, 4, 0, rows, width=2)
    _check_fp2(F, (cname, "fe2_sqr_lz<4>"), rows, vals, limbs, lambda r: lm.f2_mul(F, r, r), 200)


@pytest.mark.gpu
@pytest.mark.parametrize("chain", [0, 1])
@pytest.mark.parametrize("cname", CURVES)
def test_pf2_lane_pairs(gm_ctx, cname, chain):
    """pf2_mul (pair_fp2.hpp:46-54: inputs < 4p per component, the sum is < (16 +
    20) p^2 / R' + p < 1.22p) and pf2_sqr<IN> (pair_fp2.hpp:124, inputs < IN p,
    result < 2p; BETA = -1: < 1.4p, pair_fp2.hpp:134)."""
    F = lm.Field(cname, FP)
    jm = (4, 4, 4, 4)
    rows = lm.lifted(F, jm, seed=1800, cap=600)
    assert lm.covers_every_j(rows, jm, F.p)
    vals, limbs = _run(gm_ctx, F, PF2_MUL, 0, chain, rows, width=2)
    _check_fp2(F, (cname, chain, "pf2_mul 36p^2"), rows, vals, limbs, lambda r: lm.f2_mul(F, r[:2], r[2:]), 122)
    for IN in (1, 2, 4):
        rows = lm.lifted(F, (IN, IN), seed=1900 + IN, per_combo=16)
        vals, limbs = _run(gm_ctx, F, PF2_SQR, IN, chain, rows, width=2)
        _check_fp2(F, (cname, chain, "pf2_sqr<%d>" % IN), rows, vals, limbs, lambda r: lm.f2_mul(F, r, r),
                   140 if F.beta == -1 else 200)


def _mul_sub_rows(F):
    """R, W < 4p; Y, PP < 2p per component (pair_fp2.hpp:114), with the rows where
    one lane's negative side is largest and its positive side smallest."""
    p = F.p
    jm = (4, 4, 4, 4, 2, 2, 2, 2)
    rows = lm.lifted(F, jm, seed=2000, cap=500)
    hi4, hi2 = 4 * p - 1, 2 * p - 1
    # lane 0: R0 W0 + Y1 P1 - R1 W1 - Y0 P0;  lane 1: R1 W0 + R0 W1 - Y1 P0 - Y0 P1
    rows.append((0, hi4, 0, hi4, hi2, 0, hi2, 0))       # lane 0: - 16 p^2 - 4 p^2, positive side 0
    rows.append((0, hi4, hi4, 0, hi2, 0, hi2, 0))
    rows.append((0, 0, 0, 0, hi2, hi2, hi2, hi2))       # lane 1: - 8 p^2, positive side 0
    rows.append((hi4, hi4, hi4, hi4, 0, 0, 0, 0))       # positive side largest
    rows.append((hi4, hi4, hi4, hi4, hi2, hi2, hi2, hi2))
    return jm, rows


@pytest.mark.gpu
def test_mul_sub_four_products(gm_ctx):
    """pf2_mul_sub and fe_mul4_redc (pair_fp2.hpp:68-71, 111-115; BN254 only):
    "the negative products are < 20 p^2 < p R', so the result is >= 0, and <
    2.3p", limbs normalised."""
    F = lm.Field("bn254", FP)
    p = F.p
    jm, rows = _mul_sub_rows(F)
    assert lm.covers_every_j(rows, jm, p)

    def expect(r):
        Rv, W, Y, PP = r[0:2], r[2:4], r[4:6], r[6:8]
        a, b = lm.f2_mul(F, Rv, W), lm.f2_mul(F, Y, PP)
        return (a[0] - b[0], a[1] - b[1])

    vals, limbs = _run(gm_ctx, F, PF2_MUL_SUB, 0, 0, rows, width=2)
    for i, r in enumerate(rows):
        e = expect(r)
        for c in (0, 1):
            v, l = vals[2 * i + c], limbs[2 * i + c]
            t = ("pf2_mul_sub", c, [x // p for x in r])
            assert F.normalised(l), t                      # a negative result would leave a huge top limb
            assert v % p == F.redc(e[c]) % p, t
            assert 10 * v < 23 * p, t
    # fe_mul4_redc itself: x1 y1 + x2 y2 - x3 y3 - x4 y4 with the lane-0 operand roles
    m4 = [(r[0], r[2], r[5], r[7], r[1], r[3], r[4], r[6]) for r in rows]
    vals, limbs = _run(gm_ctx, F, MUL4_REDC, 0, 0, m4, width=2)
    for i, r in enumerate(m4):
        t = ("fe_mul4_redc", [x // p for x in r])
        e = r[0] * r[1] + r[2] * r[3] - r[4] * r[5] - r[6] * r[7]
        v, l = vals[2 * i], limbs[2 * i]
        assert F.normalised(l), t
        assert v % p == F.redc(e) % p, t
        assert 10 * v < 23 * p, t


# ---------------------------------------------------------------------------
# the named maxima, one explicit row each
# ---------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("chain", [0, 1, 2])
@pytest.mark.parametrize("cname", CURVES)
def test_named_maxima(gm_ctx, cname, chain):
    """Both operands at the top of their range together: the 100 p^2, 144 p^2,
    76 p^2, 36 p^2 and 20 p^2 products of the comments."""
    F = lm.Field(cname, FP)
    p = F.p

    def one(fam, K, ops, integer, bound, width=1, comp=0):
        vals, limbs = _run(gm_ctx, F, fam, K, chain, [ops], width)
        assert vals[comp] % p == F.redc(integer) % p and 100 * vals[comp] < bound * p and F.normalised(limbs[comp]), \
            (cname, chain, fam, K)

    m = lambda k: k * p - 1
    one(MUL_LZ, 0, (m(10), m(10)), m(10) ** 2, 200)                                  # 100 p^2, curve.hpp:125
    one(SQR_LZ, 0, (m(10),), m(10) ** 2, 200)
    if cname == "bn254":
        one(MUL_LZ, 0, (m(12), m(12)), m(12) ** 2, 200)                              # 144 p^2, field.hpp:710
    # 76 p^2, curve.hpp:166: R = 6p - 1, Q - X3 + 9p = 11p - 1, 5p - Y1 = 5p, PPP = 2p - 1
    one(MUL2_NEGK, 5, (m(6), m(11), 0, m(2)), m(6) * m(11) + 5 * p * m(2), 150)
    one(MUL2, 0, (m(6), m(11), 5 * p, m(2)), m(6) * m(11) + 5 * p * m(2), 150)
    if chain <= 1:
        # 36 p^2, pair_fp2.hpp:53: lane 0 with a1 = 0: a0 b0 + 5p b1
        r = (m(4), 0, m(4), m(4))
        one(PF2_MUL, 0, r, lm.f2_mul(F, r[:2], r[2:])[0], 122, width=2)
    if cname == "bn254" and chain == 0:
        # 20 p^2 negative, pair_fp2.hpp:70-71, positive side 0
        one(MUL4_REDC, 0, (0, 0, 0, 0, m(4), m(4), m(2), m(2)), -(m(4) ** 2 + m(2) ** 2), 230, width=2)


# ---------------------------------------------------------------------------
# CPU self-check of the model and the input builder
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("kind", [FR, FP])
@pytest.mark.parametrize("cname", CURVES)
def test_model_and_inputs_cover_their_claims(cname, kind):
    F = lm.Field(cname, kind)
    p = F.p
    assert F.N == (14 if (cname, kind) == ("bls12377", FP) else 9) and F.R > 128 * p
    for x in F.edge_values() + [10 * p - 1, 33 * p - 1]:
        assert lm.Field.val(F.limbs(F.enc(x))[0]) == x and F.normalised(F.limbs(F.enc(x))[0])
    lo = F.limbs(F.enc(F.edge_values()[6]))[0]
    m = (p.bit_length() - 1) // lm.RADIX
    assert all(v == lm.MASK for v in lo[:m]) and not any(F.limbs(F.enc(F.edge_values()[7]))[0][:m])
    assert F.redc(F.to_mont(5) * F.to_mont(7)) == F.to_mont(35)
    for name, fam, K, jm, integer, bound, where in _product_rows(F):
        rows = lm.lifted(F, jm, seed=fam * 100 + K, cap=700)
        assert lm.covers_every_j(rows, jm, p), name
        assert tuple(j * p - 1 for j in jm) in rows, name              # all operands at their maximum together
        assert all(0 <= integer(*r) < F.R * p for r in rows), name     # inside the precondition
        assert len(rows) <= 1200, (name, len(rows))
    for name, fam, K, jm, expect, bound, top_excess, where in _identity_rows(F):
        rows = lm.lifted(F, jm, seed=fam * 100 + K, cap=600)
        assert lm.covers_every_j(rows, jm, p), name
        assert all(0 <= expect(*r) < bound(*r) for r in rows), name
    if kind == FP and cname == "bn254":
        jm, rows = _mul_sub_rows(F)
        assert lm.covers_every_j(rows, jm, p)
        # the rows with an empty positive side and the largest negative one are there
        neg0 = [r for r in rows if r[0] * r[2] + r[5] * r[7] == 0 and r[1] * r[3] + r[4] * r[6] > 19 * p * p]
        assert neg0 and all(r[1] * r[3] + r[4] * r[6] < 20 * p * p for r in rows)
