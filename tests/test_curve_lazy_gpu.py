"""The lazily reduced point additions (curve.hpp, pair_fp2.hpp) over every
representative their contracts allow, through the raw-limb hook
gm_test_point_raw_op: raw XYZZ accumulators in, raw XYZZ accumulators out.

Every result must decode (x / zz, y / zzz in big integers) to the group result
of oracle/pyref.py, satisfy zz^3 = zzz^2, show infinity the way xyzz_is_inf /
pxyzz_is_inf read it (every limb of zz zero), and obey the output contract
written at the function:
  xyzz_add_aff_lz G1  curve.hpp:118-123  x < 8p; y < 1.5p after an add, <= p after
                      the copy of a first entry, canonical after a doubling;
                      zz, zzz < 2p
  xyzz_add_aff_lz G2  curve.hpp:176-178  every component < 2p
  pxyzz_add_aff       pair_fp2.hpp:186-188  every component < 2p
  xyzz_add_lz         curve.hpp:273-276  every coordinate < 2p; an operand comes
                      back as it came when the other one is infinity
  xyzz_canon_raw, pxyzz_add, pxyzz_dbl, pxyzz_dbl_aff   canonical
with normalised limbs throughout.  The case builders check their own coverage
without a GPU (test_case_tables_cover_their_claims)."""
import itertools
import random

import pytest

import lazy_model as lm
import pyref

CURVES = ["bn254", "bls12377"]
G1_ADD_AFF, G1_ADD, G1_CANON, G2_ADD_AFF, G2P_ADD_AFF, G2P_DBL_AFF, G2P_ADD, G2P_DBL = range(8)

# multiples of p per flat accumulator integer (x, y, zz, zzz; G2: a0, a1 of each)
LIFT_G1_AFF = (8, 4, 2, 2)     # curve.hpp:119 "x < 8p, y < 4p, zz < 2p, zzz < 2p"
LIFT_G1_FULL = (8, 2, 2, 2)    # curve.hpp:273-274 "x < 8p, y, zz, zzz < 2p on either operand"
LIFT_G2 = (2,) * 8             # curve.hpp:177 "every component of a.x, a.y, a.zz, a.zzz < 2p"
CANONICAL_G2 = (1,) * 8        # pair_fp2.hpp:379 "canonical components in and out"


class Case:
    def __init__(self, acc, js, other, flag, label, exp, other_js=None):
        self.acc, self.js, self.other, self.flag, self.label, self.exp = acc, js, other, flag, label, exp
        self.other_js = other_js


def mixed_cases(M, jm, seed):
    """Accumulators for points Q in every combination of representatives, each
    against: a generic point with both signs, Q (doubling), -Q (infinity), Q with
    the sign set (infinity), -Q with the sign set (doubling), the (0, 0) point
    (unchanged); and an infinite accumulator with both signs (the copy path)."""
    rng = random.Random(seed)
    G = M.G
    pts = pyref.random_points(M.F.c, 3, seed, M.g2)
    others = pyref.random_points(M.F.c, 4, seed + 1, M.g2)
    cases = []
    for idx, js in enumerate(itertools.product(*[range(j) for j in jm])):
        Q = pts[idx % len(pts)]
        s = M.one() if rng.random() < 0.5 else M.random_s(rng)
        acc = M.lift(M.acc_from(Q, s), js)
        T = others[idx % len(others)]
        Q2 = G.add(Q, Q)
        for label, other, flag, exp in (("add", T, 0, G.add(Q, T)), ("add", T, 1, G.add(Q, G.neg(T))),
                                        ("dbl", Q, 0, Q2), ("inf", G.neg(Q), 0, None), ("inf", Q, 1, None),
                                        ("dbl", G.neg(Q), 1, Q2), ("same", None, idx & 1, Q)):
            cases.append(Case(acc, js, other, flag, label, exp))
    for T in others:
        for flag in (0, 1):
            cases.append(Case(M.acc_inf(), None, T, flag, "copy", G.neg(T) if flag else T))
    if not M.g2:
        cases += g1_targeted_cases(M, pts, others, seed)
    return cases


def g1_pd(M, acc, T):
    """Pd = U2 - X1 + 8p of the G1 mixed add (curve.hpp:145) for accumulator acc and point T"""
    F = M.F
    return F.redc_exact(F.to_mont(T[0]) * acc[2]) - acc[0] + 8 * F.p


def g1_targeted_cases(M, pts, others, seed):
    """The ends of two ranges that uniform data does not reach.
    Pd = 9p (fe_is_zero_lz<10>, curve.hpp:148): U2 = x zz / R' lands in [p, 2p) only
    for about x zz / (R' p) of the accumulators -- 1 % for BN254, 2^-28 for
    BLS12-377, where no such row exists -- so s is searched for it.
    Y1 in the top limb of 4p (fe_negk_cf<5>, curve.hpp:171: 5p - Y1 with the
    smallest K p that keeps the top limb non-negative): y s^3 is placed at p - 1 - k
    by a cube root, then lifted by 3p."""
    rng = random.Random(seed + 7)
    G, F, p = M.G, M.F, M.F.p
    cases = []
    if F.R < 1024 * p:
        found = 0
        for _ in range(4000):
            Q = pts[found % len(pts)]
            acc = M.lift(M.acc_from(Q, M.random_s(rng)), (0, rng.randrange(4), 1, rng.randrange(2)))
            if g1_pd(M, acc, Q) == 9 * p:
                Q2 = G.add(Q, Q)
                for label, other, flag, exp in (("dbl", Q, 0, Q2), ("inf", G.neg(Q), 0, None), ("inf", Q, 1, None),
                                                ("dbl", G.neg(Q), 1, Q2)):
                    cases.append(Case(acc, "Pd=9p", other, flag, label, exp))
                found += 1
                if found == 3:
                    break
    start = 0
    for i, Q in enumerate(pts):
        acc, k = M.acc_with_y(Q, p - 1, start)
        start = k + 1
        acc = M.lift(acc, (i, 3, i & 1, 1 - (i & 1)))
        T = others[i % len(others)]
        cases.append(Case(acc, "Y1~4p", T, 0, "add", G.add(Q, T)))
        cases.append(Case(acc, "Y1~4p", T, 1, "add", G.add(Q, G.neg(T))))
    return cases


def full_cases(M, jm, seed):
    """Pairs of accumulators (a, b), each in every representative: generic, a = b
    in different representatives and with different s, a = -b, either side
    infinite."""
    rng = random.Random(seed)
    G = M.G
    pts = pyref.random_points(M.F.c, 3, seed, M.g2)
    others = pyref.random_points(M.F.c, 4, seed + 1, M.g2)
    combos = list(itertools.product(*[range(j) for j in jm]))
    perm = combos[:]
    rng.shuffle(perm)
    cases = []
    for idx, (ja, jb) in enumerate(zip(combos, perm)):
        Q, T = pts[idx % len(pts)], others[idx % len(others)]
        sa, sb = M.random_s(rng), (M.one() if idx % 3 == 0 else M.random_s(rng))
        a = M.lift(M.acc_from(Q, sa), ja)
        mk = lambda P: M.lift(M.acc_from(P, sb), jb)
        for label, b, exp in (("add", mk(T), G.add(Q, T)), ("dbl", mk(Q), G.add(Q, Q)), ("inf", mk(G.neg(Q)), None),
                              ("b_inf", M.acc_inf(), Q)):
            cases.append(Case(a, ja, b, 0, label, exp, jb))
        cases.append(Case(M.acc_inf(), None, mk(T), 0, "a_inf", T, jb))
    return cases


def _bounds(M, op, label):
    """exclusive upper bounds of the flat output integers, as a list of
    (numerator, denominator) multiples of p"""
    n = M.ncomp
    canonical = [(1, 1)] * (4 * n)
    if label in ("dbl",) or op in (G1_CANON, G2P_ADD, G2P_DBL, G2P_DBL_AFF):
        return canonical
    if label == "copy":
        # G1: y = p - y' is <= p (fe_pminus, p itself for y' = 0: never on the curve)
        return canonical
    if op == G1_ADD_AFF:
        return [(8, 1), (3, 2), (2, 1), (2, 1)]
    return [(2, 1)] * (4 * n)


def _enc_other(M, cases, affine):
    if affine:
        return b"".join(pyref.encode_point(M.F.c, c.other, M.g2) for c in cases)
    return b"".join(M.enc(c.other) for c in cases)


def _run_and_check(ctx, M, op, chain, cases, affine, tag):
    F, p = M.F, M.F.p
    acc_in = b"".join(M.enc(c.acc) for c in cases)
    other = _enc_other(M, cases, affine) if cases[0].other is not None or affine else None
    flags = bytes(c.flag for c in cases)
    out = ctx.test_point_raw_op(F.cname, M.g2, op, chain, acc_in, other, flags, len(cases))
    flats, limbs = M.dec(out)
    w = 4 * M.ncomp * 4 * F.N
    for i, (c, flat, L) in enumerate(zip(cases, flats, limbs)):
        t = tag + (c.label, c.flag, c.js, c.other_js)
        assert all(F.normalised(l) for l in L), t
        if c.label in ("same", "b_inf"):
            assert out[i * w:(i + 1) * w] == acc_in[i * w:(i + 1) * w], t      # limb for limb
        elif c.label == "a_inf":
            assert out[i * w:(i + 1) * w] == other[i * w:(i + 1) * w], t
        else:
            for v, (num, den) in zip(flat, _bounds(M, op, c.label)):
                assert den * v < num * p, t
        pt, consistent = M.affine(flat)
        assert consistent, t                                                   # zz^3 = zzz^2
        assert pt == c.exp, t
        assert M.is_inf(flat) == (c.exp is None), t                            # infinity: zz's limbs all zero
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("chain", [0, 2])
@pytest.mark.parametrize("cname", CURVES)
def test_g1_mixed_add(gm_ctx, cname, chain):
    M = lm.GroupModel(cname, False)
    _run_and_check(gm_ctx, M, G1_ADD_AFF, chain, mixed_cases(M, LIFT_G1_AFF, 31), True, (cname, "g1 aff", chain))


@pytest.mark.gpu
@pytest.mark.parametrize("cname", CURVES)
def test_g1_full_add_and_canon(gm_ctx, cname):
    M = lm.GroupModel(cname, False)
    cases = full_cases(M, LIFT_G1_FULL, 32)
    _run_and_check(gm_ctx, M, G1_ADD, 0, cases, False, (cname, "g1 full"))
    # xyzz_canon_raw (curve.hpp:267): the same accumulators, canonical and the same point
    canon = [Case(c.acc, c.js, None, 0, "canon", M.affine(c.acc)[0]) for c in cases]
    out = _run_and_check(gm_ctx, M, G1_CANON, 0, canon, False, (cname, "g1 canon"))
    assert M.dec(out)[0] == [[v % M.F.p for v in c.acc] for c in canon]


@pytest.mark.gpu
@pytest.mark.parametrize("variant", ["lane", "pair0", "pair1"])
@pytest.mark.parametrize("cname", CURVES)
def test_g2_mixed_add(gm_ctx, cname, variant):
    M = lm.GroupModel(cname, True)
    op, chain = {"lane": (G2_ADD_AFF, 0), "pair0": (G2P_ADD_AFF, 0), "pair1": (G2P_ADD_AFF, 1)}[variant]
    _run_and_check(gm_ctx, M, op, chain, mixed_cases(M, LIFT_G2, 33), True, (cname, "g2 aff", variant))


@pytest.mark.gpu
@pytest.mark.parametrize("cname", CURVES)
def test_g2_pair_full_ops(gm_ctx, cname):
    """pxyzz_add, pxyzz_dbl, pxyzz_dbl_aff: canonical components in and out."""
    M = lm.GroupModel(cname, True)
    G = M.G
    cases = full_cases(M, CANONICAL_G2, 34)
    rng = random.Random(35)
    pts = pyref.random_points(M.F.c, 24, 36, True)
    for k in range(0, 24, 2):
        Q, T = pts[k], pts[k + 1]
        sa, sb = M.random_s(rng), M.random_s(rng)
        a = M.acc_from(Q, sa)
        for label, b, exp in (("add", M.acc_from(T, sb), G.add(Q, T)), ("dbl", M.acc_from(Q, sb), G.add(Q, Q)),
                              ("inf", M.acc_from(G.neg(Q), sb), None), ("b_inf", M.acc_inf(), Q)):
            cases.append(Case(a, None, b, 0, label, exp))
        cases.append(Case(M.acc_inf(), None, M.acc_from(T, sb), 0, "a_inf", T))
    _run_and_check(gm_ctx, M, G2P_ADD, 0, cases, False, (cname, "pxyzz_add"))
    dbl = [Case(c.acc, None, None, 0, "dbl", G.add(M.affine(c.acc)[0], M.affine(c.acc)[0])) for c in cases]
    _run_and_check(gm_ctx, M, G2P_DBL, 0, dbl, False, (cname, "pxyzz_dbl"))
    dba = [Case(M.acc_inf(), None, Q, 0, "dbl", G.add(Q, Q)) for Q in pts]
    _run_and_check(gm_ctx, M, G2P_DBL_AFF, 0, dba, True, (cname, "pxyzz_dbl_aff"))


def chain_plan(M, seed, lanes=4, steps=16):
    """Per lane a sequence of (point, sign) with a doubling (the running sum
    itself) at step 6, a cancellation (minus the running sum) at step 10, so
    step 11 copies into an infinite accumulator.  Returns the steps and the
    running sums after each."""
    rng = random.Random(seed)
    G = M.G
    pts = pyref.random_points(M.F.c, 8, seed, M.g2)
    sums = [None] * lanes
    plan = []
    for k in range(steps):
        step = []
        for l in range(lanes):
            T, flag, label = pts[rng.randrange(len(pts))], rng.randrange(2), "add"
            if sums[l] is None:
                label = "copy"
            elif k == 6:
                flag = l & 1
                T, label = (G.neg(sums[l]) if flag else sums[l]), "dbl"
            elif k == 10:
                flag = l & 1
                T, label = (sums[l] if flag else G.neg(sums[l])), "inf"
            elif sums[l] == T or sums[l] == G.neg(T):
                T, flag = pts[0], 0          # keep the unplanned special cases out
            sums[l] = G.add(sums[l], G.neg(T) if flag else T)
            step.append((T, flag, label, sums[l]))
        plan.append(step)
    return plan


@pytest.mark.gpu
@pytest.mark.parametrize("variant", ["g1c0", "g1c2", "lane", "pair0", "pair1"])
@pytest.mark.parametrize("cname", CURVES)
def test_chained_accumulation(gm_ctx, cname, variant):
    """acc_out of one call is acc_in of the next through 16 points with a
    doubling and a cancellation mid-way: the contract is closed under the
    operation, not merely met once."""
    g2 = not variant.startswith("g1")
    op, chain = {"g1c0": (G1_ADD_AFF, 0), "g1c2": (G1_ADD_AFF, 2), "lane": (G2_ADD_AFF, 0),
                 "pair0": (G2P_ADD_AFF, 0), "pair1": (G2P_ADD_AFF, 1)}[variant]
    M = lm.GroupModel(cname, g2)
    plan = chain_plan(M, 41)
    accs = [M.acc_inf() for _ in plan[0]]
    seen = set()
    for k, step in enumerate(plan):
        cases = [Case(acc, None, T, flag, label, exp) for acc, (T, flag, label, exp) in zip(accs, step)]
        out = _run_and_check(gm_ctx, M, op, chain, cases, True, (cname, variant, "step", k))
        accs = M.dec(out)[0]
        seen |= {c.label for c in cases}
    assert seen == {"add", "copy", "dbl", "inf"}


@pytest.mark.gpu
def test_point_hook_rejects_what_the_library_does_not_build(gm_ctx):
    import gnark_mi355x as gm
    M = lm.GroupModel("bn254", False)
    acc = M.enc(M.acc_inf())
    pt = pyref.encode_point(M.F.c, None, False)
    for g2, op, chain in ((False, G1_ADD_AFF, 1), (False, G2P_ADD, 0), (True, G1_ADD, 0), (True, G2P_ADD_AFF, 2)):
        with pytest.raises(gm.GmError):
            gm_ctx.test_point_raw_op("bn254", g2, op, chain, acc * 2, pt * 2, b"\0", 1)


# ---------------------------------------------------------------------------
# CPU self-check: the tables cover what they claim
# ---------------------------------------------------------------------------
def _in_contract(M, flat, jm):
    return all(0 <= v < j * M.F.p for v, j in zip(flat, jm))


@pytest.mark.parametrize("cname", CURVES)
@pytest.mark.parametrize("which", ["g1_aff", "g2_aff", "g1_full", "g2_full"])
def test_case_tables_cover_their_claims(cname, which):
    g2 = which.startswith("g2")
    M = lm.GroupModel(cname, g2)
    G, p = M.G, M.F.p
    mixed = which.endswith("aff")
    jm = {"g1_aff": LIFT_G1_AFF, "g2_aff": LIFT_G2, "g1_full": LIFT_G1_FULL, "g2_full": CANONICAL_G2}[which]
    cases = mixed_cases(M, jm, 31) if mixed else full_cases(M, jm, 32)
    assert {c.label for c in cases} == ({"add", "dbl", "inf", "same", "copy"} if mixed
                                        else {"add", "dbl", "inf", "a_inf", "b_inf"})
    for label in ("add", "dbl", "inf"):
        sub = [c for c in cases if c.label == label]
        # every j of every coordinate occurs (on both operands of the full add)
        for k, j in enumerate(jm):
            assert {c.acc[k] // p for c in sub} >= set(range(j)), (label, k)
            assert all(c.acc[k] < j * p for c in sub), (label, k)
            if not mixed:
                assert {c.other[k] // p for c in sub} == set(range(j)), (label, k)
    for c in cases:
        P, ok = M.affine(c.acc)
        assert ok
        if c.label in ("copy", "a_inf"):
            assert P is None and M.is_inf(c.acc)
        else:
            assert P is not None and _in_contract(M, c.acc, jm) and G.on_curve(P)
        if mixed:
            T = G.neg(c.other) if c.flag else c.other
        else:
            T, ok = M.affine(c.other)
            assert ok and (M.is_inf(c.other) or _in_contract(M, c.other, jm))
            assert M.is_inf(c.other) == (c.label == "b_inf")
        if c.label == "dbl":
            assert P == T and c.exp == G.add(P, P) and c.exp is not None
        elif c.label == "inf":
            assert P == G.neg(T) and c.exp is None
        elif c.label == "add":
            assert P != T and P != G.neg(T) and c.exp == G.add(P, T) and c.exp is not None
        elif c.label == "same":
            assert c.other is None and c.exp == P
    if which == "g1_aff":
        N = M.F.N
        pd = {g1_pd(M, c.acc, c.other) for c in cases if c.label in ("dbl", "inf")}
        assert all(v % p == 0 for v in pd)
        # every multiple the zero test can meet: 1..9 (BLS12-377: U2 < p, so 1..8)
        assert {v // p for v in pd} == set(range(1, 10 if cname == "bn254" else 9))
        top = [c for c in cases if c.js == "Y1~4p"]
        assert len(top) >= 4 and {c.flag for c in top} == {0, 1}
        assert all(c.acc[1] >> (lm.RADIX * (N - 1)) == (4 * p) >> (lm.RADIX * (N - 1)) for c in top)
    if mixed:
        assert {c.flag for c in cases if c.label == "dbl"} == {0, 1}
        assert {c.flag for c in cases if c.label == "inf"} == {0, 1}
        assert {c.flag for c in cases if c.label == "copy"} == {0, 1}
    else:
        # a = b in a different representative and with a different s
        assert any(c.acc != c.other for c in cases if c.label == "dbl")
    assert len(cases) <= 2100


@pytest.mark.parametrize("g2", [False, True])
@pytest.mark.parametrize("cname", CURVES)
def test_chain_plan_has_its_special_steps(cname, g2):
    M = lm.GroupModel(cname, g2)
    G = M.G
    plan = chain_plan(M, 41)
    sums = [None] * len(plan[0])
    for k, step in enumerate(plan):
        for l, (T, flag, label, exp) in enumerate(step):
            S = G.neg(T) if flag else T
            assert exp == G.add(sums[l], S)
            assert label == ("copy" if sums[l] is None else "dbl" if sums[l] == S else
                             "inf" if sums[l] == G.neg(S) else "add")
            sums[l] = exp
        assert {x[2] for x in step} == ({"dbl"} if k == 6 else {"inf"} if k == 10 else
                                        {"copy"} if k in (0, 11) else {"add"})
    assert {x[1] for x in plan[6]} == {0, 1} and {x[1] for x in plan[10]} == {0, 1}


def test_model_roundtrip():
    """acc_from / affine / lift are inverse to each other and infinity reads as zz = 0."""
    for cname in CURVES:
        for g2 in (False, True):
            M = lm.GroupModel(cname, g2)
            rng = random.Random(5)
            for Q in pyref.random_points(M.F.c, 3, 9, g2):
                acc = M.acc_from(Q, M.random_s(rng))
                assert M.affine(acc) == (Q, True)
                assert M.affine(M.lift(acc, [1] * len(acc))) == (Q, True)
                assert M.dec(M.enc(acc))[0] == [acc]
            assert M.affine(M.acc_inf()) == (None, True) and M.is_inf(M.acc_inf())
