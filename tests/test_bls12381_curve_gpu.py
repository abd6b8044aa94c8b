"""BLS12-381 (curve id 2) lazily reduced point additions at their stated bounds,
through the raw-limb hook gm_test_point_raw_op: the case builders and checks of
test_curve_lazy_gpu.py (every combination of representatives an accumulator's
contract allows -- G1: x < 8p, y < 4p, zz, zzz < 2p, the raw emit form x < 8p,
rest < 2p on both operands of the full add; G2: every component < 2p -- each
against an add with both signs, the doubling case, the cancellation, the (0, 0)
point and the copy into an infinite accumulator), run for the field pair this
curve alone instantiates: 14 limbs with the non-residue -1, one-lane and on lane
pairs.  Results decode to pyref's group law with the curve's CurveParams."""
import random

import pytest

import lazy_model as lm
import pyref
import bls12381_params as bp
import test_curve_lazy_gpu as tc
from test_bls12381_field_gpu import Field381, FP


class Group381(lm.GroupModel):
    """lm.GroupModel for curve id 2 (lm.GroupModel looks its curve up in pyref.CURVES)."""

    def __init__(self, g2: bool):
        self.F = Field381(FP)
        self.g2 = g2
        self.G = pyref.Group(bp.C, g2)
        self.K = pyref.F2(bp.C) if g2 else pyref.F1(bp.C)
        self.ncomp = 2 if g2 else 1


@pytest.mark.gpu
@pytest.mark.parametrize("chain", [0, 2])
def test_g1_mixed_add(gm_ctx, chain):
    M = Group381(False)
    cases = tc.mixed_cases(M, tc.LIFT_G1_AFF, 381)
    assert any(c.js == "Y1~4p" for c in cases)  # y in the top limb of 4p
    tc._run_and_check(gm_ctx, M, tc.G1_ADD_AFF, chain, cases, True, ("bls12381", "g1 aff", chain))


@pytest.mark.gpu
def test_g1_full_add_and_canon(gm_ctx):
    """xyzz_add_lz on raw-emit operands (x < 8p, y, zz, zzz < 2p on either side) and xyzz_canon_raw"""
    M = Group381(False)
    cases = tc.full_cases(M, tc.LIFT_G1_FULL, 382)
    tc._run_and_check(gm_ctx, M, tc.G1_ADD, 0, cases, False, ("bls12381", "g1 full"))
    canon = [tc.Case(c.acc, c.js, None, 0, "canon", M.affine(c.acc)[0]) for c in cases]
    out = tc._run_and_check(gm_ctx, M, tc.G1_CANON, 0, canon, False, ("bls12381", "g1 canon"))
    assert M.dec(out)[0] == [[v % M.F.p for v in c.acc] for c in canon]


@pytest.mark.gpu
@pytest.mark.parametrize("variant", ["lane", "pair0", "pair1"])
def test_g2_mixed_add(gm_ctx, variant):
    """one-lane xyzz_add_aff_lz<Fe2> and the lane-pair pxyzz_add_aff (CH off / on)"""
    M = Group381(True)
    op, chain = {"lane": (tc.G2_ADD_AFF, 0), "pair0": (tc.G2P_ADD_AFF, 0), "pair1": (tc.G2P_ADD_AFF, 1)}[variant]
    tc._run_and_check(gm_ctx, M, op, chain, tc.mixed_cases(M, tc.LIFT_G2, 383), True, ("bls12381", "g2 aff", variant))


@pytest.mark.gpu
def test_g2_pair_full_ops(gm_ctx):
    """pxyzz_add, pxyzz_dbl, pxyzz_dbl_aff: canonical components in and out"""
    M = Group381(True)
    G = M.G
    cases = tc.full_cases(M, tc.CANONICAL_G2, 384)
    rng = random.Random(385)
    pts = pyref.random_points(bp.C, 24, 386, True)
    for k in range(0, 24, 2):
        Q, T = pts[k], pts[k + 1]
        sa, sb = M.random_s(rng), M.random_s(rng)
        a = M.acc_from(Q, sa)
        for label, b, exp in (("add", M.acc_from(T, sb), G.add(Q, T)), ("dbl", M.acc_from(Q, sb), G.add(Q, Q)),
                              ("inf", M.acc_from(G.neg(Q), sb), None), ("b_inf", M.acc_inf(), Q)):
            cases.append(tc.Case(a, None, b, 0, label, exp))
        cases.append(tc.Case(M.acc_inf(), None, M.acc_from(T, sb), 0, "a_inf", T))
    tc._run_and_check(gm_ctx, M, tc.G2P_ADD, 0, cases, False, ("bls12381", "pxyzz_add"))
    dbl = [tc.Case(c.acc, None, None, 0, "dbl", G.add(M.affine(c.acc)[0], M.affine(c.acc)[0])) for c in cases]
    tc._run_and_check(gm_ctx, M, tc.G2P_DBL, 0, dbl, False, ("bls12381", "pxyzz_dbl"))
    dba = [tc.Case(M.acc_inf(), None, Q, 0, "dbl", G.add(Q, Q)) for Q in pts]
    tc._run_and_check(gm_ctx, M, tc.G2P_DBL_AFF, 0, dba, True, ("bls12381", "pxyzz_dbl_aff"))


@pytest.mark.gpu
@pytest.mark.parametrize("variant", ["g1c0", "g1c2", "lane", "pair0", "pair1"])
def test_chained_accumulation(gm_ctx, variant):
    """acc_out of one call is acc_in of the next through 16 points with a doubling
    and a cancellation mid-way: the contract is closed under the operation"""
    g2 = not variant.startswith("g1")
    op, chain = {"g1c0": (tc.G1_ADD_AFF, 0), "g1c2": (tc.G1_ADD_AFF, 2), "lane": (tc.G2_ADD_AFF, 0),
                 "pair0": (tc.G2P_ADD_AFF, 0), "pair1": (tc.G2P_ADD_AFF, 1)}[variant]
    M = Group381(g2)
    plan = tc.chain_plan(M, 387)
    accs = [M.acc_inf() for _ in plan[0]]
    seen = set()
    for k, step in enumerate(plan):
        cases = [tc.Case(acc, None, T, flag, label, exp) for acc, (T, flag, label, exp) in zip(accs, step)]
        out = tc._run_and_check(gm_ctx, M, op, chain, cases, True, ("bls12381", variant, "step", k))
        accs = M.dec(out)[0]
        seen |= {c.label for c in cases}
    assert seen == {"add", "copy", "dbl", "inf"}


# ---- CPU self-check: the tables cover what they claim for this curve ----------
@pytest.mark.parametrize("which", ["g1_aff", "g2_aff", "g1_full", "g2_full"])
def test_case_tables_cover_their_claims(which):
    g2 = which.startswith("g2")
    M = Group381(g2)
    p = M.F.p
    mixed = which.endswith("aff")
    jm = {"g1_aff": tc.LIFT_G1_AFF, "g2_aff": tc.LIFT_G2, "g1_full": tc.LIFT_G1_FULL, "g2_full": tc.CANONICAL_G2}[which]
    cases = tc.mixed_cases(M, jm, 381) if mixed else tc.full_cases(M, jm, 382)
    assert {c.label for c in cases} == ({"add", "dbl", "inf", "same", "copy"} if mixed
                                        else {"add", "dbl", "inf", "a_inf", "b_inf"})
    for label in ("add", "dbl", "inf"):
        sub = [c for c in cases if c.label == label]
        for k, j in enumerate(jm):  # every multiple of p of every coordinate occurs, none beyond
            assert {c.acc[k] // p for c in sub} >= set(range(j)) and all(c.acc[k] < j * p for c in sub), (label, k)
    for c in cases:
        P, ok = M.affine(c.acc)
        assert ok and (P is None) == (c.label in ("copy", "a_inf"))
    assert M.affine(M.acc_inf()) == (None, True) and M.is_inf(M.acc_inf())
