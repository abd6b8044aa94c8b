"""gm_plonk_verify_batch, gm_kzg_verify_batch / _folded and their keys on the device.

Every expected value and status comes from plonk_verify_model.py (integers, written
from verify.go), never from the code under test.  Valid proofs come from the
model's own prover (all three curves) and from the library's prover session
(BN254, BLS12-377), whose five rounds meet a verifier here for the first time.
"""
import ctypes
import random

import numpy as np
import pytest

import plonk_verify_model as pvm
import points_check_cases as pc
import pyref

pytestmark = pytest.mark.gpu

ERR_INVALID = -1
BAD_AT = (0, 31, 32, 63, 64)


def upload(gm_ctx, oracle, cname, vk, **over):
    import gnark_mi355x as gm
    d = pvm.vk_bytes(oracle, cname, vk)
    d.update(over)
    return gm.PlonkVk(gm_ctx, cname, d)


def run_batch(key, oracle, cname, proofs, per_chunk=None):
    st, ok = key.verify_batch(*pvm.batch_bytes(oracle, cname, proofs), per_chunk=per_chunk)
    assert ok == int((st == 0).sum())
    return st.tolist()


# ---------------------------------------------------------------------------
# 1. the scalars kernel against the model
# ---------------------------------------------------------------------------
SCALAR_CONFIGS = [(8, 0, 0), (8, 1, 2), (8, 2, 2), (1 << 20, 1, 0), (1 << 20, 70, 2), (1 << 27, 2, 0), (1 << 27, 70, 2)]


@pytest.mark.parametrize("cname", pvm.CURVES)
def test_scalars_against_the_model(gm_ctx, oracle, cname):
    c = pyref.CURVES[cname]
    r = c.r
    rng = random.Random(0xA100 + len(cname))
    for n, nbp, nb in SCALAR_CONFIGS:
        rows = [nbp + 1 + 2 * j for j in range(nb)]
        dl = {k: 2 + i for i, k in enumerate(pvm.KEY_POINTS)}
        dl["qcp"] = [20 + j for j in range(nb)]
        vk = pvm.types.SimpleNamespace(n=n, nb_public=nbp, rows=rows, dl=dl, tau=5)
        w = pyref.domain_generator(c, n)
        rnd = lambda k: [rng.randrange(r) for _ in range(k)]
        fresh = lambda: dict(values=rnd(7 + nb), publics=rnd(nbp), hashed=rnd(nb), chal=rnd(6))
        cases = [fresh() for _ in range(3)]
        zetas = [1, w] + ([pow(w, nbp - 1, r)] if nbp else []) + ([pow(w, rows[-1], r)] if nb else [])
        for ze in zetas:  # the zero-denominator paths
            p = fresh()
            p["chal"][3] = ze
            cases.append(p)
        p = fresh()
        p["chal"][2] = 0  # alpha = 0
        cases.append(p)
        cases.append(dict(values=[r - 1] * (7 + nb), publics=[r - 1] * nbp, hashed=[r - 1] * nb, chal=[r - 1] * 6))
        for field in ("values", "publics", "hashed", "chal"):  # one word string >= r in each array
            p = fresh()
            if p[field]:
                p[field][rng.randrange(len(p[field]))] = rng.choice([r, r + 1, (1 << 256) - 1])
                cases.append(p)
        p = fresh()
        p["chal"][5] = 0  # u = 0
        cases.append(p)
        cases.append(fresh())
        want = [pvm.scalars(c, vk, p["values"], p["publics"], p["hashed"], p["chal"]) for p in cases]
        key = upload(gm_ctx, oracle, cname, vk)
        try:
            scal, aux, cls = key.test_scalars(b"".join(pvm.enc_raw(c, p["values"]) for p in cases),
                                              b"".join(pvm.enc_raw(c, p["publics"]) for p in cases),
                                              b"".join(pvm.enc_raw(c, p["hashed"]) for p in cases),
                                              b"".join(pvm.enc_raw(c, p["chal"]) for p in cases))
        finally:
            key.free()
        T = 18 + 2 * nb
        assert cls.tolist() == [x[3] for x in want], (n, nbp, nb)
        assert pvm.BAD_INPUT in cls.tolist() and pvm.ALGEBRAIC in cls.tolist()
        for i, (sc, pi, cl, st) in enumerate(want):
            if st == pvm.BAD_INPUT:
                continue
            assert pvm.dec(c, aux[64 * i:64 * i + 64]) == [pi, cl], (n, nbp, nb, i)
            assert pvm.dec(c, scal[32 * T * i:32 * T * (i + 1)]) == sc, (n, nbp, nb, i)
        # constLin = claimed lin is OK: the class of a proof whose first value is the model's constLin
        good = dict(cases[0])
        good["values"] = [want[0][2]] + good["values"][1:]
        assert pvm.scalars(c, vk, good["values"], good["publics"], good["hashed"], good["chal"])[3] == pvm.OK
        key = upload(gm_ctx, oracle, cname, vk)
        try:
            _, _, cls = key.test_scalars(pvm.enc(c, good["values"]), pvm.enc(c, good["publics"]),
                                         pvm.enc(c, good["hashed"]), pvm.enc(c, good["chal"]))
        finally:
            key.free()
        assert cls.tolist() == [pvm.OK]


# ---------------------------------------------------------------------------
# 2. the model prover's proofs are accepted
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("nb", [0, 2])
@pytest.mark.parametrize("n", [8, 64])
@pytest.mark.parametrize("cname", pvm.CURVES)
def test_model_prover_proofs_accepted(gm_ctx, oracle, cname, n, nb):
    c = pyref.CURVES[cname]
    _, vk, proof = pvm.case(cname, n, nb)
    assert pvm.verify(c, vk, proof) == pvm.OK
    key = upload(gm_ctx, oracle, cname, vk)
    try:
        assert run_batch(key, oracle, cname, [proof]) == [pvm.OK]
        other = pvm.clone(proof, chal=proof.chal[:5] + [0xC0FFEE])  # any non-zero u
        assert run_batch(key, oracle, cname, [proof, other, proof]) == [pvm.OK] * 3
    finally:
        key.free()


# ---------------------------------------------------------------------------
# 3. the library's prover session meets a verifier
# ---------------------------------------------------------------------------
def group_verify(c, vkb, nb, pts, sc, tau):
    """The model verifier's pairing part on points: A = [tau] B in the group."""
    G = pyref.Group(c, False)
    P = lambda b: pyref.decode_point(c, b, False)
    pb = len(vkb["ql"])
    key = [G.generator()] + [P(vkb[k]) for k in ("ql", "qr", "qm", "qo", "s3", "s1", "s2")] + \
          [P(vkb["qcp"][j * pb:(j + 1) * pb]) for j in range(nb)]
    bases = key + pts + [pts[8]]
    A = P(vkb["qk"])
    for s, b in zip(sc[:-1], bases[:-1]):
        A = G.add(A, G.mul(b, s))
    B = G.add(pts[7], G.mul(pts[8], sc[-1]))
    return A == G.mul(B, tau)


def session_proof(gm_ctx, oracle, sess, cname, inst, h_rand, lin_key_qk):
    """(points, values, challenges) of one proof by the session, in the verifier's order."""
    c = inst.c
    key = sess.make_key(gm_ctx, oracle, cname, inst, lin_key_qk=lin_key_qk)
    try:
        out = sess.run_proof(key, inst, h_rand)
    finally:
        key.free()
    ch = sess.challenge
    beta = ch(c, "beta", inst.salt, *out["bsb"], *out["lro"])
    gamma = ch(c, "gamma", inst.salt, *out["bsb"], *out["lro"])
    alpha = ch(c, "alpha", out["z"])
    zeta = ch(c, "zeta", *out["h"])
    v = ch(c, "kzg", out["lin"], *out["claimed"], out["z_shifted"], out["z_open"])
    points = out["lro"] + [out["z"]] + out["h"] + [out["batch"], out["z_open"]] + out["bsb"]
    values = pvm.dec(c, b"".join(out["claimed"]) + out["z_shifted"])
    return points, values, [gamma, beta, alpha, zeta, v, 0xABCDEF]


@pytest.mark.parametrize("h_rand", [False, True])
@pytest.mark.parametrize("nb", [0, 2])
@pytest.mark.parametrize("n", [8, 64])
@pytest.mark.parametrize("cname", ["bn254", "bls12377"])
def test_gpu_prover_proofs_accepted(gm_ctx, oracle, cname, n, nb, h_rand):
    """The satisfying instance of the model prover through gm_plonk_pk_upload and the
    five session rounds, the challenges chained by SHA-256 as in
    test_plonk_session_gpu.py; the proof must be accepted by the device verifier and
    by the model verifier (scalars in integers, the pairing equation in the group).

    The key is uploaded with GM_PLONK_PK_LIN_KEY_QK.  The first run of this test, on
    a key without it, failed in all sixteen cases: device and model both answered
    ALGEBRAIC with claimed_0 - constLin = PI(zeta) exactly, because round 4 built the
    linearised polynomial from the completed Qk where gnark's
    innerComputeLinearizedPoly reads the key's trace.Qk.  The flag makes round 4 do
    what gnark does; the next test pins what a key without it produces.
    """
    import test_plonk_session_gpu as sess
    c = pyref.CURVES[cname]
    inst, vk, _ = pvm.case(cname, n, nb)
    points, values, chal = session_proof(gm_ctx, oracle, sess, cname, inst, h_rand, True)
    sc, pi, const_lin, cls = pvm.scalars(c, vk, values, inst.public, inst.cvals, chal)
    print("claimed lin - constLin =", (values[0] - const_lin) % c.r, " PI(zeta) =", pi, " model class", cls)
    vkb = pvm.vk_bytes(oracle, cname, vk)
    model_ok = cls == pvm.OK and group_verify(c, vkb, nb, [pyref.decode_point(c, b, False) for b in points], sc,
                                              vk.tau)
    vkey = upload(gm_ctx, oracle, cname, vk)
    try:
        st, ok = vkey.verify_batch(b"".join(points), pvm.enc(c, values), pvm.enc(c, inst.public),
                                   pvm.enc(c, inst.cvals), pvm.enc(c, chal))
    finally:
        vkey.free()
    print("device status", st.tolist())
    assert model_ok, "the model verifier rejects the session's proof: class %d" % cls
    assert st.tolist() == [pvm.OK] and ok == 1


@pytest.mark.parametrize("h_rand", [False, True])
@pytest.mark.parametrize("nb", [0, 2])
@pytest.mark.parametrize("n", [8, 64])
@pytest.mark.parametrize("cname", ["bn254", "bls12377"])
def test_session_without_the_flag_keeps_the_completed_qk(gm_ctx, oracle, cname, n, nb, h_rand):
    """A key uploaded without GM_PLONK_PK_LIN_KEY_QK: the session's earlier bytes.
    Against the real key those proofs are ALGEBRAIC for device and model alike, off by
    PI(zeta) exactly; against a key whose Qk digest is the commitment of the completed
    Qk, with zero public inputs and zero hashed commitments (so PI(zeta) = 0), device
    and model accept them, and a changed claimed value is still refused: the five
    rounds are consistent, and the Qk of the linearised polynomial is the whole
    difference."""
    import test_plonk_session_gpu as sess
    c = pyref.CURVES[cname]
    r = c.r
    inst, vk, _ = pvm.case(cname, n, nb)
    dl = dict(vk.dl, qk=pvm.horner(r, pvm.canon(c, inst.qk_full), vk.tau))
    vk2 = pvm.types.SimpleNamespace(n=vk.n, nb_public=vk.nb_public, rows=vk.rows, dl=dl, tau=vk.tau)
    points, values, chal = session_proof(gm_ctx, oracle, sess, cname, inst, h_rand, False)
    _, pi, const_lin, cls = pvm.scalars(c, vk, values, inst.public, inst.cvals, chal)
    assert cls == pvm.ALGEBRAIC and pi != 0 and (values[0] - const_lin) % r == pi
    vkey = upload(gm_ctx, oracle, cname, vk)
    try:
        st, ok = vkey.verify_batch(b"".join(points), pvm.enc(c, values), pvm.enc(c, inst.public),
                                   pvm.enc(c, inst.cvals), pvm.enc(c, chal))
    finally:
        vkey.free()
    assert st.tolist() == [pvm.ALGEBRAIC] and ok == 0
    zeros, zc = [0] * inst.nb_public, [0] * nb
    sc, pi, const_lin, cls = pvm.scalars(c, vk2, values, zeros, zc, chal)
    assert pi == 0 and cls == pvm.OK
    vkb = pvm.vk_bytes(oracle, cname, vk2)
    assert group_verify(c, vkb, nb, [pyref.decode_point(c, b, False) for b in points], sc, vk2.tau)
    worse = list(values)
    worse[1] = (worse[1] + 1) % r
    vkey = upload(gm_ctx, oracle, cname, vk2)
    try:
        st, ok = vkey.verify_batch(b"".join(points) * 2, pvm.enc(c, values + worse), pvm.enc(c, zeros * 2),
                                   pvm.enc(c, zc * 2), pvm.enc(c, chal * 2))
    finally:
        vkey.free()
    assert st[0] == pvm.OK and st[1] in (pvm.ALGEBRAIC, pvm.MISMATCH) and ok == 1


@pytest.mark.parametrize("cname", ["bn254", "bls12377"])
def test_setup_prove_verify_end_to_end(gm_ctx, oracle, cname):
    """The flag through a setup entry (gm_plonk_pk_setup), and the library's own
    digests as the verifying key: setup, five rounds, verification, nothing from the
    model but the instance, the hashed commitments and the challenges' order."""
    import gnark_mi355x as gm
    import test_plonk_session_gpu as sess
    c = pyref.CURVES[cname]
    n, nb = 64, 2
    inst, vk, _ = pvm.case(cname, n, nb)
    _, can, _, _ = sess.srs(oracle, cname, n)
    key, dig, _ = gm.PlonkProvingKey.setup(gm_ctx, cname, n, inst.nb_public,
                                           {k: pvm.enc(c, inst.fixed[k]) for k in gm.PLONK_SETUP_POLYS}, inst.sigma,
                                           [pvm.enc(c, f) for f in inst.qcp], list(inst.rows), can, lin_key_qk=True)
    try:
        out = sess.run_proof(key, inst, True)
    finally:
        key.free()
    d = [bytes(x) for x in dig]
    assert len(d) == 8 + nb
    vkd = dict(zip(("s1", "s2", "s3", "ql", "qr", "qm", "qo", "qk"), d[:8]), qcp=b"".join(d[8:]), n=n,
               nb_public=inst.nb_public, commitment_row=list(inst.rows), kzg_g1=gm.generator(cname),
               kzg_g2_0=gm.generator(cname, True), kzg_g2_1=pvm.g2_tau(cname, vk.tau))
    want = pvm.vk_bytes(oracle, cname, vk)
    assert all(vkd[k] == want[k] for k in pvm.KEY_POINTS + ("qcp",))  # the setup's digests are the model's
    ch = sess.challenge
    chal = [ch(c, "gamma", inst.salt, *out["bsb"], *out["lro"]), ch(c, "beta", inst.salt, *out["bsb"], *out["lro"]),
            ch(c, "alpha", out["z"]), ch(c, "zeta", *out["h"]),
            ch(c, "kzg", out["lin"], *out["claimed"], out["z_shifted"], out["z_open"]), 0x5EED]
    points = out["lro"] + [out["z"]] + out["h"] + [out["batch"], out["z_open"]] + out["bsb"]
    vkey = gm.PlonkVk(gm_ctx, cname, vkd)
    try:
        st, ok = vkey.verify_batch(b"".join(points), b"".join(out["claimed"]) + out["z_shifted"],
                                   pvm.enc(c, inst.public), pvm.enc(c, inst.cvals), pvm.enc(c, chal))
    finally:
        vkey.free()
    assert st.tolist() == [pvm.OK] and ok == 1


# ---------------------------------------------------------------------------
# 4. every kind of bad proof gets its own class and leaves its neighbours alone
# ---------------------------------------------------------------------------
def bad_point_bytes(cname):
    c = pc.params(cname)
    out = {}
    for name, raw, cls in pc.cases(cname, False):
        if cls != pc.OK and cls not in out:
            out[cls] = pc.raw_bytes(c, raw)
    return out


@pytest.mark.parametrize("cname", pvm.CURVES)
def test_bad_proofs_are_classed_and_leave_their_neighbours_alone(gm_ctx, oracle, cname):
    c = pyref.CURVES[cname]
    nb = 2
    _, vk, proof = pvm.case(cname, 8, nb)
    muts = [(name, p, pvm.verify(c, vk, p)) for name, p in pvm.mutations(c, vk, proof) if name != "bad point"]
    for k, (cls, b) in enumerate(sorted(bad_point_bytes(cname).items())):
        where = (3, 9 + 1, 7)[k % 3]  # Z, Bsb22[1], Hb
        muts.append(("bad point class %d at %d" % (cls, where), pvm.clone(proof, raw_points={where: b}), pvm.BAD_POINT))
    if cname != "bn254":  # BN254's G1 has cofactor 1
        assert pc.OFF_SUBGROUP in bad_point_bytes(cname)
    assert {pvm.MISMATCH, pvm.ALGEBRAIC, pvm.BAD_INPUT, pvm.BAD_POINT} <= {m[2] for m in muts}
    key = upload(gm_ctx, oracle, cname, vk)
    try:
        for b0 in range(0, len(muts), len(BAD_AT)):
            group = muts[b0:b0 + len(BAD_AT)]
            proofs, want = [proof] * 65, [pvm.OK] * 65
            for pos, (name, p, st) in zip(BAD_AT, group):
                proofs[pos], want[pos] = p, st
            got = run_batch(key, oracle, cname, proofs)
            assert got == want, [m[0] for m in group]
    finally:
        key.free()
    # a wrong key digest, each of the eight and each Qcp: every proof mismatches
    arrays = pvm.batch_bytes(oracle, cname, [proof] * 3)
    pb = len(pvm.to_points(oracle, cname, [1])[0])
    good_qcp = b"".join(pvm.to_points(oracle, cname, vk.dl["qcp"]))
    over = [{k: pvm.to_points(oracle, cname, [(vk.dl[k] + 1) % c.r])[0]} for k in pvm.KEY_POINTS]
    for j in range(nb):
        wrong = pvm.to_points(oracle, cname, [(vk.dl["qcp"][j] + 1) % c.r])[0]
        over.append({"qcp": good_qcp[:j * pb] + wrong + good_qcp[(j + 1) * pb:]})
    for o in over:
        key = upload(gm_ctx, oracle, cname, vk, **o)
        try:
            st, ok = key.verify_batch(*arrays)
            assert st.tolist() == [pvm.MISMATCH] * 3 and ok == 0, list(o)
        finally:
            key.free()


# ---------------------------------------------------------------------------
# 5. chunk boundary
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("cname", pvm.CURVES)
def test_chunk_boundary(gm_ctx, oracle, cname):
    c = pyref.CURVES[cname]
    _, vk, proof = pvm.case(cname, 8, 2)
    muts = dict((name, p) for name, p in pvm.mutations(c, vk, proof))
    proofs = [proof, muts["value 0 + 1"], proof, muts["point 4 replaced"], muts["u = 0"]]
    want = [pvm.verify(c, vk, p) for p in proofs]
    assert want == [pvm.OK, pvm.ALGEBRAIC, pvm.OK, pvm.MISMATCH, pvm.BAD_INPUT]
    key = upload(gm_ctx, oracle, cname, vk)
    try:
        assert run_batch(key, oracle, cname, proofs) == want
        for per in (1, 2, 5):
            assert run_batch(key, oracle, cname, proofs, per_chunk=per) == want, per
    finally:
        key.free()


# ---------------------------------------------------------------------------
# 6. KZG
# ---------------------------------------------------------------------------
def kzg_key(gm_ctx, cname, tau):
    import gnark_mi355x as gm
    return gm.KzgVk(gm_ctx, cname, gm.generator(cname), gm.generator(cname, True), pvm.g2_tau(cname, tau))


def model_openings(c, tau, m, seed):
    """m valid openings in the exponent: (dl_c, dl_h, z, y, bad_point)."""
    rng = random.Random(seed)
    out = []
    for _ in range(m):
        dc, z, y = (rng.randrange(c.r) for _ in range(3))
        out.append((dc, (dc - y) * pow(tau - z, -1, c.r) % c.r, z, y, False))
    return out


def kzg_arrays(oracle, cname, ops, raw=None):
    c = pyref.CURVES[cname]
    pts = pvm.to_points(oracle, cname, [o[0] for o in ops] + [o[1] for o in ops])
    m = len(ops)
    for i, b in (raw or {}).items():
        pts[i] = b
    return b"".join(pts[:m]), b"".join(pts[m:]), pvm.enc_raw(c, [o[2] for o in ops]), pvm.enc_raw(c, [o[3] for o in ops])


@pytest.mark.parametrize("m", [1, 2, 65])
@pytest.mark.parametrize("cname", pvm.CURVES)
def test_kzg_model_openings(gm_ctx, oracle, cname, m):
    c = pyref.CURVES[cname]
    r, tau = c.r, 0x5EED5EED5EED5EED5EED5EED5EED5EED5EED5EED
    ops = model_openings(c, tau, m, 0xB200 + m)
    raw = {}
    edits = {0: "y+1"} if m == 1 else ({0: "z+1", 1: "inf"} if m == 2 else
                                       {0: "y+1", 31: "z+1", 32: "swap", 63: "inf", 64: "bad", 5: "y>=r"})
    for i, kind in edits.items():
        dc, dh, z, y, _ = ops[i]
        if kind == "y+1":
            ops[i] = (dc, dh, z, (y + 1) % r, False)
        elif kind == "z+1":
            ops[i] = (dc, dh, (z + 1) % r, y, False)
        elif kind == "swap":
            ops[i] = (dc, ops[i - 1][1], z, y, False)
        elif kind == "inf":
            ops[i] = (0, 0, z, 0, False)  # C at infinity, y = 0: H is the infinity too, and it verifies
        elif kind == "bad":
            ops[i] = (dc, dh, z, y, True)
            raw[m + i] = sorted(bad_point_bytes(cname).items())[-1][1]  # H
        elif kind == "y>=r":
            ops[i] = (dc, dh, z, r + 3, False)
    want = [pvm.kzg_verify(c, tau, *o) for o in ops]
    key = kzg_key(gm_ctx, cname, tau)
    try:
        st, ok = key.verify_batch(*kzg_arrays(oracle, cname, ops, raw))
        assert st.tolist() == want and ok == want.count(pvm.OK)
        if m == 65:
            assert set(want) == {pvm.OK, pvm.MISMATCH, pvm.BAD_POINT, pvm.BAD_INPUT} and want[63] == pvm.OK
    finally:
        key.free()


@pytest.mark.parametrize("cname", pvm.CURVES)
def test_kzg_folded(gm_ctx, oracle, cname):
    c = pyref.CURVES[cname]
    r, tau = c.r, 0x1234567890ABCDEF1234567
    m = 37
    good = model_openings(c, tau, m, 0xB300)
    bad = list(good)
    bad[20] = bad[20][:3] + ((bad[20][3] + 1) % r, False)
    rng = random.Random(0xB301)
    key = kzg_key(gm_ctx, cname, tau)
    try:
        for _ in range(2):
            lam = [rng.randrange(1, r) for _ in range(m)]
            for ops in (good, bad):
                want = pvm.kzg_verify_folded(c, tau, ops, lam)
                assert want == (pvm.OK if ops is good else pvm.MISMATCH)
                assert key.verify_folded(*kzg_arrays(oracle, cname, ops), pvm.enc(c, lam)) == want
        lam = [0] + [rng.randrange(1, r) for _ in range(m - 1)]   # lambda_0 is not read
        assert key.verify_folded(*kzg_arrays(oracle, cname, good), pvm.enc(c, lam)) == pvm.OK
        lam[7] = 0
        assert key.verify_folded(*kzg_arrays(oracle, cname, good), pvm.enc(c, lam)) == pvm.BAD_INPUT
        assert key.verify_folded(*kzg_arrays(oracle, cname, good[:1]), pvm.enc(c, [5])) == pvm.OK
        assert key.verify_folded(*kzg_arrays(oracle, cname, bad[20:21]), pvm.enc(c, [5])) == pvm.MISMATCH
    finally:
        key.free()


@pytest.mark.parametrize("cname", pvm.CURVES)
def test_kzg_chunk_boundaries(gm_ctx, oracle, cname):
    """The chunk loops through the hook: per opening at 1, 2 and 5 per chunk, and the
    folded form's carry across chunks -- a bad opening in the first chunk, in a later
    one, lambda = 0 and a bad point in a later chunk, and a batch whose chunk sums
    take three levels of the 16-way sum (301 -> 19 -> 2 -> 1)."""
    c = pyref.CURVES[cname]
    r, tau = c.r, 0xABCDEF0123456789ABCDEF
    rng = random.Random(0xB600)
    key = kzg_key(gm_ctx, cname, tau)
    try:
        ops = model_openings(c, tau, 5, 0xB601)
        ops[1] = ops[1][:3] + ((ops[1][3] + 1) % r, False)
        ops[4] = ops[4][:2] + (r + 1,) + ops[4][3:]
        want = [pvm.kzg_verify(c, tau, *o) for o in ops]
        assert want == [pvm.OK, pvm.MISMATCH, pvm.OK, pvm.OK, pvm.BAD_INPUT]
        arrays = kzg_arrays(oracle, cname, ops)
        assert key.verify_batch(*arrays)[0].tolist() == want
        for per in (1, 2, 5):
            st, ok = key.verify_batch(*arrays, per_chunk=per)
            assert st.tolist() == want and ok == 3, per
        # folded, two openings per chunk over 37 openings (19 chunks)
        m = 37
        good = model_openings(c, tau, m, 0xB602)
        lam = [rng.randrange(1, r) for _ in range(m)]
        spoil = lambda ops, i: ops[:i] + [ops[i][:3] + ((ops[i][3] + 1) % r, False)] + ops[i + 1:]
        bad_pt = sorted(bad_point_bytes(cname).items())[-1][1]
        cases = [("good", good, lam, None), ("bad opening in chunk 0", spoil(good, 1), lam, None),
                 ("bad opening in chunk 9", spoil(good, 19), lam, None), ("bad opening last", spoil(good, 36), lam, None),
                 ("lambda 0 in chunk 5", good, lam[:11] + [0] + lam[12:], None),
                 ("bad point in chunk 12", good[:25] + [good[25][:4] + (True,)] + good[26:], lam, {25: bad_pt}),
                 ("lambda 0 in chunk 1, bad point in chunk 12", good[:25] + [good[25][:4] + (True,)] + good[26:],
                  lam[:2] + [0] + lam[3:], {25: bad_pt})]
        for name, ops, lm, raw in cases:
            want = pvm.kzg_verify_folded(c, tau, ops, lm)
            arrays = kzg_arrays(oracle, cname, ops, raw) + (pvm.enc(c, lm),)
            assert key.verify_folded(*arrays) == want, name
            for per in (2, 7, 37):
                assert key.verify_folded(*arrays, per_chunk=per) == want, (name, per)
        assert [pvm.kzg_verify_folded(c, tau, x[1], x[2]) for x in cases] == \
            [pvm.OK, pvm.MISMATCH, pvm.MISMATCH, pvm.MISMATCH, pvm.BAD_INPUT, pvm.BAD_POINT, pvm.BAD_POINT]
        # three levels of the sum kernel in a chunk, and a carry on top
        m = 600
        big = model_openings(c, tau, m, 0xB603)
        lam = [rng.randrange(1, r) for _ in range(m)]
        for name, ops in (("good", big), ("bad in chunk 0", spoil(big, 5)), ("bad in chunk 1", spoil(big, 450))):
            want = pvm.kzg_verify_folded(c, tau, ops, lam)
            assert want == (pvm.OK if name == "good" else pvm.MISMATCH)
            assert key.verify_folded(*kzg_arrays(oracle, cname, ops), pvm.enc(c, lam), per_chunk=300) == want, name
    finally:
        key.free()


@pytest.mark.parametrize("cname", pvm.CURVES)
def test_kzg_openings_of_the_library_and_the_hand_built_check(gm_ctx, oracle, cname):
    """Openings made by gm_kzg_open; the hand-built pairing check of
    test_pairing_gpu.py::test_kzg_opening_verifies_through_pairing_check agrees."""
    c = pyref.CURVES[cname]
    G1, G2 = pyref.Group(c, False), pyref.Group(c, True)
    r, n, tau = c.r, 16, 0x5EED5EED5EED5EED5EED5EED5EED5EED5EED5EED
    rng = random.Random(0xB400)
    srs = b"".join(pvm.to_points(oracle, cname, [pow(tau, i, r) for i in range(n)]))
    coeffs = [rng.randrange(r) for _ in range(n)]
    z = rng.randrange(r)
    S = gm_ctx.points_upload(cname, srs)
    F = gm_ctx.copy_to_device(pvm.enc(c, coeffs))
    try:
        commit = gm_ctx.kzg_commit(cname, S, pvm.enc(c, coeffs))
        val, h = gm_ctx.kzg_open(cname, S, F, pvm.enc(c, [z]))
    finally:
        S.free()
        F.free()
    (y,) = pvm.dec(c, val)
    assert y == sum(co * pow(z, i, r) for i, co in enumerate(coeffs)) % r
    Cp, H = pyref.decode_point(c, commit, False), pyref.decode_point(c, h, False)
    encp = lambda pts, g2: b"".join(pyref.encode_point(c, P, g2) for P in pts)

    def hand(claim):
        lhs = G1.add(G1.add(Cp, G1.neg(G1.mul(c.g1, claim))), G1.mul(H, z))
        return gm_ctx.pairing_check(cname, encp([lhs, G1.neg(H)], False), encp([c.g2, G2.mul(c.g2, tau)], True), 2)

    # 65 openings of the same polynomial by the library, then the issue's edits
    zs = [rng.randrange(r) for _ in range(65)]
    S = gm_ctx.points_upload(cname, srs)
    F = gm_ctx.copy_to_device(pvm.enc(c, coeffs))
    try:
        opened = [gm_ctx.kzg_open(cname, S, F, pvm.enc(c, [zi])) for zi in zs]
    finally:
        S.free()
        F.free()
    ys = [pvm.dec(c, o[0])[0] for o in opened]
    assert all(yi == sum(co * pow(zi, i, r) for i, co in enumerate(coeffs)) % r for yi, zi in zip(ys, zs))
    ftau = sum(co * pow(tau, i, r) for i, co in enumerate(coeffs)) % r
    assert pvm.to_points(oracle, cname, [ftau])[0] == bytes(commit)  # the model's footing for the expectations
    pb = len(bytes(commit))
    inf = bytes(pb)
    bad_pt = sorted(bad_point_bytes(cname).items())[0][1]
    key = kzg_key(gm_ctx, cname, tau)
    try:
        st, ok = key.verify_batch(commit * 3, h * 3, pvm.enc(c, [z, z, (z + 1) % r]), pvm.enc(c, [y, (y + 1) % r, y]))
        assert st.tolist() == [pvm.OK, pvm.MISMATCH, pvm.MISMATCH] and ok == 1
        assert hand(y).tolist() == [1] and hand((y + 1) % r).tolist() == [0]
        for m, edits in ((1, {}), (1, {0: "y+1"}), (2, {0: "z+1", 1: "inf"}),
                         (65, {0: "y+1", 31: "z+1", 32: "swap", 63: "inf", 64: "bad"})):
            C = [bytes(commit)] * m
            H = [bytes(o[1]) for o in opened[:m]]
            Z, Y, want = list(zs[:m]), list(ys[:m]), [pvm.OK] * m
            for i, kind in edits.items():
                want[i] = pvm.MISMATCH
                if kind == "y+1":
                    Y[i] = (Y[i] + 1) % r
                elif kind == "z+1":
                    Z[i] = (Z[i] + 1) % r
                elif kind == "swap":
                    H[i] = bytes(opened[i - 1][1])
                elif kind == "inf":  # the zero polynomial: C and H at infinity, y = 0
                    C[i], H[i], Y[i], want[i] = inf, inf, 0, pvm.OK
                elif kind == "bad":
                    C[i], want[i] = bad_pt, pvm.BAD_POINT
            st, ok = key.verify_batch(b"".join(C), b"".join(H), pvm.enc(c, Z), pvm.enc(c, Y))
            assert st.tolist() == want and ok == want.count(pvm.OK), (m, edits)
    finally:
        key.free()


# ---------------------------------------------------------------------------
# 7. refusals leave the context usable
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("cname", pvm.CURVES)
def test_refusals_leave_the_context_usable(gm_ctx, oracle, cname):
    import gnark_mi355x as gm
    L = gm.load_library()
    c = pyref.CURVES[cname]
    _, vk, proof = pvm.case(cname, 8, 2)
    vkb = pvm.vk_bytes(oracle, cname, vk)
    err = lambda: L.gm_last_error().decode()
    h = gm_ctx.handle
    key = upload(gm_ctx, oracle, cname, vk)
    arrays = pvm.batch_bytes(oracle, cname, [proof])
    right = lambda: key.verify_batch(*arrays)[0].tolist() == [pvm.OK]

    def refused(what, **over):
        with pytest.raises(gm.GmError) as e:
            gm.PlonkVk(gm_ctx, cname, dict(vkb, **over)).free()
        assert "error -1" in str(e.value) and what in str(e.value), str(e.value)
        assert right()

    try:
        assert right()
        refused("power of two", n=12)
        refused("power of two", n=4)
        refused("commitment_row[1]", commitment_row=[3, 8])
        refused("nb_public", nb_public=9)
        bad = sorted(bad_point_bytes(cname).items())[0]
        refused("qm fails the point check", qm=bad[1])
        refused("qcp[1] fails the point check", qcp=vkb["qcp"][:len(bad[1])] + bad[1])
        refused("kzg_g2_1 fails the point check", kzg_g2_1=bytes(range(1, 1 + 4 * len(bad[1]) // 2)))
        out = ctypes.c_void_p()
        assert L.gm_plonk_vk_upload(h, 9, None, ctypes.byref(out)) == ERR_INVALID and "unknown curve id" in err()
        assert right()
        # NULL arguments
        assert L.gm_plonk_vk_upload(h, gm.curve_id(cname), None, ctypes.byref(out)) == ERR_INVALID and right()
        assert L.gm_plonk_vk_upload(None, gm.curve_id(cname), None, None) == ERR_INVALID
        keep, host, m = key._proofs(*arrays)
        st = np.full(4, 0xEE, np.uint8)
        p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
        nb_ok = ctypes.c_size_t(99)
        assert L.gm_plonk_verify_batch(h, key.handle, None, 0, p(st), ctypes.byref(nb_ok)) == 0 and nb_ok.value == 0
        assert L.gm_plonk_verify_batch(h, key.handle, None, 1, p(st), None) == ERR_INVALID and right()
        assert L.gm_plonk_verify_batch(h, key.handle, ctypes.byref(host), 1, None, None) == ERR_INVALID and right()
        assert L.gm_plonk_verify_batch(h, None, ctypes.byref(host), 1, p(st), None) == ERR_INVALID and right()
        host.challenges = None
        assert L.gm_plonk_verify_batch(h, key.handle, ctypes.byref(host), 1, p(st), None) == ERR_INVALID and right()
        assert st.tolist() == [0xEE] * 4
        # a key of another context
        with gm.Context(0) as other:
            keep, host, m = key._proofs(*arrays)
            assert L.gm_plonk_verify_batch(other.handle, key.handle, ctypes.byref(host), 1, p(st), None) == ERR_INVALID
            assert "another context" in err()
            assert L.gm_plonk_vk_free(other.handle, key.handle) == ERR_INVALID
        assert right()
        # KZG: the same
        tau = vk.tau
        kk = kzg_key(gm_ctx, cname, tau)
        try:
            ops = model_openings(c, tau, 2, 0xB500)
            kright = lambda: kk.verify_batch(*kzg_arrays(oracle, cname, ops))[0].tolist() == [pvm.OK] * 2
            assert kright()
            with pytest.raises(gm.GmError) as e:
                gm.KzgVk(gm_ctx, cname, bad[1], gm.generator(cname, True), pvm.g2_tau(cname, tau))
            assert "g1 fails the point check" in str(e.value) and kright()
            assert L.gm_kzg_verify_batch(h, kk.handle, None, 0, p(st), None) == 0
            assert L.gm_kzg_verify_batch(h, kk.handle, None, 1, p(st), None) == ERR_INVALID and kright()
            assert L.gm_kzg_verify_folded(h, kk.handle, None, 1, p(st)) == ERR_INVALID and kright()
            assert L.gm_kzg_vk_upload(h, 9, None, ctypes.byref(out)) == ERR_INVALID and "unknown curve id" in err()
            assert st.tolist() == [0xEE] * 4
        finally:
            kk.free()
    finally:
        key.free()
