"""The device pairing layer by layer (csrc/pairing_impl.hpp): the tower against
the integer model, Miller loop + final exponentiation against the model's
pairing, gm_pairing_check against discrete logarithms alone, batched Groth16
verification of GPU-made proofs under the oracle's setup, the twelve external
bellman vectors on BLS12-381, one KZG opening, and the refusals."""
import ctypes
import random

import numpy as np
import pytest

import pyref
import pairing_model as pm
import points_check_cases as pc

pytestmark = pytest.mark.gpu
CURVES = ("bn254", "bls12377", "bls12381")
ERR_INVALID = -1
N_TOWER = 70  # one wave and a tail


def enc_points(c, pts, g2):
    return b"".join(pyref.encode_point(c, P, g2) for P in pts)


# ---- 1. tower operations ---------------------------------------------------------------
def tower_elements(m, rng):
    """0, 1, elements of Fp, Fp2 and Fp6 (C1 = 0), then random ones."""
    z = (0, 0)
    rnd2 = lambda: (rng.randrange(m.p), rng.randrange(m.p))
    out = [m.zero(), m.one(), m.from_fp(rng.randrange(m.p)), m.from_fp(m.p - 1),
           [rnd2(), z, z, z, z, z], [rnd2(), z, rnd2(), z, rnd2(), z], [rnd2(), z, rnd2(), z, rnd2(), z]]
    while len(out) < N_TOWER:
        out.append([rnd2() for _ in range(6)])
    return out


def sparse_line(m, y):
    """The element gm_test_pairing_op's LINE_MUL reads from y: its three line slots."""
    keep = (0, 2, 3) if m.m_twist else (0, 1, 3)
    return [x if i in keep else (0, 0) for i, x in enumerate(y)]


@pytest.mark.parametrize("name", CURVES)
def test_tower_ops_against_the_model(gm_ctx, name):
    import gnark_mi355x as gm
    m = pm.model(name)
    rng = random.Random(0x70E + len(name))
    a = tower_elements(m, rng)
    b = a[::-1]
    b[3] = [(rng.randrange(m.p), rng.randrange(m.p)) for _ in range(6)]
    enc = lambda xs: b"".join(m.encode(x) for x in xs)
    ab, bb = enc(a), enc(b)
    eb = len(ab) // N_TOWER

    def run(op, x, y=None):
        got = gm_ctx.test_pairing_op(name, op, x, y, N_TOWER)
        return [m.decode(got[i * eb:(i + 1) * eb]) for i in range(N_TOWER)]
    assert run(gm.TPAIR_MUL, ab, bb) == [m.mul(x, y) for x, y in zip(a, b)]
    assert run(gm.TPAIR_SQR, ab) == [m.sqr(x) for x in a]
    assert run(gm.TPAIR_INV, ab) == [m.inv(x) for x in a]          # inv(0) = 0
    assert run(gm.TPAIR_CONJ, ab) == [m.conj(x) for x in a]
    assert run(gm.TPAIR_FROB1, ab) == [m.frob(x, 1) for x in a]
    assert run(gm.TPAIR_FROB2, ab) == [m.frob(x, 2) for x in a]
    assert run(gm.TPAIR_LINE_MUL, ab, bb) == [m.mul(x, sparse_line(m, y)) for x, y in zip(a, b)]
    # easy-part outputs: x^((p^6 - 1)(p^2 + 1)) lies in the cyclotomic subgroup
    easy = []
    for x in a:
        if x == m.zero():
            x = m.one()
        e = m.mul(m.conj(x), m.inv(x))
        easy.append(m.mul(m.frob(e, 2), e))
    eb_ = enc(easy)
    assert run(gm.TPAIR_CYC_SQR, eb_) == [m.sqr(x) for x in easy]
    assert run(gm.TPAIR_EXP_U, eb_) == [m.pow(x, abs(m.u)) for x in easy]


# ---- 2. Miller loop and final exponentiation -----------------------------------------------
@pytest.mark.parametrize("name", CURVES)
def test_pairing_value_against_the_model(gm_ctx, name):
    import gnark_mi355x as gm
    m = pm.model(name)
    c = m.c
    rng = random.Random(0x2A1 + len(name))
    g1, g2 = m.G1.generator(), m.G2.generator()
    logs = [(1, 1)] + [(rng.randrange(1, m.r), rng.randrange(1, m.r)) for _ in range(4)]
    P = [m.G1.mul(g1, x) for x, _ in logs] + [None, g1, None]
    Q = [m.G2.mul(g2, y) for _, y in logs] + [g2, None, None]
    n = len(P)
    f = gm_ctx.test_pairing_op(name, gm.TPAIR_MILLER, enc_points(c, P, False), enc_points(c, Q, True), n)
    eb = len(f) // n
    assert [m.decode(f[i * eb:(i + 1) * eb]) for i in range(5, 8)] == [m.one()] * 3
    got = gm_ctx.test_pairing_op(name, gm.TPAIR_FINAL_EXP, f, None, n)
    got = [m.decode(got[i * eb:(i + 1) * eb]) for i in range(n)]
    e = m.pair(g1, g2)
    assert not m.is_one(e)
    for i, (x, y) in enumerate(logs):
        assert got[i] == m.pair(P[i], Q[i]), (name, i)
        assert got[i] == m.pow(e, x * y % m.r), (name, i)
    assert got[5:] == [m.one()] * 3


# ---- 3. gm_pairing_check: the truth from discrete logarithms alone --------------------------
POOL = 16


class Pool:
    """[a]G1 for -16 <= a <= 16 and [b]G2 for 1 <= b <= 16 as gnark bytes; a pair
    is (a, b), with a = 0 or b = 0 standing for the point at infinity."""

    def __init__(self, name):
        self.m = m = pm.model(name)
        c = m.c
        self.b1, self.b2 = {0: pyref.encode_point(c, None, False)}, {0: pyref.encode_point(c, None, True)}
        acc1 = acc2 = None
        for i in range(1, POOL + 1):
            acc1, acc2 = m.G1.add(acc1, m.G1.generator()), m.G2.add(acc2, m.G2.generator())
            self.b1[i], self.b1[-i] = pyref.encode_point(c, acc1, False), pyref.encode_point(c, m.G1.neg(acc1), False)
            self.b2[i] = pyref.encode_point(c, acc2, True)

    def big(self, a):
        """[a]G1 for a scalar outside the pool."""
        if a not in self.b1:
            self.b1[a] = pyref.encode_point(self.m.c, self.m.G1.mul(self.m.G1.generator(), a), False)
        return a

    def arrays(self, products):
        flat = [pr for prod in products for pr in prod]
        return b"".join(self.b1[a] for a, _ in flat), b"".join(self.b2[b] for _, b in flat)

    def truth(self, products):
        return [int(sum(a * b for a, b in prod) % self.m.r == 0) for prod in products]


def make_product(k, accept, rng):
    if k == 1:
        return [(0, 3)] if accept else [(1, 1)]
    pairs, rem = [], k
    if k % 2:
        pairs += [(1, 2), (1, 3), (-5, 1)]
        rem -= 3
    while rem:
        a, b = rng.randrange(1, POOL), rng.randrange(1, POOL + 1)
        pairs += [(a, b), (-a, b)]
        rem -= 2
    if not accept:
        i = next(i for i, (a, _) in enumerate(pairs) if 0 < a < POOL)
        pairs[i] = (pairs[i][0] + 1, pairs[i][1])
    rng.shuffle(pairs)
    return pairs


@pytest.fixture(scope="module")
def pools():
    return {name: Pool(name) for name in CURVES}


@pytest.mark.parametrize("name", CURVES)
def test_pairing_check_matrix(gm_ctx, pools, name):
    pool = pools[name]
    rng = random.Random(0x3C4 + len(name))
    for k in (1, 2, 4, 17, 300):          # one, one, one, two and three reduce turns (none for k = 1)
        for flags in ([1], [0], [0, 1, 0], [0] + [1] * 63 + [0]):
            products = [make_product(k, bool(f), rng) for f in flags]
            want = pool.truth(products)
            assert want == flags
            g1, g2 = pool.arrays(products)
            got = gm_ctx.pairing_check(name, g1, g2, k)
            assert got.tolist() == want, (name, k, len(flags))
            if len(flags) == 65 or k == 17:
                d1, d2 = gm_ctx.copy_to_device(g1), gm_ctx.copy_to_device(g2)
                try:
                    assert gm_ctx.pairing_check_device(name, d1, d2, len(flags), k).tolist() == want
                finally:
                    d1.free()
                    d2.free()


@pytest.mark.parametrize("name", CURVES)
def test_pairing_check_special_sums(gm_ctx, pools, name):
    pool = pools[name]
    r = pool.m.r
    products = [
        [(2, 3), (-6, 1), (0, 0), (0, 0)],                  # sum = 0, every term nonzero (and two infinity pairs)
        [(pool.big(r - 6), 1), (2, 3), (0, 5), (4, 0)],     # sum = r exactly; P = infinity, Q = infinity inside
        [(3, 1), (-2, 1), (0, 0), (0, 0)],                  # sum = 1
        [(5, 7), (-5, 7), (0, 0), (0, 0)],                  # e(P, Q) e(-P, Q)
        [(5, 7), (-5, 7), (1, 0), (0, 1)],                  # infinity pairs leave it at 1
        [(5, 7), (-5, 7), (1, 1), (0, 1)],                  # one more pair: sum = 1
    ]
    want = pool.truth(products)
    assert want == [1, 1, 0, 1, 1, 0]
    assert gm_ctx.pairing_check(name, *pool.arrays(products), 4).tolist() == want
    singles = [[(0, 0)], [(0, 4)], [(4, 0)], [(1, 1)], [(16, 16)], [(-3, 2)]]   # k = 1 accepts only an infinity pair
    assert gm_ctx.pairing_check(name, *pool.arrays(singles), 1).tolist() == [1, 1, 1, 0, 0, 0]


# ---- 4. batched Groth16 verification ----------------------------------------------------------
TOXIC = [0x1D5A2B3C4D5E6F708192A3B4C5D6E7F8091A2B3C4D5E6F708192A3B4C5D6E7F8,
         0x2E6B3C4D5E6F708192A3B4C5D6E7F8091A2B3C4D5E6F708192A3B4C5D6E7F8,
         0x3F7C4D5E6F708192A3B4C5D6E7F8091A2B3C4D5E6F708192A3B4C5D6E7F809,
         0x0A8D5E6F708192A3B4C5D6E7F8091A2B3C4D5E6F708192A3B4C5D6E7F8091A,
         0x1B9E6F708192A3B4C5D6E7F8091A2B3C4D5E6F708192A3B4C5D6E7F8091A2B]
CUBIC = [([(2, 1)], [(2, 1)], [(3, 1)]), ([(3, 1)], [(2, 1)], [(4, 1)]), ([(0, 1)], [(1, 1)], [(4, 1), (2, 1), (0, 5)])]
NB_WIRES, NB_PUBLIC = 5, 2


def cubic_witness(c, x):
    x %= c.r
    return [1, (x ** 3 + x + 5) % c.r, x, x * x % c.r, x ** 3 % c.r]


def vk_points(c, toxic):
    """The verifying key of the cubic circuit from the toxic scalars (setup.go:
    K[i] = (beta A_i(t) + alpha B_i(t) + C_i(t)) / gamma for the public wires)."""
    t, alpha, beta, gamma, delta = (x % c.r for x in toxic)
    r, n = c.r, 4
    w = pyref.domain_generator(c, n)
    A, B, C = [0] * NB_WIRES, [0] * NB_WIRES, [0] * NB_WIRES
    tn1, ninv = (pow(t, n, r) - 1) % r, pow(n, -1, r)
    for j, (L, Rr, O) in enumerate(CUBIC):
        wj = pow(w, j, r)
        lag = wj * tn1 * ninv * pow((t - wj) % r, -1, r) % r
        for row, acc in ((L, A), (Rr, B), (O, C)):
            for wi, co in row:
                acc[wi] = (acc[wi] + co * lag) % r
    G1, G2 = pyref.Group(c, False), pyref.Group(c, True)
    ginv = pow(gamma, -1, r)
    K = [(beta * A[i] + alpha * B[i] + C[i]) * ginv % r for i in range(NB_PUBLIC)]
    return dict(alpha_g1=G1.mul(c.g1, alpha), beta_g2=G2.mul(c.g2, beta), gamma_g2=G2.mul(c.g2, gamma),
                delta_g2=G2.mul(c.g2, delta), k=[G1.mul(c.g1, k) for k in K])


def vk_bytes(c, vk):
    return dict(alpha_g1=enc_points(c, [vk["alpha_g1"]], False), beta_g2=enc_points(c, [vk["beta_g2"]], True),
                gamma_g2=enc_points(c, [vk["gamma_g2"]], True), delta_g2=enc_points(c, [vk["delta_g2"]], True),
                k_g1=enc_points(c, vk["k"], False))


def pk_bytes(c, pk):
    out = {k: enc_points(c, [pk[k]], k.startswith("g2")) for k in ("g1_alpha", "g1_beta", "g1_delta", "g2_beta", "g2_delta")}
    for k in ("g1_A", "g1_B", "g1_Z", "g1_K", "g2_B"):
        out[k] = enc_points(c, pk[k], k.startswith("g2"))
    out["infA"] = np.array(pk["infA"], dtype=np.uint8)
    out["infB"] = np.array(pk["infB"], dtype=np.uint8)
    return out


def solve_abc(c, W):
    return tuple([sum(W[w] * co for w, co in row[k]) % c.r for row in CUBIC] for k in range(3))


@pytest.mark.parametrize("name", CURVES)
def test_g16_verify_batch(gm_ctx, name):
    import gnark_mi355x as gm
    c = pyref.CURVES[name]
    fr = lambda vals: b"".join(pyref.encode_fr(c, v) for v in vals)
    pk = pyref.g16_setup(c, CUBIC, NB_WIRES, NB_PUBLIC, TOXIC)
    vk = vk_points(c, TOXIC)
    xs = [3, 4, 11, c.r - 2, 0x1234567]
    dpk = gm.ProvingKey(gm_ctx, name, pk_bytes(c, pk), pk["n"], NB_WIRES, NB_PUBLIC)
    try:
        proofs = []
        for i, x in enumerate(xs):
            W = cubic_witness(c, x)
            a, b, cc = solve_abc(c, W)
            proofs.append((b"".join(dpk.prove(fr(W), fr(a), fr(b), fr(cc), fr([0xA11CE + i]), fr([c.r - 77 - i]))), W[1]))
    finally:
        dpk.free()
    W = cubic_witness(c, 3)
    oracle_proof = pyref.g16_prove(c, pk, W, *solve_abc(c, W), 12345, 67890)
    proofs.append((enc_points(c, [oracle_proof[0]], False) + enc_points(c, [oracle_proof[1]], True)
                   + enc_points(c, [oracle_proof[2]], False), W[1]))
    fpb = 8 * c.fp_limbs
    g1b, g2b = 2 * fpb, 4 * fpb
    ar_of, bs_of, krs_of = (lambda p: p[:g1b]), (lambda p: p[g1b:g1b + g2b]), (lambda p: p[g1b + g2b:])

    with pytest.raises(gm.GmError, match="gamma_g2.*subgroup"):
        bad = dict(vk, gamma_g2=pc.sub.random_curve_points(c, True, 1, 0x6A)[0])
        gm.VerifyingKey(gm_ctx, name, vk_bytes(c, bad))
    key = gm.VerifyingKey(gm_ctx, name, vk_bytes(c, vk))
    try:
        # every good proof, the oracle's own included
        st, ok = key.verify_batch(b"".join(p for p, _ in proofs), fr([y for _, y in proofs]))
        assert st.tolist() == [0] * len(proofs) and ok == len(proofs)
        st, ok = key.verify_batch(proofs[0][0], fr([proofs[0][1]]))              # m = 1
        assert st.tolist() == [0] and ok == 1

        other_g1 = enc_points(c, [pyref.Group(c, False).mul(c.g1, 0xBADC0DE)], False)
        good = lambda i: proofs[i % len(proofs)]
        cases = {}   # position -> (record, input bytes, status)
        p0, y0 = good(0)
        cases["ar_replaced"] = (other_g1 + bs_of(p0) + krs_of(p0), fr([y0]), 2)
        cases["wrong_input"] = (p0, fr([y0 + 1]), 2)
        cases["swapped_a"] = (good(1)[0], fr([good(2)[1]]), 2)
        cases["swapped_b"] = (good(2)[0], fr([good(1)[1]]), 2)
        bs_pt = pyref.decode_point(c, bs_of(p0), True)
        off_curve = enc_points(c, [(bs_pt[0], pyref.F2(c).add(bs_pt[1], (1, 0)))], True)
        cases["bs_off_curve"] = (ar_of(p0) + off_curve + krs_of(p0), fr([y0]), 1)
        cases["input_is_r"] = (p0, c.r.to_bytes(32, "little"), 3)
        if name != "bn254":   # BN254's G1 has cofactor 1
            off_sub = enc_points(c, pc.sub.random_curve_points(c, False, 1, 0x6B), False)
            cases["krs_off_subgroup"] = (ar_of(p0) + bs_of(p0) + off_sub, fr([y0]), 1)
        # m = 5: bad first and last
        recs = [cases["wrong_input"], good(1) + (0,), good(2) + (0,), good(3) + (0,), cases["bs_off_curve"]]
        recs = [(r[0], r[1] if isinstance(r[1], bytes) else fr([r[1]]), r[2]) for r in recs]
        st, ok = key.verify_batch(b"".join(r[0] for r in recs), b"".join(r[1] for r in recs))
        assert st.tolist() == [2, 0, 0, 0, 1] and ok == 3
        # m = 70: bad proofs first, last and on both sides of the wave edge
        m = 70
        recs = [(good(i)[0], fr([good(i)[1]]), 0) for i in range(m)]
        for pos, cs in zip((0, 63, 64, 69, 17, 30, 40), cases.values()):
            recs[pos] = cs
        st, ok = key.verify_batch(b"".join(r[0] for r in recs), b"".join(r[1] for r in recs))
        assert st.tolist() == [r[2] for r in recs]
        assert ok == sum(1 for r in recs if r[2] == 0) and ok >= m - 7
    finally:
        key.free()


# ---- 5. the twelve bellman vectors ----------------------------------------------------------------
def test_bellman_vectors(gm_ctx):
    import gnark_mi355x as gm
    c = pyref.CURVES["bls12381"]
    vectors = pm.bellman_vectors()
    assert len(vectors) == 12
    verdicts = []
    for v in vectors:
        vk = v["vk"]
        g1_recs = [vk["alpha_g1"]] + vk["k"] + [v["proof"][0], v["proof"][2]]
        g2_recs = [vk["beta_g2"], vk["gamma_g2"], vk["delta_g2"], v["proof"][1]]
        p1, rep1 = gm_ctx.points_decode_host(2, b"".join(g1_recs), False, gm.ENC_COMPRESSED)
        p2, rep2 = gm_ctx.points_decode_host(2, b"".join(g2_recs), True, gm.ENC_COMPRESSED)
        if rep1["first_bad"] != rep1["n"] or rep2["first_bad"] != rep2["n"]:
            verdicts.append(False)     # a record that does not decode: rejected
            continue
        nk = len(vk["k"])
        key = gm.VerifyingKey(gm_ctx, 2, dict(alpha_g1=p1[:96], k_g1=p1[96:96 * (1 + nk)], beta_g2=p2[:192],
                                               gamma_g2=p2[192:384], delta_g2=p2[384:576]))
        try:
            proof = p1[96 * (1 + nk):96 * (2 + nk)] + p2[576:] + p1[96 * (2 + nk):]
            st, ok = key.verify_batch(proof, b"".join(pyref.encode_fr(c, x % c.r) for x in v["inputs"]))
            verdicts.append(st.tolist() == [0])
            assert ok == int(st[0] == 0)
        finally:
            key.free()
    assert verdicts == [v["ok"] for v in vectors]


# ---- 6. a KZG opening through gm_pairing_check ---------------------------------------------------
def test_kzg_opening_verifies_through_pairing_check(gm_ctx):
    name = "bls12377"
    c = pyref.CURVES[name]
    G1, G2 = pyref.Group(c, False), pyref.Group(c, True)
    n, tau = 64, 0x5EED5EED5EED5EED5EED5EED5EED5EED5EED5EED
    rng = random.Random(0x6C9)
    srs = [G1.mul(c.g1, pow(tau, i, c.r)) for i in range(n)]
    coeffs = [rng.randrange(c.r) for _ in range(n)]
    z = rng.randrange(c.r)
    fr = lambda vals: b"".join(pyref.encode_fr(c, v) for v in vals)
    S = gm_ctx.points_upload(name, enc_points(c, srs, False))
    F = gm_ctx.copy_to_device(fr(coeffs))
    try:
        commit = pyref.decode_point(c, gm_ctx.kzg_commit(name, S, fr(coeffs)), False)
        val, h = gm_ctx.kzg_open(name, S, F, fr([z]))
    finally:
        S.free()
        F.free()
    y = pyref.decode_fr(c, val)
    assert y == sum(co * pow(z, i, c.r) for i, co in enumerate(coeffs)) % c.r
    H = pyref.decode_point(c, h, False)
    tau_g2 = G2.mul(c.g2, tau)

    def check(claim):
        # e(C - claim G1 + z H, G2) e(-H, tau G2) = 1
        lhs = G1.add(G1.add(commit, G1.neg(G1.mul(c.g1, claim))), G1.mul(H, z))
        return gm_ctx.pairing_check(name, enc_points(c, [lhs, G1.neg(H)], False), enc_points(c, [c.g2, tau_g2], True), 2)
    assert check(y).tolist() == [1]
    assert check((y + 1) % c.r).tolist() == [0]


# ---- 7. refusals on a live context -------------------------------------------------------------------
@pytest.mark.parametrize("name", CURVES)
def test_refusals_leave_the_context_usable(gm_ctx, pools, name):
    import gnark_mi355x as gm
    L = gm.load_library()
    pool = pools[name]
    cid = gm.curve_id(name)
    g1, g2 = pool.arrays([[(5, 7), (-5, 7)]])
    a1, a2 = np.frombuffer(g1, np.uint8), np.frombuffer(g2, np.uint8)
    ok = np.full(4, 0xEE, np.uint8)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    h = gm_ctx.handle
    err = lambda: L.gm_last_error().decode()
    right = lambda: gm_ctx.pairing_check(name, g1, g2, 2).tolist() == [1]
    assert L.gm_pairing_check(h, 9, p(a1), p(a2), 1, 2, p(ok)) == ERR_INVALID and "unknown curve id" in err()
    assert right()
    assert L.gm_pairing_check(h, cid, None, p(a2), 1, 2, p(ok)) == ERR_INVALID and right()
    assert L.gm_pairing_check(h, cid, p(a1), p(a2), 1, 0, p(ok)) == ERR_INVALID and right()
    assert L.gm_pairing_check(h, cid, p(a1), p(a2), 0, 2, p(ok)) == 0 and right()
    d1, d2 = gm_ctx.copy_to_device(g1), gm_ctx.copy_to_device(g2)
    try:
        assert L.gm_pairing_check_device(h, cid, d1.ptr + 8, d2.ptr, 1, 2, p(ok)) == ERR_INVALID and "aligned" in err()
        assert L.gm_pairing_check_device(h, cid, d1.ptr, d2.ptr, 0, 2, p(ok)) == 0
        assert gm_ctx.pairing_check_device(name, d1, d2, 1, 2).tolist() == [1]
    finally:
        d1.free()
        d2.free()
    assert ok.tolist() == [0xEE] * 4
    # verification: m = 0 writes nothing, NULL arrays are refused, and a right call follows
    c = pool.m.c
    vk = vk_points(c, TOXIC)
    key = gm.VerifyingKey(gm_ctx, name, vk_bytes(c, vk))
    try:
        nb = ctypes.c_size_t(99)
        assert L.gm_g16_verify_batch(h, key.handle, None, None, 0, p(ok), ctypes.byref(nb)) == 0 and nb.value == 0
        assert L.gm_g16_verify_batch(h, key.handle, None, p(a1), 1, p(ok), None) == ERR_INVALID
        assert L.gm_g16_verify_batch(h, key.handle, p(a1), None, 1, p(ok), None) == ERR_INVALID
        assert L.gm_g16_verify_batch(h, key.handle, p(a1), p(a1), 1, None, None) == ERR_INVALID
        assert ok.tolist() == [0xEE] * 4
        # an all-infinity "proof" with input 0: kSum = K[0], and e(K[0], -gamma) e(-alpha, beta) != 1
        st, n_ok = key.verify_batch(bytes(8 * 8 * c.fp_limbs), bytes(32))
        assert st.tolist() == [2] and n_ok == 0
    finally:
        key.free()
    assert right()
