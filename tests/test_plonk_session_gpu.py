"""gm_plonk_pk_* / gm_plonk_session_*: a PLONK proving key resident on the device
and the prover's five rounds on it (backend/plonk/bls12-377/prove.go).

The expected values come from a model written here in Python integers from the
definitions in include/gnark_mi355x.h: blinded coefficient lists, Z by running
products with one modular inverse per row, h by its definition on the 4n coset
(pyref.fft / fft_inverse), the shard edits, the linearized polynomial by the
header's formula, the opening quotients by synthetic division.  The SRS comes
from a known tau (canonical points tau^i G, Lagrange points L_i(tau) G, both made
by the oracle from integer scalars), so the commit of a polynomial f in either
basis has one expected affine value: [f(tau)] G.  The model never calls the
library under test.

The challenges are derived between the rounds from the digests and values the
round before returned (SHA-256 of their bytes), so a round cannot be right by
accident of a fixed challenge.
"""
import functools
import hashlib
import random
import types

import pytest

import pyref

pytestmark = pytest.mark.gpu

CURVES = ("bn254", "bls12377")
NB_PUBLIC = 2
FIXED = ("ql", "qr", "qm", "qo", "qk", "s1", "s2", "s3")
BLINDS = (("l", "bl"), ("r", "br"), ("o", "bo"), ("z", "bz"))


# ---------------------------------------------------------------------------
# integers <-> bytes, small polynomial helpers
# ---------------------------------------------------------------------------
def enc(c, vals):
    """gnark's Montgomery words (pyref.encode_fr, without a call per element)."""
    r, R = c.r, 1 << 256
    assert c.fr_limbs == 4
    return b"".join([(v % r * R % r).to_bytes(32, "little") for v in vals])


def dec(c, b):
    """Integers of Montgomery words; every stored word must be fully reduced."""
    r = c.r
    raw = [int.from_bytes(b[i:i + 32], "little") for i in range(0, len(b), 32)]
    assert max(raw) < r
    rinv = pow(1 << 256, -1, r)
    return [x * rinv % r for x in raw]


def horner(r, f, x):
    acc = 0
    for a in reversed(f):
        acc = (acc * x + a) % r
    return acc


def canon(c, ev):
    """Lagrange regular -> canonical regular, integer inverse FFT."""
    return pyref.bit_reverse(pyref.fft_inverse(c, ev, "DIF"))


def blind(r, n, f, b):
    """f + (X^n - 1) b as a coefficient list (getBlindedCoefficients)."""
    out = list(f) + [0] * len(b)
    for i, bi in enumerate(b):
        out[i] = (out[i] - bi) % r
        out[n + i] = (out[n + i] + bi) % r
    return out


def quotient(r, f, fz, z):
    """(f - f(z)) / (X - z) by synthetic division."""
    f = list(f)
    f[0] = (f[0] - fz) % r
    for i in range(len(f) - 2, -1, -1):
        f[i] = (f[i] + f[i + 1] * z) % r
    return f[1:]


def fold(r, polys, gamma):
    out = [0] * max(len(f) for f in polys)
    gi = 1
    for f in polys:
        for j, a in enumerate(f):
            out[j] = (out[j] + gi * a) % r
        gi = gi * gamma % r
    return out


def challenge(c, label, *parts):
    """A fixed function of the bytes the prover has sent so far; never zero."""
    h = hashlib.sha256(label.encode())
    for p in parts:
        h.update(p)
    return 1 + int.from_bytes(h.digest(), "big") % (c.r - 1)


# ---------------------------------------------------------------------------
# SRS from a known tau
# ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def srs(oracle, cname, n):
    """(tau, canonical points tau^i G for i < n + 3, Lagrange points L_i(tau) G)."""
    import gnark_mi355x as gm
    c = pyref.CURVES[cname]
    r = c.r
    tau = pyref.random_scalars(c, 1, 0x8100 + n)[0]
    w = pyref.domain_generator(c, n)
    zn, ninv = (pow(tau, n, r) - 1) % r, pow(n, -1, r)
    assert zn
    lag, wi = [], 1
    for _ in range(n):  # L_i(tau) = (tau^n - 1) w^i / (n (tau - w^i))
        lag.append(zn * wi % r * ninv % r * pow((tau - wi) % r, -1, r) % r)
        wi = wi * w % r
    assert sum(lag) % r == 1
    g = gm.generator(cname)
    return (tau, oracle.batch_mul_base(cname, False, g, enc(c, [pow(tau, i, r) for i in range(n + 3)])),
            oracle.batch_mul_base(cname, False, g, enc(c, lag)), tuple(lag))


def point(oracle, cname, k):
    """[k] G as gnark affine bytes."""
    import gnark_mi355x as gm
    return oracle.batch_mul_base(cname, False, gm.generator(cname), enc(pyref.CURVES[cname], [k]))


# ---------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------
class Inst:
    """One circuit and one witness, as integers in the form the calls take them:
    Lagrange values, regular order; qk without public inputs / commitment values."""

    def __init__(self, c, n, nb, seed):
        rng = random.Random(seed)
        rnd = lambda k: [rng.randrange(c.r) for _ in range(k)]
        self.c, self.n, self.nb = c, n, nb
        self.fixed = {k: rnd(n) for k in FIXED}
        self.qcp = [rnd(n) for _ in range(nb)]
        self.rows = [NB_PUBLIC + 1 + 2 * j for j in range(nb)]  # 3, 5: inside n = 8
        self.set_witness(seed + 1)

    def set_witness(self, seed):
        c, n, nb = self.c, self.n, self.nb
        rng = random.Random(seed)
        rnd = lambda k: [rng.randrange(c.r) for _ in range(k)]
        self.w = {k: rnd(n) for k in ("l", "r", "o")}
        self.pi2 = [rnd(n) for _ in range(nb)]
        self.public, self.cvals = rnd(NB_PUBLIC), rnd(nb)
        self.b = {"bl": rnd(2), "br": rnd(2), "bo": rnd(2), "bz": rnd(3)}
        self.h_rand = rnd(2)
        self.salt = b"%d" % seed
        return self


# ---------------------------------------------------------------------------
# the model
# ---------------------------------------------------------------------------
def t_over_zh(c, n, ch, x, v, zs):
    """T(x) / Z_H(x) (gm_plonk_quotient's T) from the values v of the blinded
    polynomials at x, zs = Z~(w0 x)."""
    r, g = c.r, c.coset_gen
    a, b, gm_ = ch["alpha"], ch["beta"], ch["gamma"]
    L, R, O, Z = v["l"], v["r"], v["o"], v["z"]
    t = v["ql"] * L + v["qr"] * R + v["qm"] * L * R + v["qo"] * O + v["qk"]
    t += sum(q * p for q, p in zip(v["qcp"], v["pi2"]))
    t += a * ((L + b * v["s1"] + gm_) * (R + b * v["s2"] + gm_) * (O + b * v["s3"] + gm_) * zs
              - (L + b * x + gm_) * (R + b * g * x + gm_) * (O + b * g * g * x + gm_) * Z)
    zh = (pow(x, n, r) - 1) % r
    l1 = zh * pow(n * (x - 1) % r, -1, r)
    t += a * a * (Z - 1) * l1
    return t % r * pow(zh, -1, r) % r


def model_front(oracle, cname, inst):
    """Rounds 1 to 3 up to h: everything that does not depend on h_rand."""
    c, r, n = inst.c, inst.c.r, inst.n
    tau = srs(oracle, cname, n)[0]
    commit = lambda f: point(oracle, cname, horner(r, f, tau))
    m = types.SimpleNamespace(inst=inst, tau=tau, commit=commit, ch={})
    m.p = {k: canon(c, inst.fixed[k]) for k in FIXED if k != "qk"}
    qk = list(inst.fixed["qk"])
    qk[:NB_PUBLIC] = inst.public
    for row, v in zip(inst.rows, inst.cvals):
        qk[row] = v
    m.p["qk"] = canon(c, qk)
    m.qcp = [canon(c, f) for f in inst.qcp]
    m.pi2 = [canon(c, f) for f in inst.pi2]
    m.bsb = [commit(f) for f in m.pi2]
    for k in ("l", "r", "o"):
        m.p[k] = canon(c, inst.w[k])
    m.t = {k: blind(r, n, m.p[k], inst.b[bk]) for k, bk in BLINDS[:3]}
    m.lro = [commit(m.t[k]) for k in ("l", "r", "o")]
    beta = m.ch["beta"] = challenge(c, "beta", inst.salt, *m.bsb, *m.lro)
    gamma = m.ch["gamma"] = challenge(c, "gamma", inst.salt, *m.bsb, *m.lro)
    # Z: running products, one inverse per row (gm_plonk_perm_z)
    g, w = c.coset_gen, pyref.domain_generator(c, n)
    l, rr, o = (inst.w[k] for k in ("l", "r", "o"))
    s1, s2, s3 = (inst.fixed[k] for k in ("s1", "s2", "s3"))
    z, N, D, wi = [1], 1, 1, 1
    for i in range(n - 1):
        num = (l[i] + beta * wi + gamma) * (rr[i] + beta * g * wi + gamma) * (o[i] + beta * g * g * wi + gamma)
        den = (l[i] + beta * s1[i] + gamma) * (rr[i] + beta * s2[i] + gamma) * (o[i] + beta * s3[i] + gamma)
        N, D = N * num % r, D * den % r
        z.append(N * (pow(D, -1, r) if D else 0) % r)
        wi = wi * w % r
    m.p["z"] = canon(c, z)
    m.t["z"] = blind(r, n, m.p["z"], inst.b["bz"])
    m.z_digest = commit(m.t["z"])
    m.ch["alpha"] = challenge(c, "alpha", m.z_digest)
    # h: T / Z_H at the 4n points g w1^k, then the inverse coset transform
    N4 = 4 * n
    w1 = pyref.domain_generator(c, N4)
    assert pow(w1, 4, r) == w
    evals = lambda f: pyref.fft(c, pyref.bit_reverse(list(f) + [0] * (N4 - len(f))), "DIT", True)  # natural order
    polys = {k: m.t.get(k, m.p[k]) for k in FIXED + ("l", "r", "o", "z")}
    ev = {k: evals(f) for k, f in polys.items()}
    eq, ep = [evals(f) for f in m.qcp], [evals(f) for f in m.pi2]
    vals, x = [], g
    for k in range(N4):
        v = {name: e[k] for name, e in ev.items()}
        v["qcp"], v["pi2"] = [e[k] for e in eq], [e[k] for e in ep]
        vals.append(t_over_zh(c, n, m.ch, x, v, ev["z"][(k + 4) % N4]))  # w0 = w1^4
        x = x * w1 % r
    m.h = pyref.fft_inverse(c, pyref.bit_reverse(vals), "DIT", True)
    return m


def model_back(oracle, cname, m, h_rand):
    """The expected outputs of a whole proof, in the shape run_proof returns."""
    inst = m.inst
    c, r, n, nb = inst.c, inst.c.r, inst.n, inst.nb
    mm = n + 2
    commit, ch = m.commit, dict(m.ch)
    h = m.h
    sh = [list(h[k * mm:(k + 1) * mm]) for k in range(3)]
    if h_rand:
        r0, r1 = inst.h_rand
        sh[0].append(r0)
        sh[1][0] = (sh[1][0] - r0) % r
        sh[1].append(r1)
        sh[2][0] = (sh[2][0] - r1) % r
    h_digests = [commit(f) for f in sh]
    ze = ch["zeta"] = challenge(c, "zeta", *h_digests)
    al, be, ga = ch["alpha"], ch["beta"], ch["gamma"]
    g, w = c.coset_gen, pyref.domain_generator(c, n)
    wze = w * ze % r
    # the evaluations and the scalars of the combination (gm_plonk_linearize)
    le, re_, oe = (horner(r, m.t[k], ze) for k in ("l", "r", "o"))
    s1e, s2e = horner(r, m.p["s1"], ze), horner(r, m.p["s2"], ze)
    zue = horner(r, m.t["z"], wze)
    qcpe = [horner(r, f, ze) for f in m.qcp]
    zh = (pow(ze, n, r) - 1) % r
    zm = pow(ze, mm, r)
    inv0 = pow(ze - 1, -1, r) if (ze - 1) % r else 0
    rl = le * re_ % r
    c1 = al * (le + be * s1e + ga) % r * (re_ + be * s2e + ga) % r * be % r * zue % r
    c2 = -al * (le + be * ze + ga) % r * (re_ + be * g * ze + ga) % r * (oe + be * g * g * ze + ga) % r
    a2l = al * al % r * zh % r * inv0 % r * pow(n, -1, r) % r
    p, zt = m.p, m.t["z"]
    lin = []
    for i in range(n + 3):
        t = (c2 + a2l) * zt[i]
        if i < n:
            t += (c1 * p["s3"][i] + rl * p["qm"][i] + le * p["ql"][i] + re_ * p["qr"][i] + oe * p["qo"][i] + p["qk"][i])
            t += sum(q * f[i] for q, f in zip(qcpe, m.pi2))
        if i < mm:
            t -= zh * (h[i] + zm * h[mm + i] + zm * zm * h[2 * mm + i])
        lin.append(t % r)
    if h_rand:
        r0, r1 = inst.h_rand
        lin[0] = (lin[0] + zh * (zm * r0 + zm * zm * r1)) % r
        lin[mm] = (lin[mm] - zh * (r0 + zm * r1)) % r
    lin_digest = commit(lin)
    claimed = [horner(r, lin, ze), le, re_, oe, s1e, s2e] + qcpe
    z_open = commit(quotient(r, zt, zue, wze))
    claimed_b = [enc(c, [v]) for v in claimed]
    kg = ch["kzg_gamma"] = challenge(c, "kzg", lin_digest, *claimed_b, enc(c, [zue]), z_open)
    polys = [lin, m.t["l"], m.t["r"], m.t["o"], p["s1"], p["s2"]] + m.qcp
    folded = fold(r, polys, kg)
    fv = sum(pow(kg, i, r) * v for i, v in enumerate(claimed)) % r
    assert fv == horner(r, folded, ze)
    batch = commit(quotient(r, folded, fv, ze))
    out = dict(bsb=m.bsb, lro=m.lro, z=m.z_digest, h=h_digests, lin=lin_digest, claimed=claimed_b,
               z_shifted=enc(c, [zue]), z_open=z_open, batch=batch)
    return out, types.SimpleNamespace(ch=ch, lin=lin, sh=sh, claimed=claimed, zue=zue)


@functools.lru_cache(maxsize=None)
def random_case(oracle, cname, n, nb):
    inst = Inst(pyref.CURVES[cname], n, nb, 0x8200 + 16 * n + nb)
    return inst, model_front(oracle, cname, inst)


# ---------------------------------------------------------------------------
# the device side
# ---------------------------------------------------------------------------
def make_key(ctx, oracle, cname, inst, cache=True, **over):
    import gnark_mi355x as gm
    c = inst.c
    _, can, lag, _ = srs(oracle, cname, inst.n)
    a = dict(n=inst.n, nb_public=NB_PUBLIC, polys={k: enc(c, inst.fixed[k]) for k in FIXED},
             qcp=[enc(c, f) for f in inst.qcp], commitment_row=list(inst.rows), srs_canonical=can,
             srs_lagrange=lag, cache=cache)
    a.update(over)
    return gm.PlonkProvingKey(ctx, cname, **a)


def run_proof(key, inst, h_rand, upto=5):
    """A whole proof (or its first `upto` rounds) with the challenges derived from
    what the rounds return; every output, keyed as model_back keys them."""
    c = inst.c
    e1 = lambda v: enc(c, [v])
    s = key.session()
    try:
        out = {"bsb": [s.bsb22(j, enc(c, inst.pi2[j])) for j in range(inst.nb)]}
        out["lro"] = s.round1(enc(c, inst.w["l"]), enc(c, inst.w["r"]), enc(c, inst.w["o"]), enc(c, inst.public),
                              {k: enc(c, v) for k, v in inst.b.items()},
                              commitment_vals=enc(c, inst.cvals) if inst.nb else None,
                              h_rand=enc(c, inst.h_rand) if h_rand else None)
        if upto == 1:
            return out
        beta = challenge(c, "beta", inst.salt, *out["bsb"], *out["lro"])
        gamma = challenge(c, "gamma", inst.salt, *out["bsb"], *out["lro"])
        out["z"] = s.round2(e1(beta), e1(gamma))
        if upto == 2:
            return out
        out["h"] = s.round3(e1(challenge(c, "alpha", out["z"])))
        if upto == 3:
            return out
        out["lin"], out["claimed"], out["z_shifted"], out["z_open"] = s.round4(e1(challenge(c, "zeta", *out["h"])))
        if upto == 4:
            return out
        out["batch"] = s.round5(e1(challenge(c, "kzg", out["lin"], *out["claimed"], out["z_shifted"], out["z_open"])))
        return out
    finally:
        s.free()


def assert_same(got, want):
    """Round by round, so that the first round that is off is the one named."""
    for k in ("bsb", "lro", "z", "h", "lin", "claimed", "z_shifted", "z_open", "batch"):
        assert got[k] == want[k], k
    assert set(got) == set(want)


# ---------------------------------------------------------------------------
# 1. a whole proof against the integer model
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("h_rand", [False, True])
@pytest.mark.parametrize("nb", [0, 2])
@pytest.mark.parametrize("n", [8, 64, 1024])
@pytest.mark.parametrize("cname", CURVES)
def test_whole_proof_against_the_integer_model(gm_ctx, oracle, cname, n, nb, h_rand):
    inst, front = random_case(oracle, cname, n, nb)
    c, r = inst.c, inst.c.r
    if n == 8:
        # the model's own footing: a commit over the Lagrange SRS is [f(tau)] G
        tau, _, _, lag = srs(oracle, cname, n)
        assert sum(v * k for v, k in zip(inst.w["l"], lag)) % r == horner(r, front.p["l"], tau)
    assert any(front.h[3 * (n + 2):])  # not a satisfying instance: h fills all 4n coefficients
    want, _ = model_back(oracle, cname, front, h_rand)
    key = make_key(gm_ctx, oracle, cname, inst)
    try:
        assert_same(run_proof(key, inst, h_rand), want)
    finally:
        key.free()


# ---------------------------------------------------------------------------
# 2. a satisfying instance: the verifier's identity and the openings in the exponent
# ---------------------------------------------------------------------------
class Sat(Inst):
    """Two public-input rows (ql = -1, the input in l and, through Qk, against it)
    followed by multiplication gates l r = o with shared wires -- a permutation
    that is not the identity and that ties a public input into the circuit (the
    construction of test_plonk_linearize_gpu.py, restated and extended)."""

    def __init__(self, c, n):
        r = c.r
        rng = random.Random(0x8300)
        g, w = c.coset_gen, pyref.domain_generator(c, n)
        lv, rv, ov = [0] * n, [0] * n, [0] * n
        sigma = list(range(3 * n))  # wire column k, row i -> k n + i

        def tie(a, b):  # merge the cycles of a and b
            sigma[a], sigma[b] = sigma[b], sigma[a]

        public = [rng.randrange(r) for _ in range(NB_PUBLIC)]
        lv[:NB_PUBLIC] = public
        first = NB_PUBLIC
        for i in range(first, n):
            lv[i] = rng.randrange(r)
            rv[i] = rng.randrange(r)
            if i % 2 == 1:
                rv[i] = ov[i - 1]
                tie(n + i, 2 * n + i - 1)
            if i % 4 == 0:
                lv[i] = lv[first]
                tie(i, first)
            if i == 6:
                lv[i] = lv[0]  # the first public input is used by a gate
                tie(i, 0)
            ov[i] = lv[i] * rv[i] % r
        assert sigma != list(range(3 * n))
        vals = lv + rv + ov
        assert all(vals[sigma[k]] == vals[k] for k in range(3 * n))
        ids = [pow(w, i, r) for i in range(n)] + [g * pow(w, i, r) % r for i in range(n)] + \
              [g * g * pow(w, i, r) % r for i in range(n)]
        s = [ids[sigma[k]] for k in range(3 * n)]
        rnd = lambda m: [rng.randrange(r) for _ in range(m)]
        self.c, self.n, self.nb = c, n, 0
        mul = [0] * first + [1] * (n - first)
        self.fixed = {"ql": [r - 1] * first + [0] * (n - first), "qr": [0] * n, "qm": mul,
                      "qo": [(r - x) % r for x in mul], "qk": [0] * n,
                      "s1": s[:n], "s2": s[n:2 * n], "s3": s[2 * n:]}
        self.qcp, self.pi2, self.rows, self.cvals = [], [], [], []
        self.w = {"l": lv, "r": rv, "o": ov}
        self.public = public
        self.b = {"bl": rnd(2), "br": rnd(2), "bo": rnd(2), "bz": rnd(3)}
        self.h_rand = rnd(2)
        self.salt = b"sat"


@pytest.mark.parametrize("cname", CURVES)
def test_satisfying_instance_verifies(gm_ctx, oracle, cname):
    n = 64
    c = pyref.CURVES[cname]
    r = c.r
    sat = Sat(c, n)
    front = model_front(oracle, cname, sat)
    # the quotient of a satisfied instance has degree 3n + 5
    assert not any(front.h[3 * n + 6:]) and any(front.h[2 * n + 4:3 * n + 6])
    want, w = model_back(oracle, cname, front, True)
    key = make_key(gm_ctx, oracle, cname, sat)
    try:
        got = run_proof(key, sat, True)
    finally:
        key.free()
    assert_same(got, want)
    ch, tau = w.ch, front.tau
    al, be, ga, ze = ch["alpha"], ch["beta"], ch["gamma"], ch["zeta"]
    lin_ze, le, re_, oe, s1e, s2e = dec(c, b"".join(got["claimed"]))
    (zue,) = dec(c, got["z_shifted"])
    # the verifier's identity at zeta on the returned values (verify.go:213-225; the
    # public inputs are inside the completed Qk, so inside lin)
    l1 = (pow(ze, n, r) - 1) * pow(n * (ze - 1) % r, -1, r) % r
    assert lin_ze == -(al * (le + be * s1e + ga) % r * (re_ + be * s2e + ga) % r * (oe + ga) % r * zue
                       - al * al * l1) % r
    # the KZG identities in the exponent: C - [v] G = [tau - z] H
    G = pyref.Group(c, False)
    P = lambda b: pyref.decode_point(c, b, False)
    gen = G.generator()

    def opens(commitment, value, z, proof):
        return G.add(commitment, G.neg(G.mul(gen, value))) == G.mul(proof, (tau - z) % r)

    wze = pyref.domain_generator(c, n) * ze % r
    assert opens(P(got["z"]), zue, wze, P(got["z_open"]))
    kg = ch["kzg_gamma"]
    s1c, s2c = (P(point(oracle, cname, horner(r, front.p[k], tau))) for k in ("s1", "s2"))
    commitments = [P(got["lin"])] + [P(b) for b in got["lro"]] + [s1c, s2c]
    folded_c, folded_v, gi = None, 0, 1
    for cm, v in zip(commitments, (lin_ze, le, re_, oe, s1e, s2e)):
        t = G.mul(cm, gi)
        folded_c = t if folded_c is None else G.add(folded_c, t)
        folded_v = (folded_v + gi * v) % r
        gi = gi * kg % r
    assert opens(folded_c, folded_v, ze, P(got["batch"]))
    # and the shards recombine to h at tau: h1' + tau^m h2' + tau^2m h3' (m + 1 with StatisticalZK's degree)
    hs = [P(b) for b in got["h"]]
    tm = pow(tau, n + 2, r)
    assert G.add(G.add(hs[0], G.mul(hs[1], tm)), G.mul(hs[2], tm * tm % r)) == G.mul(gen, horner(r, front.h, tau))


# ---------------------------------------------------------------------------
# 3. cache on = cache off
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("nb", [0, 2])
@pytest.mark.parametrize("n", [8, 1024])
@pytest.mark.parametrize("cname", CURVES)
def test_cache_on_equals_cache_off(gm_ctx, oracle, cname, n, nb):
    inst, _ = random_case(oracle, cname, n, nb)
    keys = [make_key(gm_ctx, oracle, cname, inst, cache=on) for on in (True, False)]
    try:
        resident = [k.resident_bytes() for k in keys]
        assert resident[0][1] == 4 * (8 + nb) * n * 32 and resident[1][1] == 0
        assert resident[0][0] == resident[1][0] + resident[0][1]
        a, b = (run_proof(k, inst, True) for k in keys)
        assert_same(a, b)
    finally:
        for k in keys:
            k.free()


# ---------------------------------------------------------------------------
# 4. the key is never written; sessions are independent
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("cname", CURVES)
def test_key_untouched_and_sessions_independent(gm_ctx, oracle, cname):
    n, nb = 64, 2
    inst, front = random_case(oracle, cname, n, nb)
    want, _ = model_back(oracle, cname, front, True)
    other = Inst(inst.c, n, nb, 0x8200 + 16 * n + nb).set_witness(0x8400)  # the same circuit, another witness
    key = make_key(gm_ctx, oracle, cname, inst)
    try:
        first = run_proof(key, inst, True)
        assert_same(first, want)
        second = run_proof(key, other, False)
        assert second["lro"] != first["lro"] and second["batch"] != first["batch"]
        gm_ctx.trim()
        # a session that ends after round 2
        assert run_proof(key, other, True, upto=2)["z"] == second["z"]
        third = run_proof(key, inst, True)
        assert_same(third, first)
        gm_ctx.trim()
        assert_same(run_proof(key, other, False), second)
    finally:
        key.free()


# ---------------------------------------------------------------------------
# 5. refusals: each leaves the session or the key's context able to finish a proof
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("cname", CURVES)
def test_refusals(gm_ctx, oracle, cname):
    import gnark_mi355x as gm
    n, nb = 64, 2
    inst, front = random_case(oracle, cname, n, nb)
    c = inst.c
    want, _ = model_back(oracle, cname, front, False)
    e1 = lambda v: enc(c, [v])
    one = e1(1)

    def refused(f, *a, **kw):
        with pytest.raises(gm.GmError) as e:
            f(*a, **kw)
        assert "error -1: plonk" in str(e.value), str(e.value)

    # uploads
    fixed = {k: enc(c, inst.fixed[k]) for k in FIXED}
    for name, over in {
        "n = 48": dict(n=48),
        "n = 4": dict(n=4),
        "short canonical SRS": dict(srs_canonical_len=n + 2),
        "commitment row = n": dict(commitment_row=[3, n]),
        "null ql": dict(polys=dict(fixed, ql=None)),
        "null s3": dict(polys=dict(fixed, s3=None)),
        "null Lagrange SRS": dict(srs_lagrange=None),
        "null qcp table": dict(qcp=None),
        "null qcp entry": dict(qcp=[enc(c, inst.qcp[0]), None]),
    }.items():
        refused(make_key, gm_ctx, oracle, cname, inst, **over)

    key = make_key(gm_ctx, oracle, cname, inst)
    s = key.session()
    try:
        wires = [enc(c, inst.w[k]) for k in ("l", "r", "o")]
        blinds = {k: enc(c, v) for k, v in inst.b.items()}
        pub, cv = enc(c, inst.public), enc(c, inst.cvals)
        # before round 1
        refused(s.round2, one, one)
        refused(s.round3, one)
        refused(s.round4, one)
        refused(s.round5, one)
        refused(s.round1, *wires, pub, blinds, commitment_vals=cv)  # no bsb22 call yet
        refused(s.bsb22, nb, enc(c, inst.pi2[0]))
        refused(s.bsb22, 0, None)
        got = {"bsb": [s.bsb22(0, enc(c, inst.pi2[0]))]}
        refused(s.round1, *wires, pub, blinds, commitment_vals=cv)  # one of two
        got["bsb"].append(s.bsb22(1, enc(c, inst.pi2[1])))
        refused(s.round1, None, wires[1], wires[2], pub, blinds, commitment_vals=cv)
        refused(s.round1, *wires, None, blinds, commitment_vals=cv)
        refused(s.round1, *wires, pub, blinds, commitment_vals=None)
        refused(s.round1, *wires, pub, dict(blinds, bz=None), commitment_vals=cv)
        got["lro"] = s.round1(*wires, pub, blinds, commitment_vals=cv)
        # after round 1
        refused(s.bsb22, 0, enc(c, inst.pi2[0]))
        refused(s.round1, *wires, pub, blinds, commitment_vals=cv)
        refused(s.round3, one)
        L = gm.load_library()
        assert L.gm_plonk_session_round2(s.handle, None, None, None) == -1
        assert L.gm_last_error().decode().startswith("plonk session: round 2")
        beta = challenge(c, "beta", inst.salt, *got["bsb"], *got["lro"])
        gamma = challenge(c, "gamma", inst.salt, *got["bsb"], *got["lro"])
        got["z"] = s.round2(e1(beta), e1(gamma))
        refused(s.round2, e1(beta), e1(gamma))
        refused(s.round4, one)
        assert L.gm_plonk_session_round3(s.handle, None, None) == -1
        got["h"] = s.round3(e1(challenge(c, "alpha", got["z"])))
        refused(s.round3, one)
        refused(s.round5, one)
        assert L.gm_plonk_session_round4(s.handle, None, None, None, None, None) == -1
        got["lin"], got["claimed"], got["z_shifted"], got["z_open"] = s.round4(e1(challenge(c, "zeta", *got["h"])))
        refused(s.round4, one)
        assert L.gm_plonk_session_round5(s.handle, None, None) == -1
        got["batch"] = s.round5(e1(challenge(c, "kzg", got["lin"], *got["claimed"], got["z_shifted"], got["z_open"])))
        refused(s.round5, one)
        refused(s.round1, *wires, pub, blinds, commitment_vals=cv)
        # the session that met every refusal made a correct proof
        assert_same(got, want)
    finally:
        s.free()
        key.free()
