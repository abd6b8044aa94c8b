"""Integer model of PLONK and KZG verification (gm_plonk_verify_batch,
gm_kzg_verify_batch), written from backend/plonk/bn254/verify.go:128-322 with
kzg.FoldProof and kzg.BatchVerifyMultiPoints, and a model prover that makes valid
proofs without the library.

Everything lives in the exponent: the SRS has a known tau, so a commitment to f is
[f(tau)] G and a point is carried as its discrete logarithm.  The verifier's two
pairs (A, G2[0]) (B, -[tau] G2) then hold exactly when a - tau b = 0 mod r, with a
and b the logarithms of A and B.  Points as bytes are made in one
oracle.batch_mul_base call (to_points); the model itself never calls the library.

The prover follows gnark: the linearised polynomial carries the key's Qk (prove.go
innerComputeLinearizedPoly reads trace.Qk), the public inputs and the hashed
commitments reach the verifier through PI(zeta) alone.
"""
import functools
import hashlib
import random
import types

import pyref

_SESSION_HELPERS = ("blind", "canon", "fold", "horner", "quotient", "t_over_zh")


def __getattr__(name):
    """The polynomial helpers of test_plonk_session_gpu.py, imported when the prover
    first needs them: the verifier half (scalars, verify, enc) stands alone, so a
    tool can use it without importing a test module."""
    if name in _SESSION_HELPERS:
        import test_plonk_session_gpu as sess
        for k in _SESSION_HELPERS:
            globals()[k] = getattr(sess, k)
        return globals()[name]
    raise AttributeError(name)


def _load_helpers():
    __getattr__("horner")


OK, BAD_POINT, MISMATCH, BAD_INPUT, ALGEBRAIC = 0, 1, 2, 3, 4
CURVES = ("bn254", "bls12377", "bls12381")
KEY_POINTS = ("ql", "qr", "qm", "qo", "qk", "s1", "s2", "s3")
PROOF_POINTS = ("L", "R", "O", "Z", "H0", "H1", "H2", "Hb", "Hz")
CHALLENGES = ("gamma", "beta", "alpha", "zeta", "v", "u")


def enc(c, vals):
    """gnark's Montgomery words of reduced integers."""
    r, R = c.r, 1 << 256
    return b"".join([(v % r * R % r).to_bytes(32, "little") for v in vals])


def enc_raw(c, vals):
    """The same for values that may be >= r: a value below r is encoded, a value
    >= r is stored as it is (the word string the entry must refuse)."""
    r, R = c.r, 1 << 256
    return b"".join([(v * R % r if v < r else v).to_bytes(32, "little") for v in vals])


def dec(c, b):
    r = c.r
    raw = [int.from_bytes(b[i:i + 32], "little") for i in range(0, len(b), 32)]
    assert max(raw) < r
    rinv = pow(1 << 256, -1, r)
    return [x * rinv % r for x in raw]


def inv0(x, r):
    """gnark's inverse: 0 for 0."""
    return pow(x, -1, r) if x % r else 0


def challenge(c, label, *ints):
    h = hashlib.sha256(label.encode())
    for v in ints:
        h.update(int(v).to_bytes(32, "big"))
    return 1 + int.from_bytes(h.digest(), "big") % (c.r - 1)


# ---------------------------------------------------------------------------
# the verifier
# ---------------------------------------------------------------------------
def scalars(c, vk, values, publics, hashed, chal):
    """(scalar vector in the order of the device's ladders, PI(zeta), constLin, class
    without the points).  vk: n, nb_public, rows.  Any input >= r, or u = 0: BAD_INPUT,
    and the rest is computed with that input replaced by 0."""
    r, n, nb = c.r, vk.n, len(vk.rows)
    bad = any(x >= r for x in list(values) + list(publics) + list(hashed) + list(chal))
    z = lambda x: 0 if x >= r else x
    values, publics, hashed = [z(x) for x in values], [z(x) for x in publics], [z(x) for x in hashed]
    gamma, beta, alpha, zeta, v, u = [z(x) for x in chal]
    bad = bad or u == 0
    lin, l, rr, o, s1, s2 = values[:6]
    qcp, zu = values[6:6 + nb], values[6 + nb]
    w, g = pyref.domain_generator(c, n), c.coset_gen
    ninv = pow(n, -1, r)
    zn = pow(zeta, n, r)
    zh = (zn - 1) % r
    lag0 = inv0(zeta - 1, r) * zh % r * ninv % r
    pi, wi = 0, 1
    for x in publics:
        pi = (pi + x * wi % r * ninv % r * zh % r * inv0(zeta - wi, r)) % r
        wi = wi * w % r
    for row, hc in zip(vk.rows, hashed):
        wr = pow(w, row, r)
        pi = (pi + hc * wr % r * ninv % r * zh % r * inv0(zeta - wr, r)) % r
    a2l = lag0 * alpha % r * alpha % r
    p12 = (beta * s1 + gamma + l) % r * ((s2 * beta + gamma + rr) % r) % r
    const_lin = -((o + gamma) * p12 % r * alpha % r * zu - a2l + pi) % r
    cls = BAD_INPUT if bad else (ALGEBRAIC if const_lin != lin else OK)
    s1c = p12 * beta % r * alpha % r * zu % r
    s2c = -((beta * zeta + gamma + l) * (beta * g * zeta + gamma + rr) % r * (beta * g * g * zeta + o + gamma) % r
            * alpha) % r
    coeff_z = (a2l + s2c) % r
    znp2 = zn * zeta * zeta % r
    y = sum(pow(v, i, r) * x for i, x in enumerate(values[:6 + nb])) % r
    key = [-(y + u * zu) % r, l, rr, l * rr % r, o, s1c, pow(v, 4, r), pow(v, 5, r)] + \
          [pow(v, 6 + j, r) for j in range(nb)]
    proof = [v, v * v % r, pow(v, 3, r), (coeff_z + u) % r, -zh % r, -znp2 * zh % r, -znp2 * znp2 % r * zh % r,
             zeta, u * w % r * zeta % r] + qcp
    return key + proof + [u], pi, const_lin, cls


def verify(c, vk, proof):
    """The status gm_plonk_verify_batch must give.  vk.dl: the key points' logarithms
    (ql ... s3, qcp list), vk.tau; proof: dl (9 + nb_bsb logarithms in the entry's
    order), values, publics, hashed, chal, and bad_point (a point that is not one)."""
    r, nb = c.r, len(vk.rows)
    if getattr(proof, "bad_point", False):
        return BAD_POINT
    sc, _, _, cls = scalars(c, vk, proof.values, proof.publics, proof.hashed, proof.chal)
    if cls != OK:
        return cls
    d = vk.dl
    key = [1, d["ql"], d["qr"], d["qm"], d["qo"], d["s3"], d["s1"], d["s2"]] + list(d["qcp"])
    bases = key + list(proof.dl) + [proof.dl[8]]
    assert len(bases) == len(sc) == 18 + 2 * nb
    a = (sum(s * b for s, b in zip(sc[:-1], bases[:-1])) + d["qk"]) % r
    b = (proof.dl[7] + sc[-1] * bases[-1]) % r
    return OK if (a - vk.tau * b) % r == 0 else MISMATCH


def kzg_verify(c, tau, dl_c, dl_h, z, y, bad_point=False):
    r = c.r
    if bad_point:
        return BAD_POINT
    if z >= r or y >= r:
        return BAD_INPUT
    return OK if (dl_c - y + z * dl_h - tau * dl_h) % r == 0 else MISMATCH


def kzg_verify_folded(c, tau, openings, lambdas):
    """openings: (dl_c, dl_h, z, y, bad_point); lambda_0 is taken as 1."""
    r = c.r
    lam = [1] + list(lambdas[1:])
    if any(o[4] for o in openings):
        return BAD_POINT
    if any(o[2] >= r or o[3] >= r for o in openings) or any(x >= r or x == 0 for x in lam[1:]):
        return BAD_INPUT
    a = sum(x * (o[0] - o[3] + o[2] * o[1]) for x, o in zip(lam, openings)) % r
    b = sum(x * o[1] for x, o in zip(lam, openings)) % r
    return OK if (a - tau * b) % r == 0 else MISMATCH


# ---------------------------------------------------------------------------
# a satisfying instance
# ---------------------------------------------------------------------------
class SatInst:
    """A circuit of n rows and a witness that satisfies it, as Lagrange values in
    regular order, in the form gm_plonk_pk_upload and the session take them:
    - a permutation with real cycles over the 3n positions, the wire values constant
      on each cycle, s1, s2, s3 taken from it;
    - random ql, qr, qm, qo, qcp_j and committed-values polynomials pi2_j;
    - the key's qk solved per row so that the gate holds; on the public rows and the
      commitment rows it is 0 (gnark's trace.Qk), the completed Qk carries the public
      input or the hashed commitment there, and qo is solved instead."""

    def __init__(self, c, n, nb_public, nb, seed):
        r = c.r
        rng = random.Random(seed)
        rnd = lambda k: [rng.randrange(r) for _ in range(k)]
        self.c, self.n, self.nb, self.nb_public = c, n, nb, nb_public
        # cycles of length 1 to 4 over a shuffle of the 3n positions
        pos = list(range(3 * n))
        rng.shuffle(pos)
        sigma, vals, k = list(range(3 * n)), [0] * (3 * n), 0
        while k < len(pos):
            cyc = pos[k:k + rng.randrange(1, 5)]
            k += len(cyc)
            v = rng.randrange(1, r)
            for a, b in zip(cyc, cyc[1:] + cyc[:1]):
                sigma[a] = b
                vals[a] = v
        assert sigma != list(range(3 * n)) and all(vals[sigma[q]] == vals[q] for q in range(3 * n))
        g, w = c.coset_gen, pyref.domain_generator(c, n)
        wp = [pow(w, i, r) for i in range(n)]
        ids = wp + [g * x % r for x in wp] + [g * g * x % r for x in wp]
        s = [ids[sigma[q]] for q in range(3 * n)]
        self.sigma = sigma  # gnark's trace.S
        self.w = {"l": vals[:n], "r": vals[n:2 * n], "o": vals[2 * n:]}
        self.rows = [nb_public + 1 + 2 * j for j in range(nb)]
        self.public, self.cvals = rnd(nb_public), rnd(nb)   # cvals: the hashed commitments
        self.qcp, self.pi2 = [rnd(n) for _ in range(nb)], [rnd(n) for _ in range(nb)]
        ql, qr, qm, qo = rnd(n), rnd(n), rnd(n), rnd(n)
        forced = {i: x for i, x in enumerate(self.public)}
        forced.update(dict(zip(self.rows, self.cvals)))
        qk, full = [0] * n, [0] * n
        l, rr, o = self.w["l"], self.w["r"], self.w["o"]
        for i in range(n):
            rest = (ql[i] * l[i] + qr[i] * rr[i] + qm[i] * l[i] * rr[i]
                    + sum(q[i] * p[i] for q, p in zip(self.qcp, self.pi2))) % r
            if i in forced:
                full[i] = forced[i]
                qo[i] = -(rest + full[i]) * pow(o[i], -1, r) % r
            else:
                qk[i] = full[i] = -(rest + qo[i] * o[i]) % r
            assert (rest + qo[i] * o[i] + full[i]) % r == 0
        self.fixed = {"ql": ql, "qr": qr, "qm": qm, "qo": qo, "qk": qk, "s1": s[:n], "s2": s[n:2 * n], "s3": s[2 * n:]}
        self.qk_full = full
        self.b = {"bl": rnd(2), "br": rnd(2), "bo": rnd(2), "bz": rnd(3)}
        self.h_rand = rnd(2)
        self.salt = b"sat%d" % seed


def tau_of(c, n):
    return pyref.random_scalars(c, 1, 0x8100 + n)[0]  # test_plonk_session_gpu.srs's tau


def model_vk(inst, tau):
    """The verifying key in the exponent."""
    _load_helpers()
    c, r = inst.c, inst.c.r
    dl = {k: horner(r, canon(c, inst.fixed[k]), tau) for k in KEY_POINTS}
    dl["qcp"] = [horner(r, canon(c, f), tau) for f in inst.qcp]
    return types.SimpleNamespace(n=inst.n, nb_public=inst.nb_public, rows=list(inst.rows), dl=dl, tau=tau)


def model_prove(inst, tau, u_seed=1):
    """A proof of inst as the verifier's inputs, every point as its logarithm."""
    _load_helpers()
    c, r, n, nb = inst.c, inst.c.r, inst.n, inst.nb
    mm = n + 2
    at_tau = lambda f: horner(r, f, tau)
    p = {k: canon(c, inst.fixed[k]) for k in KEY_POINTS}
    p["qk_full"] = canon(c, inst.qk_full)
    qcp, pi2 = [canon(c, f) for f in inst.qcp], [canon(c, f) for f in inst.pi2]
    t = {k: blind(r, n, canon(c, inst.w[k]), inst.b[bk]) for k, bk in (("l", "bl"), ("r", "br"), ("o", "bo"))}
    dl = {"L": at_tau(t["l"]), "R": at_tau(t["r"]), "O": at_tau(t["o"])}
    bsb = [at_tau(f) for f in pi2]
    gamma = challenge(c, "gamma", *bsb, dl["L"], dl["R"], dl["O"], *inst.public)
    beta = challenge(c, "beta", gamma)
    # Z: running products
    g, w = c.coset_gen, pyref.domain_generator(c, n)
    l, rr, o = (inst.w[k] for k in ("l", "r", "o"))
    s1, s2, s3 = (inst.fixed[k] for k in ("s1", "s2", "s3"))
    z, N, D, wi = [1], 1, 1, 1
    for i in range(n - 1):
        N = N * (l[i] + beta * wi + gamma) % r * (rr[i] + beta * g * wi + gamma) % r * (o[i] + beta * g * g * wi + gamma) % r
        D = D * (l[i] + beta * s1[i] + gamma) % r * (rr[i] + beta * s2[i] + gamma) % r * (o[i] + beta * s3[i] + gamma) % r
        z.append(N * pow(D, -1, r) % r)
        wi = wi * w % r
    t["z"] = blind(r, n, canon(c, z), inst.b["bz"])
    dl["Z"] = at_tau(t["z"])
    alpha = challenge(c, "alpha", *bsb, dl["Z"])
    ch = {"alpha": alpha, "beta": beta, "gamma": gamma}
    # h = T / Z_H on the 4n coset
    N4 = 4 * n
    w1 = pyref.domain_generator(c, N4)
    evals = lambda f: pyref.fft(c, pyref.bit_reverse(list(f) + [0] * (N4 - len(f))), "DIT", True)
    names = ("ql", "qr", "qm", "qo", "s1", "s2", "s3")
    ev = {k: evals(p[k]) for k in names}
    ev["qk"] = evals(p["qk_full"])
    ev.update({k: evals(t[k]) for k in ("l", "r", "o", "z")})
    eq, ep = [evals(f) for f in qcp], [evals(f) for f in pi2]
    vals, x = [], g
    for k in range(N4):
        v = {name: e[k] for name, e in ev.items()}
        v["qcp"], v["pi2"] = [e[k] for e in eq], [e[k] for e in ep]
        vals.append(t_over_zh(c, n, ch, x, v, ev["z"][(k + 4) % N4]))
        x = x * w1 % r
    h = pyref.fft_inverse(c, pyref.bit_reverse(vals), "DIT", True)
    # the instance is satisfied exactly when T / Z_H is a polynomial of degree < 3 (n + 2)
    assert not any(h[3 * mm:]), "the instance is not satisfied: h = T / Z_H has degree >= 3 (n + 2)"
    sh = [h[k * mm:(k + 1) * mm] for k in range(3)]
    dl.update({"H%d" % k: at_tau(f) for k, f in enumerate(sh)})
    zeta = challenge(c, "zeta", dl["H0"], dl["H1"], dl["H2"])
    # evaluations and the linearised polynomial with the key's Qk
    le, re_, oe = (horner(r, t[k], zeta) for k in ("l", "r", "o"))
    s1e, s2e = horner(r, p["s1"], zeta), horner(r, p["s2"], zeta)
    wz = w * zeta % r
    zue = horner(r, t["z"], wz)
    qcpe = [horner(r, f, zeta) for f in qcp]
    zh = (pow(zeta, n, r) - 1) % r
    zm = pow(zeta, mm, r)
    a2l = alpha * alpha % r * zh % r * inv0(zeta - 1, r) % r * pow(n, -1, r) % r
    c1 = alpha * (le + beta * s1e + gamma) % r * (re_ + beta * s2e + gamma) % r * beta % r * zue % r
    c2 = -alpha * (le + beta * zeta + gamma) % r * (re_ + beta * g * zeta + gamma) % r * (oe + beta * g * g * zeta + gamma) % r
    lin = []
    for i in range(n + 3):
        x = (c2 + a2l) * t["z"][i]
        if i < n:
            x += c1 * p["s3"][i] + le * re_ * p["qm"][i] + le * p["ql"][i] + re_ * p["qr"][i] + oe * p["qo"][i] + p["qk"][i]
            x += sum(q * f[i] for q, f in zip(qcpe, pi2))
        if i < mm:
            x -= zh * (sh[0][i] + zm * sh[1][i] + zm * zm * sh[2][i])
        lin.append(x % r)
    claimed = [horner(r, lin, zeta), le, re_, oe, s1e, s2e] + qcpe
    dl["Hz"] = at_tau(quotient(r, t["z"], zue, wz))
    v = challenge(c, "v", at_tau(lin), *claimed, zue, dl["Hz"])
    polys = [lin, t["l"], t["r"], t["o"], p["s1"], p["s2"]] + qcp
    folded = fold(r, polys, v)
    fv = sum(pow(v, i, r) * x for i, x in enumerate(claimed)) % r
    assert fv == horner(r, folded, zeta)
    dl["Hb"] = at_tau(quotient(r, folded, fv, zeta))
    u = challenge(c, "u", v, u_seed)
    return types.SimpleNamespace(dl=[dl[k] for k in PROOF_POINTS] + bsb, values=claimed + [zue],
                                 publics=list(inst.public), hashed=list(inst.cvals),
                                 chal=[gamma, beta, alpha, zeta, v, u], bad_point=False, raw_points={})


@functools.lru_cache(maxsize=None)
def case(cname, n, nb, nb_public=2):
    """(instance, key, proof) of one curve and size, made once."""
    c = pyref.CURVES[cname]
    inst = SatInst(c, n, nb_public, nb, 0x9100 + 16 * n + nb)
    tau = tau_of(c, n)
    vk, proof = model_vk(inst, tau), model_prove(inst, tau)
    assert verify(c, vk, proof) == OK
    return inst, vk, proof


def clone(proof, **over):
    d = dict(dl=list(proof.dl), values=list(proof.values), publics=list(proof.publics), hashed=list(proof.hashed),
             chal=list(proof.chal), bad_point=proof.bad_point, raw_points=dict(proof.raw_points))
    d.update(over)
    return types.SimpleNamespace(**d)


def mutations(c, vk, proof):
    """[(name, mutated proof)]: every kind of bad proof of the batch test.  A bad
    point (off the curve, off the subgroup) is added by the GPU test, which has the
    bytes; here bad_point stands for it."""
    r, nb = c.r, len(vk.rows)
    out = []
    for k in range(9 + nb):
        d = list(proof.dl)
        d[k] = (d[k] + 1) % r
        out.append(("point %d replaced" % k, clone(proof, dl=d)))
    out.append(("bad point", clone(proof, bad_point=True)))
    for k in range(7 + nb):
        v = list(proof.values)
        v[k] = (v[k] + 1) % r
        out.append(("value %d + 1" % k, clone(proof, values=v)))
    for k in range(len(proof.publics)):
        v = list(proof.publics)
        v[k] = (v[k] + 1) % r
        out.append(("public %d + 1" % k, clone(proof, publics=v)))
    for k in range(nb):
        v = list(proof.hashed)
        v[k] = (v[k] + 1) % r
        out.append(("hashed_cmt %d + 1" % k, clone(proof, hashed=v)))
    for k, name in enumerate(CHALLENGES):
        v = list(proof.chal)
        v[k] = (v[k] + 1) % r
        out.append(("%s + 1" % name, clone(proof, chal=v)))
    out.append(("u = 0", clone(proof, chal=proof.chal[:5] + [0])))
    # the second opening alone is wrong: Hz moved, for two different u
    for u in (3, 0x1234567):
        d = list(proof.dl)
        d[8] = (d[8] + 5) % r
        out.append(("second opening wrong, u = %d" % u, clone(proof, dl=d, chal=proof.chal[:5] + [u])))
    return out


# ---------------------------------------------------------------------------
# bytes
# ---------------------------------------------------------------------------
def to_points(oracle, cname, dls):
    """[k] G for every k, as a list of gnark affine byte strings."""
    import gnark_mi355x as gm
    c = pyref.CURVES[cname]
    pb = gm.point_bytes(cname, False)
    b = oracle.batch_mul_base(cname, False, gm.generator(cname), enc(c, dls))
    return [bytes(b[i * pb:(i + 1) * pb]) for i in range(len(dls))]


def vk_bytes(oracle, cname, vk, tau_g2=None):
    """The dict gm.PlonkVk takes."""
    import gnark_mi355x as gm
    c = pyref.CURVES[cname]
    d = vk.dl
    pts = to_points(oracle, cname, [d[k] for k in KEY_POINTS] + list(d["qcp"]))
    out = dict(zip(KEY_POINTS, pts))
    out.update(n=vk.n, nb_public=vk.nb_public, qcp=b"".join(pts[8:]), commitment_row=list(vk.rows),
               kzg_g1=gm.generator(cname), kzg_g2_0=gm.generator(cname, True),
               kzg_g2_1=tau_g2 if tau_g2 is not None else g2_tau(cname, vk.tau))
    return out


@functools.lru_cache(maxsize=None)
def g2_tau(cname, tau):
    c = pyref.CURVES[cname]
    G2 = pyref.Group(c, True)
    return pyref.encode_point(c, G2.mul(G2.generator(), tau), True)


def batch_bytes(oracle, cname, proofs):
    """(points, values, publics, hashed_cmt, challenges) of a list of proofs; a proof's
    raw_points {index: bytes} replace the points made from its logarithms."""
    c = pyref.CURVES[cname]
    np_ = len(proofs[0].dl)
    pts = to_points(oracle, cname, [k for p in proofs for k in p.dl])
    for i, p in enumerate(proofs):
        for k, b in p.raw_points.items():
            pts[i * np_ + k] = b
    return (b"".join(pts), b"".join(enc_raw(c, p.values) for p in proofs),
            b"".join(enc_raw(c, p.publics) for p in proofs), b"".join(enc_raw(c, p.hashed) for p in proofs),
            b"".join(enc_raw(c, p.chal) for p in proofs))
