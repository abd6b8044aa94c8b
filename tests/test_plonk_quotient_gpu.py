"""gm_plonk_quotient: resident polynomials in, h out (backend/plonk/bls12-377/
prove.go computeNumerator + divideByZH).

The expected h comes from models written here from the definition in
include/gnark_mi355x.h, not from the library's steps (which work coset by coset
of the n domain with the blinding added per point):

  * model_int   everything in Python integers: Horner evaluation of the blinded
                polynomials at the 4n points g w1^k, T / Z_H per point, a naive
                inverse DFT on the coset.  O(n^2): n = 8 only.
  * model_fft   the blinded polynomials, zero-padded to 4n, go through ONE
                forward coset FFT of size 4n each (oracle.fft), T / Z_H per point
                in Python integers (L1 by a modular inversion per point), and the
                oracle's inverse coset FFT.  At n = 8 it is first checked against
                model_int, so the model itself is pinned.
"""
import random

import pytest

import pyref

pytestmark = pytest.mark.gpu

CURVES = ("bn254", "bls12377")
POLYS = ("ql", "qr", "qm", "qo", "qk", "s1", "s2", "s3", "l", "r", "o", "z")


# ---------------------------------------------------------------------------
# inputs and models
# ---------------------------------------------------------------------------
class Inst:
    """One input of the quotient, as integers."""

    def __init__(self, c, n, nb, seed):
        rng = random.Random(seed)
        rnd = lambda m: [rng.randrange(c.r) for _ in range(m)]
        self.c, self.n = c, n
        self.p = {k: rnd(n) for k in POLYS}
        self.qcp = [rnd(n) for _ in range(nb)]
        self.pi2 = [rnd(n) for _ in range(nb)]
        self.bl, self.br, self.bo, self.bz = rnd(2), rnd(2), rnd(2), rnd(3)
        self.alpha, self.beta, self.gamma = rnd(3)


def _blinded(inst):
    """L~, R~, O~, Z~ = P + (X^n - 1) b as coefficient lists."""
    r, n = inst.c.r, inst.n
    out = {}
    for k, b in (("l", inst.bl), ("r", inst.br), ("o", inst.bo), ("z", inst.bz)):
        f = list(inst.p[k]) + [0] * len(b)
        for i, bi in enumerate(b):
            f[i] = (f[i] - bi) % r
            f[n + i] = (f[n + i] + bi) % r
        out[k] = f
    return out


def _domain(inst):
    c, n = inst.c, inst.n
    w1 = pyref.domain_generator(c, 4 * n)
    assert pow(w1, 4, c.r) == pyref.domain_generator(c, n)
    return c.coset_gen, w1


def _t_over_zh(inst, x, v, zs):
    """T(x) / Z_H(x) from the values v[name] of the (blinded) polynomials at x,
    zs = Z~(w0 x); qcp / pi2 values under v['qcp'], v['pi2']."""
    r, n = inst.c.r, inst.n
    g = inst.c.coset_gen
    a, b, gm_ = inst.alpha, inst.beta, inst.gamma
    L, R, O, Z = v["l"], v["r"], v["o"], v["z"]
    t = v["ql"] * L + v["qr"] * R + v["qm"] * L * R + v["qo"] * O + v["qk"]
    t += sum(q * p for q, p in zip(v["qcp"], v["pi2"]))
    t += a * ((L + b * v["s1"] + gm_) * (R + b * v["s2"] + gm_) * (O + b * v["s3"] + gm_) * zs
              - (L + b * x + gm_) * (R + b * g * x + gm_) * (O + b * g * g * x + gm_) * Z)
    zh = (pow(x, n, r) - 1) % r
    l1 = zh * pow(n * (x - 1) % r, -1, r)
    t += a * a * (Z - 1) * l1
    return t % r * pow(zh, -1, r) % r


def _horner(r, f, x):
    acc = 0
    for a in reversed(f):
        acc = (acc * x + a) % r
    return acc


def model_int(inst):
    r, n = inst.c.r, inst.n
    g, w1 = _domain(inst)
    w0 = pow(w1, 4, r)
    bl = _blinded(inst)
    polys = {k: bl.get(k, inst.p[k]) for k in POLYS}
    m = 4 * n
    vals = []
    for k in range(m):
        x = g * pow(w1, k, r) % r
        v = {name: _horner(r, f, x) for name, f in polys.items()}
        v["qcp"] = [_horner(r, f, x) for f in inst.qcp]
        v["pi2"] = [_horner(r, f, x) for f in inst.pi2]
        vals.append(_t_over_zh(inst, x, v, _horner(r, polys["z"], w0 * x % r)))
    # v_k = sum_j h_j g^j w1^(jk)  =>  h_j = g^-j / m  sum_k v_k w1^(-jk)
    w1i, gi, mi = pow(w1, -1, r), pow(g, -1, r), pow(m, -1, r)
    return [sum(vk * pow(w1i, j * k, r) for k, vk in enumerate(vals)) * pow(gi, j, r) * mi % r for j in range(m)]


def model_fft(inst, oracle, cname):
    c, r, n = inst.c, inst.c.r, inst.n
    g, w1 = _domain(inst)
    m, logm = 4 * n, (4 * n).bit_length() - 1
    enc = lambda vals: b"".join(pyref.encode_fr(c, v) for v in vals)
    dec = lambda b: [pyref.decode_fr(c, b[32 * i:32 * i + 32]) for i in range(len(b) // 32)]
    br = [pyref.bitrev(k, logm) for k in range(m)]

    def evals(f):  # natural order: value at g w1^k
        e = dec(oracle.fft(cname, enc(list(f) + [0] * (m - len(f))), False, False, True))
        return [e[br[k]] for k in range(m)]

    bl = _blinded(inst)
    ev = {k: evals(bl.get(k, inst.p[k])) for k in POLYS}
    eq = [evals(f) for f in inst.qcp]
    ep = [evals(f) for f in inst.pi2]
    vals = []
    x = g
    for k in range(m):
        v = {name: e[k] for name, e in ev.items()}
        v["qcp"] = [e[k] for e in eq]
        v["pi2"] = [e[k] for e in ep]
        vals.append(_t_over_zh(inst, x, v, ev["z"][(k + 4) % m]))  # w0 = w1^4
        x = x * w1 % r
    # FFTInverse(DIT, OnCoset): bit-reversed in, canonical regular out
    return dec(oracle.fft(cname, enc([vals[br[k]] for k in range(m)]), True, True, True))


def run_device(ctx, cname, inst, h=None):
    """Uploads inst, runs the call, returns h as integers and as bytes."""
    c, n = inst.c, inst.n
    enc = lambda vals: b"".join(pyref.encode_fr(c, v) for v in vals)
    bufs = {k: ctx.copy_to_device(enc(inst.p[k])) for k in POLYS}
    qcp = [ctx.copy_to_device(enc(f)) for f in inst.qcp]
    pi2 = [ctx.copy_to_device(enc(f)) for f in inst.pi2]
    own = h is None
    if own:
        h = ctx.malloc(32 * 4 * n)
    try:
        call_device(ctx, cname, inst, bufs, qcp, pi2, h)
        hb = h.to_host(32 * 4 * n)
        return [pyref.decode_fr(c, hb[32 * i:32 * i + 32]) for i in range(4 * n)], hb
    finally:
        for b in list(bufs.values()) + qcp + pi2 + ([h] if own else []):
            b.free()


def call_device(ctx, cname, inst, bufs, qcp, pi2, h, n=None):
    c = inst.c
    enc = lambda vals: b"".join(pyref.encode_fr(c, v) for v in vals)
    blinds = {"bl": enc(inst.bl), "br": enc(inst.br), "bo": enc(inst.bo), "bz": enc(inst.bz)}
    ctx.plonk_quotient(cname, inst.n if n is None else n, bufs, qcp, pi2, blinds, enc([inst.alpha]),
                       enc([inst.beta]), enc([inst.gamma]), h)


# ---------------------------------------------------------------------------
# 1. random inputs, all 4n elements of h
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("cname", CURVES)
@pytest.mark.parametrize("nb", [0, 2])
def test_quotient_n8_against_the_integer_model(gm_ctx, oracle, cname, nb):
    """n = 8: both NTT sizes are single-pass and Z(w0 x) wraps inside one block."""
    c = pyref.CURVES[cname]
    inst = Inst(c, 8, nb, 0x5100 + nb)
    want = model_int(inst)
    assert model_fft(inst, oracle, cname) == want  # pins the model of the larger cases
    assert any(want[3 * 8 + 6:])  # random inputs are not divisible by Z_H: every coefficient is reached
    got, _ = run_device(gm_ctx, cname, inst)
    assert got == want


@pytest.mark.parametrize("cname", CURVES)
@pytest.mark.parametrize("n,nb", [(128, 0), (128, 2), (1024, 0), (1024, 2)])
def test_quotient_against_the_fft_model(gm_ctx, oracle, cname, n, nb):
    """n = 128: the n transform is single-pass, the 4n one two-pass; n = 1024: both
    multi-pass and the constraint kernel spans several blocks."""
    c = pyref.CURVES[cname]
    inst = Inst(c, n, nb, 0x5200 + n + nb)
    want = model_fft(inst, oracle, cname)
    got, _ = run_device(gm_ctx, cname, inst)
    assert got == want


# ---------------------------------------------------------------------------
# 2. term isolation at n = 8
# ---------------------------------------------------------------------------
def _isolate(inst, case):
    n = inst.n
    if case == "alpha0":
        inst.alpha = 0
    elif case == "beta0":
        inst.beta = 0
    elif case == "no_blinding":
        inst.bl, inst.br, inst.bo, inst.bz = [0, 0], [0, 0], [0, 0], [0, 0, 0]
    elif case == "bz_only":  # the blinding of Z at w0 x
        inst.bl, inst.br, inst.bo = [0, 0], [0, 0], [0, 0]
    elif case == "z_delta_last":  # Z(w0 x) of the last index wraps to index 0
        ninv = pow(n, -1, inst.c.r)
        w = pyref.domain_generator(inst.c, n)
        # canonical coefficients of the Lagrange delta at index n - 1
        inst.p["z"] = [ninv * pow(w, -(n - 1) * k, inst.c.r) % inst.c.r for k in range(n)]
    return inst


@pytest.mark.parametrize("cname", CURVES)
@pytest.mark.parametrize("case", ["alpha0", "beta0", "no_blinding", "bz_only", "z_delta_last"])
def test_quotient_term_isolation(gm_ctx, cname, case):
    c = pyref.CURVES[cname]
    inst = _isolate(Inst(c, 8, 1, 0x5300), case)
    want = model_int(inst)
    got, _ = run_device(gm_ctx, cname, inst)
    assert got == want


# ---------------------------------------------------------------------------
# 3. a satisfying instance
# ---------------------------------------------------------------------------
def _poly_mul(r, a, b):
    out = [0] * (len(a) + len(b) - 1)
    for i, x in enumerate(a):
        if x:
            for j, y in enumerate(b):
                out[i + j] = (out[i + j] + x * y) % r
    return out


def _poly_add(r, a, b, sign=1):
    m = max(len(a), len(b))
    a, b = list(a) + [0] * (m - len(a)), list(b) + [0] * (m - len(b))
    return [(x + sign * y) % r for x, y in zip(a, b)]


def _satisfying(c, n):
    """Multiplication gates l r = o with shared wires (a permutation that is not
    the identity), Z by the running product, non-zero blinding.  Lagrange values
    -> canonical coefficients with the integer inverse FFT."""
    r = c.r
    rng = random.Random(0x5400)
    g = c.coset_gen
    w = pyref.domain_generator(c, n)
    # wire values: gate i multiplies l_i r_i = o_i; r_i of odd gates repeats the
    # previous gate's output, l_i of every fourth gate repeats l_0
    lv, rv, ov = [0] * n, [0] * n, [0] * n
    # positions: wire column k, row i -> k n + i
    sigma = list(range(3 * n))

    def tie(a, b):  # merge the cycles of a and b
        sigma[a], sigma[b] = sigma[b], sigma[a]

    for i in range(n):
        lv[i] = rng.randrange(r)
        rv[i] = rng.randrange(r)
        if i % 2 == 1:
            rv[i] = ov[i - 1]
            tie(n + i, 2 * n + i - 1)
        if i % 4 == 0 and i:
            lv[i] = lv[0]
            tie(i, 0)
        ov[i] = lv[i] * rv[i] % r
    assert sigma != list(range(3 * n))
    vals = lv + rv + ov
    assert all(vals[sigma[k]] == vals[k] for k in range(3 * n))
    ids = [pow(w, i, r) for i in range(n)] + [g * pow(w, i, r) % r for i in range(n)] + \
          [g * g * pow(w, i, r) % r for i in range(n)]
    s = [ids[sigma[k]] for k in range(3 * n)]
    inst = Inst(c, n, 0, 0x5401)  # blinding and challenges from here
    be, ga = inst.beta, inst.gamma
    z = [1] * n
    for i in range(n - 1):
        num = den = 1
        for col, wv in enumerate((lv, rv, ov)):
            num = num * (wv[i] + be * ids[col * n + i] + ga) % r
            den = den * (wv[i] + be * s[col * n + i] + ga) % r
        z[i + 1] = z[i] * num * pow(den, -1, r) % r
    canon = lambda ev: pyref.bit_reverse(pyref.fft_inverse(c, ev, "DIF"))  # Lagrange regular -> canonical regular
    inst.p = {"ql": [0] * n, "qr": [0] * n, "qm": canon([1] * n), "qo": canon([r - 1] * n), "qk": [0] * n,
              "s1": canon(s[:n]), "s2": canon(s[n:2 * n]), "s3": canon(s[2 * n:]),
              "l": canon(lv), "r": canon(rv), "o": canon(ov), "z": canon(z)}
    return inst


def _numerator_poly(inst):
    """T as a coefficient list, by integer polynomial arithmetic."""
    c, r, n = inst.c, inst.c.r, inst.n
    g = c.coset_gen
    w0 = pyref.domain_generator(c, n)
    bl = _blinded(inst)
    P = {k: bl.get(k, inst.p[k]) for k in POLYS}
    mul = lambda a, b: _poly_mul(r, a, b)
    add = lambda a, b: _poly_add(r, a, b)
    sc = lambda k, a: [k * x % r for x in a]
    L, R, O, Z = P["l"], P["r"], P["o"], P["z"]
    t = add(add(mul(P["ql"], L), mul(P["qr"], R)), add(mul(mul(P["qm"], L), R), add(mul(P["qo"], O), P["qk"])))
    be, ga, al = inst.beta, inst.gamma, inst.alpha
    zs = [x * pow(w0, k, r) % r for k, x in enumerate(Z)]
    f1 = mul(mul(add(add(L, sc(be, P["s1"])), [ga]), add(add(R, sc(be, P["s2"])), [ga])),
             mul(add(add(O, sc(be, P["s3"])), [ga]), zs))
    f2 = mul(mul(add(L, [ga, be]), add(R, [ga, be * g % r])), mul(add(O, [ga, be * g * g % r]), Z))
    t = add(t, sc(al, _poly_add(r, f1, f2, -1)))
    l1 = [pow(n, -1, r)] * n
    t = add(t, sc(al * al % r, mul(_poly_add(r, Z, [1], -1), l1)))
    return t


def test_quotient_of_a_satisfying_instance(gm_ctx, oracle):
    import gnark_mi355x as gm
    cname, n = "bls12377", 64
    c = pyref.CURVES[cname]
    r = c.r
    inst = _satisfying(c, n)
    h = gm_ctx.malloc(32 * 4 * n)
    srs = None
    try:
        got, hb = run_device(gm_ctx, cname, inst, h=h)
        assert not any(got[3 * n + 6:])
        assert any(got[2 * n + 4:3 * n + 6])
        # h (X^n - 1) == T, coefficient for coefficient
        t = _numerator_poly(inst)
        hz = _poly_add(r, [0] * n + got[:3 * n + 6], got[:3 * n + 6], -1)
        m = max(len(t), len(hz))
        assert hz + [0] * (m - len(hz)) == t + [0] * (m - len(t))
        # the commit reads h1, h2, h3 where they lie
        enc = lambda vals: b"".join(pyref.encode_fr(c, v) for v in vals)
        tau = pyref.random_scalars(c, 1, 0x5402)[0]
        canon = oracle.batch_mul_base(cname, False, gm.generator(cname), enc([pow(tau, i, r) for i in range(n + 2)]))
        srs = gm_ctx.points_upload(cname, canon)
        for i in range(3):
            part = gm.DeviceBuffer(gm_ctx, h.ptr + 32 * i * (n + 2), 32 * (n + 2))
            _, aff = gm_ctx.msm_prepared(cname, part, srs, n + 2)
            assert aff == oracle.msm(cname, False, hb[32 * i * (n + 2):32 * (i + 1) * (n + 2)], canon), i
    finally:
        h.free()
        if srs is not None:
            srs.free()


# ---------------------------------------------------------------------------
# 4. inputs unchanged, repeatability, gm_trim
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("cname", CURVES)
def test_quotient_leaves_inputs_and_repeats(gm_ctx, cname):
    c = pyref.CURVES[cname]
    n = 128
    inst = Inst(c, n, 1, 0x5500)
    enc = lambda vals: b"".join(pyref.encode_fr(c, v) for v in vals)
    bufs = {k: gm_ctx.copy_to_device(enc(inst.p[k])) for k in POLYS}
    qcp = [gm_ctx.copy_to_device(enc(f)) for f in inst.qcp]
    pi2 = [gm_ctx.copy_to_device(enc(f)) for f in inst.pi2]
    h = gm_ctx.malloc(32 * 4 * n)
    try:
        call_device(gm_ctx, cname, inst, bufs, qcp, pi2, h)
        first = h.to_host()
        for k in ("ql", "s1", "l", "z"):  # one buffer of each role
            assert bufs[k].to_host() == enc(inst.p[k]), k
        assert qcp[0].to_host() == enc(inst.qcp[0]) and pi2[0].to_host() == enc(inst.pi2[0])
        h.write(bytes(32 * 4 * n))
        call_device(gm_ctx, cname, inst, bufs, qcp, pi2, h)
        assert h.to_host() == first
        gm_ctx.trim()
        h.write(bytes(32 * 4 * n))
        call_device(gm_ctx, cname, inst, bufs, qcp, pi2, h)
        assert h.to_host() == first
    finally:
        for b in list(bufs.values()) + qcp + pi2 + [h]:
            b.free()


# ---------------------------------------------------------------------------
# 5. refusals
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("cname", CURVES)
def test_quotient_refusals(gm_ctx, cname):
    import gnark_mi355x as gm
    c = pyref.CURVES[cname]
    n = 16
    inst = Inst(c, n, 1, 0x5600)
    enc = lambda vals: b"".join(pyref.encode_fr(c, v) for v in vals)
    bufs = {k: gm_ctx.copy_to_device(enc(inst.p[k])) for k in POLYS}
    qcp = [gm_ctx.copy_to_device(enc(f)) for f in inst.qcp]
    pi2 = [gm_ctx.copy_to_device(enc(f)) for f in inst.pi2]
    h = gm_ctx.malloc(32 * 4 * n)
    try:
        for bad_n in (4, 12):
            with pytest.raises(gm.GmError):
                call_device(gm_ctx, cname, inst, bufs, qcp, pi2, h, n=bad_n)
        with pytest.raises(gm.GmError):  # h aliasing z
            call_device(gm_ctx, cname, inst, bufs, qcp, pi2, gm.DeviceBuffer(gm_ctx, bufs["z"].ptr, 32 * n))
        with pytest.raises(gm.GmError):  # nb_bsb = 1 with a NULL qcp table
            call_device(gm_ctx, cname, inst, bufs, None, pi2, h)
        call_device(gm_ctx, cname, inst, bufs, qcp, pi2, h)
        hb = h.to_host()
        assert [pyref.decode_fr(c, hb[32 * i:32 * i + 32]) for i in range(4 * n)] == model_int(inst)
    finally:
        for b in list(bufs.values()) + qcp + pi2 + [h]:
            b.free()
