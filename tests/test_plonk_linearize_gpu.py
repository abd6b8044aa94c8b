"""gm_plonk_linearize: resident selectors, permutation values, Z and h in, the
evaluations at zeta, the linearized polynomial and the blinded wires out
(backend/plonk/bls12-377/prove.go computeLinearizedPolynomial /
innerComputeLinearizedPoly).

The expected values come from a model written here in Python integers from the
definition in include/gnark_mi355x.h: Horner evaluations, the six scalars, and
one sum per coefficient.  It knows nothing of the library's lazy sums, its
constants per edited coefficient or its launch geometry.
"""
import ctypes
import functools
import itertools
import random

import pytest

import pyref

pytestmark = pytest.mark.gpu

CURVES = ("bn254", "bls12377")
POLYS = ("ql", "qr", "qm", "qo", "qk", "s1", "s2", "s3", "l", "r", "o", "z")
BLINDS = (("l", "bl", 2), ("r", "br", 2), ("o", "bo", 2), ("z", "bz", 3))
BLINDED = ("l_blinded", "r_blinded", "o_blinded", "z_blinded")


# ---------------------------------------------------------------------------
# inputs and the model
# ---------------------------------------------------------------------------
class Inst:
    """One input of the call, as integers (canonical basis, regular order)."""

    def __init__(self, c, n, nb, seed, h_rand=False, zero=False):
        rng = random.Random(seed)
        rnd = (lambda k: [0] * k) if zero else (lambda k: [rng.randrange(c.r) for _ in range(k)])
        self.c, self.n, self.nb = c, n, nb
        self.p = {k: rnd(n) for k in POLYS}
        self.qcp = [rnd(n) for _ in range(nb)]
        self.pi2 = [rnd(n) for _ in range(nb)]
        self.b = {"bl": rnd(2), "br": rnd(2), "bo": rnd(2), "bz": rnd(3)}
        self.h = rnd(4 * n)
        self.h_rand = rnd(2) if h_rand else None
        # the challenges are never zero by default, also in an otherwise zero instance
        self.alpha, self.beta, self.gamma, self.zeta = (1 + rng.randrange(c.r - 1) for _ in range(4))


def horner(r, f, x):
    acc = 0
    for a in reversed(f):
        acc = (acc * x + a) % r
    return acc


def blinded(inst):
    """L~, R~, O~, Z~ = P + (X^n - 1) b as coefficient lists (getBlindedCoefficients)."""
    r, n = inst.c.r, inst.n
    out = {}
    for k, bk, _ in BLINDS:
        b = inst.b[bk]
        f = list(inst.p[k]) + [0] * len(b)
        for i, bi in enumerate(b):
            f[i] = (f[i] - bi) % r
            f[n + i] = bi
        out[k] = f
    return out


def scalars(inst):
    """The evaluations (in the order of `evals`) and the scalars of the combination."""
    c, r, n = inst.c, inst.c.r, inst.n
    g, w = c.coset_gen, pyref.domain_generator(c, n)
    al, be, ga, ze = inst.alpha, inst.beta, inst.gamma, inst.zeta
    zn = pow(ze, n, r)
    zh = (zn - 1) % r
    # evaluateBlinded: P(x) + (x^n - 1) b(x)
    evb = lambda k, bk, x: (horner(r, inst.p[k], x) + (pow(x, n, r) - 1) * horner(r, inst.b[bk], x)) % r
    le, re_, oe = evb("l", "bl", ze), evb("r", "br", ze), evb("o", "bo", ze)
    s1e, s2e = horner(r, inst.p["s1"], ze), horner(r, inst.p["s2"], ze)
    zue = evb("z", "bz", w * ze % r)
    qcpe = [horner(r, f, ze) for f in inst.qcp]
    inv0 = pow(ze - 1, -1, r) if (ze - 1) % r else 0
    s = {
        "rl": le * re_ % r,
        "c1": al * (le + be * s1e + ga) % r * (re_ + be * s2e + ga) % r * be % r * zue % r,
        "c2": -al * (le + be * ze + ga) % r * (re_ + be * g * ze + ga) % r * (oe + be * g * g * ze + ga) % r,
        "a2L": al * al % r * zh % r * inv0 % r * pow(n, -1, r) % r,
        "zm": pow(ze, n + 2, r),
        "zh": zh,
        "le": le, "re": re_, "oe": oe, "qcpe": qcpe,
    }
    return [le, re_, oe, s1e, s2e, zue] + qcpe, s


def model(inst):
    """(lin, evals, blinded coefficient lists) from the definition."""
    r, n = inst.c.r, inst.n
    m = n + 2
    evals, s = scalars(inst)
    bl = blinded(inst)
    zt, p, h = bl["z"], inst.p, inst.h
    zh, zm = s["zh"], s["zm"]
    lin = []
    for i in range(n + 3):
        t = (s["c2"] + s["a2L"]) * zt[i]
        if i < n:
            t += (s["c1"] * p["s3"][i] + s["rl"] * p["qm"][i] + s["le"] * p["ql"][i] + s["re"] * p["qr"][i]
                  + s["oe"] * p["qo"][i] + p["qk"][i])
            t += sum(q * f[i] for q, f in zip(s["qcpe"], inst.pi2))
        if i < m:
            t -= zh * (h[i] + zm * h[m + i] + zm * zm * h[2 * m + i])
        lin.append(t % r)
    if inst.h_rand:
        r0, r1 = inst.h_rand
        lin[0] = (lin[0] + zh * (zm * r0 + zm * zm * r1)) % r
        lin[m] = (lin[m] - zh * (r0 + zm * r1)) % r
    return lin, evals, bl


def model_by_shards(inst):
    """lin once more, with the h part as the reference's loop has it: the three
    shards h1', h2', h3' of prove.go:619-654 (StatisticalZK: h1' = h1 + rho0 X^m,
    h2' = h2 - rho0 + rho1 X^m, h3' = h3 - rho1) and its two branches on i."""
    r, n = inst.c.r, inst.n
    m = n + 2
    saved, inst.h_rand = inst.h_rand, None
    saved_h, inst.h = inst.h, [0] * (4 * n)
    try:
        lin, _, _ = model(inst)  # everything but h
    finally:
        inst.h_rand, inst.h = saved, saved_h
    _, s = scalars(inst)
    h1, h2, h3 = (list(inst.h[k * m:(k + 1) * m]) for k in range(3))
    if inst.h_rand:
        r0, r1 = inst.h_rand
        h1.append(r0)
        h2[0] = (h2[0] - r0) % r
        h2.append(r1)
        h3[0] = (h3[0] - r1) % r
    zm, zh = s["zm"], s["zh"]
    for i in range(n + 3):
        if i < len(h3):
            lin[i] = (lin[i] - ((h3[i] * zm + h2[i]) * zm + h1[i]) * zh) % r
        elif inst.h_rand:
            lin[i] = (lin[i] - (h2[i] * zm + h1[i]) * zh) % r
    return lin


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


class Dev:
    """inst on the device, with outputs; slack bytes behind every buffer."""

    def __init__(self, ctx, inst, slack=0):
        c, n = inst.c, inst.n
        self.ctx, self.inst = ctx, inst
        up = lambda vals: ctx.copy_to_device(enc(c, vals) + bytes(slack))
        self.p = {k: up(inst.p[k]) for k in POLYS}
        self.qcp = [up(f) for f in inst.qcp]
        self.pi2 = [up(f) for f in inst.pi2]
        self.h = up(inst.h)
        self.lin = ctx.malloc(32 * (n + 3) + slack)
        self.out = {k: ctx.malloc(32 * (n + (3 if k == "z_blinded" else 2)) + slack) for k in BLINDED}

    def inputs(self):
        return list(self.p.values()) + self.qcp + self.pi2 + [self.h]

    def free(self):
        for b in self.inputs() + [self.lin] + list(self.out.values()):
            b.free()

    def call(self, cname, **over):
        """The call as it should be made; `over` replaces arguments by name."""
        inst, c = self.inst, self.inst.c
        a = dict(n=inst.n, polys=self.p, qcp=self.qcp, pi2=self.pi2,
                 blinds={k: enc(c, v) for k, v in inst.b.items()}, h=self.h,
                 alpha=enc(c, [inst.alpha]), beta=enc(c, [inst.beta]), gamma=enc(c, [inst.gamma]),
                 zeta=enc(c, [inst.zeta]), lin=self.lin,
                 h_rand=enc(c, inst.h_rand) if inst.h_rand else None, blinded=self.out)
        a.update(over)
        return self.ctx.plonk_linearize(cname, **a)

    def results(self, evals):
        """(lin, evals, blinded) as the model returns them."""
        c, n = self.inst.c, self.inst.n
        bl = {k[0]: dec(c, self.out[k].to_host(32 * (n + (3 if k == "z_blinded" else 2)))) for k in BLINDED}
        return dec(c, self.lin.to_host(32 * (n + 3))), [dec(c, e)[0] for e in evals], bl


def run_device(ctx, cname, inst):
    d = Dev(ctx, inst)
    try:
        return d.results(d.call(cname))
    finally:
        d.free()


# ---------------------------------------------------------------------------
# 1. n = 8: every coefficient, every evaluation, every blinded output
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("h_rand", [False, True])
@pytest.mark.parametrize("nb", [0, 2])
@pytest.mark.parametrize("cname", CURVES)
def test_linearize_n8_against_the_integer_model(gm_ctx, cname, nb, h_rand):
    c = pyref.CURVES[cname]
    n = 8
    inst = Inst(c, n, nb, 0x7100 + 2 * nb + h_rand, h_rand)
    assert any(inst.h[3 * (n + 2):])  # the tail of h that is not read
    want_lin, want_ev, want_bl = model(inst)
    # the two StatisticalZK coefficients are the reference loop's
    assert want_lin == model_by_shards(inst)
    lin, ev, bl = run_device(gm_ctx, cname, inst)
    assert ev == want_ev
    assert len(lin) == n + 3
    assert lin[:n] == want_lin[:n]
    # the tail: more than a quarter of the work at this size
    assert lin[n] == want_lin[n], "coefficient n"
    assert lin[n + 1] == want_lin[n + 1], "coefficient n + 1"
    assert lin[n + 2] == want_lin[n + 2], "coefficient n + 2"
    for k in ("l", "r", "o", "z"):
        assert bl[k] == want_bl[k], k


# ---------------------------------------------------------------------------
# 2. launch geometry: n + 3 three coefficients past a block edge; 2^15
# ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def random_case(cname, n, nb):
    inst = Inst(pyref.CURVES[cname], n, nb, 0x7200 + n, True)
    return inst, model(inst)


def _sizes():
    import gnark_mi355x as gm
    # a lane owns one coefficient and the grid is not capped (csrc/plonk_lin.hpp): no
    # lane loops, so there is no size at which a lane takes a second iteration
    return [gm.PLONK_LIN_BLOCK, 1 << 15]


@pytest.mark.parametrize("which", [0, 1])
@pytest.mark.parametrize("cname", CURVES)
def test_linearize_block_edge_and_2p15(gm_ctx, cname, which):
    import gnark_mi355x as gm
    n = _sizes()[which]
    assert n % gm.PLONK_LIN_BLOCK == 0 and (n + 3) % gm.PLONK_LIN_BLOCK == 3
    inst, (want_lin, want_ev, want_bl) = random_case(cname, n, 1)
    lin, ev, bl = run_device(gm_ctx, cname, inst)
    assert ev == want_ev
    bad = [i for i in range(n + 3) if lin[i] != want_lin[i]]
    assert not bad, (len(bad), bad[:8])
    for k in ("l", "r", "o", "z"):
        bad = [i for i in range(len(want_bl[k])) if bl[k][i] != want_bl[k][i]]
        assert not bad and len(bl[k]) == len(want_bl[k]), (k, len(bad), bad[:8])


# ---------------------------------------------------------------------------
# 3. term isolation at n = 8
# ---------------------------------------------------------------------------
# the polynomials that enter lin by their coefficients, with the name of their scalar
STREAMS = ("z", "s3", "qm", "ql", "qr", "qo", "qk", "pi2", "h0", "h1", "h2")


def _stream_scalar(s, name):
    r_zh, zm = -s["zh"], s["zm"]
    return {"z": s["c2"] + s["a2L"], "s3": s["c1"], "qm": s["rl"], "ql": s["le"], "qr": s["re"], "qo": s["oe"],
            "qk": 1, "pi2": s["qcpe"][0], "h0": r_zh, "h1": r_zh * zm, "h2": r_zh * zm * zm}[name]


def _set_stream(inst, name, vals):
    """vals: n coefficients (m for an h shard, 4n - 3m for the tail of h)."""
    m = inst.n + 2
    if name in POLYS:
        inst.p[name] = vals
    elif name == "pi2":
        inst.pi2[0] = vals
    elif name == "qcp":
        inst.qcp[0] = vals
    elif name == "h_tail":
        inst.h[3 * m:] = vals
    else:
        k = int(name[1])
        inst.h[k * m:(k + 1) * m] = vals


@pytest.mark.parametrize("cname", CURVES)
@pytest.mark.parametrize("name", POLYS + ("qcp", "pi2", "h0", "h1", "h2", "h_tail"))
def test_linearize_one_input_alone(gm_ctx, cname, name):
    """Only `name` is non-zero; the blinds are zero.  lin is that input's term
    alone: scalar times coefficients for an input that enters by its coefficients
    (the scalar is often 0 then, its evaluations being 0), all zero for one that
    enters by its evaluation only."""
    c = pyref.CURVES[cname]
    r, n = c.r, 8
    m = n + 2
    inst = Inst(c, n, 1, 0x7300, zero=True)
    rng = random.Random(0x7301)
    vals = [1 + rng.randrange(r - 1) for _ in range({"h_tail": 4 * n - 3 * m}.get(name, m if name[0] == "h" else n))]
    _set_stream(inst, name, vals)
    _, s = scalars(inst)
    if name in STREAMS:
        k = _stream_scalar(s, name)
        want = [k * v % r for v in vals] + [0] * (n + 3 - len(vals))
        if name in ("z", "qk", "h0", "h1", "h2"):
            assert any(want), "this term does not vanish on its own"
    else:
        want = [0] * (n + 3)
    assert want == model(inst)[0]
    lin, _, _ = run_device(gm_ctx, cname, inst)
    assert lin == want, name


@pytest.mark.parametrize("cname", CURVES)
@pytest.mark.parametrize("name", STREAMS[1:])
def test_linearize_one_term_beside_z(gm_ctx, cname, name):
    """The polynomials that enter by their evaluations (l, r, o, s1, s2, z, qcp_0)
    are random, so every scalar is non-zero; of the others only `name` is
    non-zero, and the blinds are zero.  lin is the Z term and that one term: a
    swapped scalar or a wrong shard offset shows under the term's own name."""
    c = pyref.CURVES[cname]
    r, n = c.r, 8
    m = n + 2
    inst = Inst(c, n, 1, 0x7310, zero=True)
    rng = random.Random(0x7311)
    rnd = lambda k: [1 + rng.randrange(r - 1) for _ in range(k)]
    for k in ("l", "r", "o", "s1", "s2", "z", "qcp"):
        _set_stream(inst, k, rnd(n))
    vals = rnd(m if name[0] == "h" else n)
    _set_stream(inst, name, vals)
    _, s = scalars(inst)
    ks = {k: _stream_scalar(s, k) % r for k in STREAMS}
    assert all(ks.values()) and len(set(ks.values())) == len(STREAMS)
    want = [(ks["z"] * zi + ks[name] * v) % r
            for zi, v in zip(inst.p["z"] + [0] * 3, vals + [0] * (n + 3 - len(vals)))]
    assert want == model(inst)[0]
    lin, _, _ = run_device(gm_ctx, cname, inst)
    assert lin == want, name


# ---------------------------------------------------------------------------
# 4. zeta = 1, zeta on the domain, zeta = 0
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("n", [8, 1024])
@pytest.mark.parametrize("kind", ["one", "w3", "zero"])
@pytest.mark.parametrize("cname", CURVES)
def test_linearize_zeta_edge_cases(gm_ctx, cname, kind, n):
    c = pyref.CURVES[cname]
    r = c.r
    inst = Inst(c, n, 1, 0x7400 + n, True)
    inst.zeta = {"one": 1, "w3": pow(pyref.domain_generator(c, n), 3, r), "zero": 0}[kind]
    _, s = scalars(inst)
    if kind == "zero":
        assert s["zh"] == r - 1 and s["zm"] == 0 and s["a2L"] == pow(n, -1, r) * inst.alpha * inst.alpha % r
    else:
        # zh = 0: h and the blinds drop out of the values, and a2L = 0 (at zeta = 1 by inv0(0) = 0)
        assert s["zh"] == 0 and s["a2L"] == 0
    want_lin, want_ev, want_bl = model(inst)
    lin, ev, bl = run_device(gm_ctx, cname, inst)
    assert ev == want_ev
    assert lin == want_lin
    assert bl == want_bl


# ---------------------------------------------------------------------------
# 5. a satisfying instance: perm -> quotient -> linearize -> commit and openings
# ---------------------------------------------------------------------------
PERM_POLYS = ("l", "r", "o", "s1", "s2", "s3")


def canon_int(c, ev):
    """Lagrange regular -> canonical regular, integer inverse FFT."""
    return pyref.bit_reverse(pyref.fft_inverse(c, ev, "DIF"))


class Sat:
    """Multiplication gates l r = o with shared wires (a permutation that is not
    the identity), non-zero blinding: the Lagrange values for gm_plonk_perm_z and
    the canonical polynomials for the quotient and the linearization (the
    construction of test_plonk_perm_gpu.py)."""

    def __init__(self, c, n):
        r = c.r
        rng = random.Random(0x7500)
        g = c.coset_gen
        w = pyref.domain_generator(c, n)
        lv, rv, ov = [0] * n, [0] * n, [0] * n
        sigma = list(range(3 * n))  # wire column k, row i -> k n + i

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
        rnd = lambda m: [rng.randrange(r) for _ in range(m)]
        self.c, self.n = c, n
        self.b = {"bl": rnd(2), "br": rnd(2), "bo": rnd(2), "bz": rnd(3)}
        self.alpha, self.beta, self.gamma, self.zeta = rnd(4)
        self.lagrange = {"l": lv, "r": rv, "o": ov, "s1": s[:n], "s2": s[n:2 * n], "s3": s[2 * n:]}
        canon = lambda ev: canon_int(c, ev)
        # z comes from gm_plonk_perm_z
        self.p = {"ql": [0] * n, "qr": [0] * n, "qm": canon([1] * n), "qo": canon([r - 1] * n), "qk": [0] * n,
                  "s1": canon(s[:n]), "s2": canon(s[n:2 * n]), "s3": canon(s[2 * n:]),
                  "l": canon(lv), "r": canon(rv), "o": canon(ov)}


def _quotient(r, f, fz, z):
    """(f - f(z)) / (X - z) by synthetic division."""
    f = list(f)
    f[0] = (f[0] - fz) % r
    for i in range(len(f) - 2, -1, -1):
        f[i] = (f[i] + f[i + 1] * z) % r
    return f[1:]


def _fold(r, polys, gamma):
    out = [0] * max(len(f) for f in polys)
    gi = 1
    for f in polys:
        for j, a in enumerate(f):
            out[j] = (out[j] + gi * a) % r
        gi = gi * gamma % r
    return out


def test_linearize_of_a_satisfying_instance_closes_the_last_round(gm_ctx, oracle):
    import gnark_mi355x as gm
    cname, n = "bls12377", 64
    c = pyref.CURVES[cname]
    r = c.r
    sat = Sat(c, n)
    e1 = lambda v: enc(c, [v])
    blinds = {k: enc(c, v) for k, v in sat.b.items()}
    pb = gm.point_bytes(cname, False)
    bufs = []

    def keep(b):
        bufs.append(b)
        return b

    try:
        lag = {k: keep(gm_ctx.copy_to_device(enc(c, sat.lagrange[k]))) for k in PERM_POLYS}
        zl, zc, h = (keep(gm_ctx.malloc(32 * k)) for k in (n, n, 4 * n))
        q = {k: keep(gm_ctx.copy_to_device(enc(c, sat.p[k]))) for k in POLYS if k != "z"}
        q["z"] = zc
        lin = keep(gm_ctx.malloc(32 * (n + 3)))
        out = {k: keep(gm_ctx.malloc(32 * (n + (3 if k == "z_blinded" else 2)))) for k in BLINDED}
        # the three stages, each on the buffers where the one before left them
        gm_ctx.plonk_perm_z(cname, n, lag, e1(sat.beta), e1(sat.gamma), zl, zc)
        gm_ctx.plonk_quotient(cname, n, q, [], [], blinds, e1(sat.alpha), e1(sat.beta), e1(sat.gamma), h)
        hv = dec(c, h.to_host())
        assert not any(hv[3 * n + 6:]) and any(hv[2 * n + 4:3 * n + 6])  # the quotient of a satisfied instance
        evb = gm_ctx.plonk_linearize(cname, n, q, [], [], blinds, h, e1(sat.alpha), e1(sat.beta), e1(sat.gamma),
                                     e1(sat.zeta), lin, blinded=out)
        le, re_, oe, s1e, s2e, zue = (dec(c, e)[0] for e in evb)
        al, be, ga, ze = sat.alpha, sat.beta, sat.gamma, sat.zeta
        w = pyref.domain_generator(c, n)
        wze = w * ze % r
        zeb, wzeb = e1(ze), e1(wze)

        # the verifier's identity (verify.go:213-225; the public inputs are inside qk)
        lin_b = lin.to_host()
        lin_v = dec(c, lin_b)
        (lin_ze_b,) = gm_ctx.kzg_eval(cname, [lin], zeb, [n + 3])
        lin_ze = dec(c, lin_ze_b)[0]
        assert lin_ze == horner(r, lin_v, ze)
        l1 = (pow(ze, n, r) - 1) * pow(n * (ze - 1) % r, -1, r) % r
        assert lin_ze == -(al * (le + be * s1e + ga) % r * (re_ + be * s2e + ga) % r * (oe + ga) % r * zue
                           - al * al * l1) % r

        # the commit of lin over a canonical SRS of n + 3 points
        tau = pyref.random_scalars(c, 1, 0x7502)[0]
        points = oracle.batch_mul_base(cname, False, gm.generator(cname), enc(c, [pow(tau, i, r) for i in range(n + 3)]))
        srs = keep(gm_ctx.points_upload(cname, points))
        _, aff = gm_ctx.msm_prepared(cname, lin, srs, n + 3)
        assert aff == oracle.msm(cname, False, lin_b, points)

        # kzg.Open of the blinded Z at w zeta
        zt = dec(c, out["z_blinded"].to_host())
        zp = dec(c, zc.to_host())
        bz = sat.b["bz"]
        assert zt == [(a - b) % r for a, b in zip(zp, bz)] + zp[3:] + bz
        claimed, hpt = gm_ctx.kzg_open(cname, srs, out["z_blinded"], wzeb, n + 3)
        assert claimed == evb[5] and zue == horner(r, zt, wze)
        qz = _quotient(r, zt, zue, wze)
        assert hpt == oracle.msm(cname, False, enc(c, qz), points[:pb * len(qz)])

        # kzg.BatchOpenSinglePoint over [lin, l~, r~, o~, s1, s2] where they lie
        polys = [lin, out["l_blinded"], out["r_blinded"], out["o_blinded"], q["s1"], q["s2"]]
        lens = [n + 3, n + 2, n + 2, n + 2, n, n]
        ints = [lin_v] + [dec(c, b.to_host(32 * k)) for b, k in zip(polys[1:], lens[1:])]
        values = [lin_ze, le, re_, oe, s1e, s2e]
        assert values == [horner(r, f, ze) for f in ints]
        gamma = pyref.random_scalars(c, 1, 0x7503)[0]
        fv, hpt = gm_ctx.kzg_batch_open(cname, srs, polys, zeb, e1(gamma), lens)
        folded = sum(pow(gamma, i, r) * v for i, v in enumerate(values)) % r
        assert fv == e1(folded)
        qf = _quotient(r, _fold(r, ints, gamma), folded, ze)
        assert hpt == oracle.msm(cname, False, enc(c, qf), points[:pb * len(qf)])
    finally:
        for b in bufs:
            b.free()


# ---------------------------------------------------------------------------
# 6. inputs unchanged, repeatability, NULL blinded outputs, gm_trim
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("cname", CURVES)
def test_linearize_leaves_inputs_and_repeats(gm_ctx, cname):
    n = 1024
    inst, (want_lin, want_ev, want_bl) = random_case(cname, n, 1)
    c = inst.c
    d = Dev(gm_ctx, inst)
    try:
        first = d.results(d.call(cname))
        assert first == (want_lin, want_ev, want_bl)
        lin_b = d.lin.to_host()
        outs_b = {k: d.out[k].to_host() for k in BLINDED}
        for k in POLYS:
            assert d.p[k].to_host() == enc(c, inst.p[k]), k
        assert d.qcp[0].to_host() == enc(c, inst.qcp[0]) and d.pi2[0].to_host() == enc(c, inst.pi2[0])
        assert d.h.to_host() == enc(c, inst.h)
        # again, into cleared outputs
        d.lin.write(bytes(32 * (n + 3)))
        for k in BLINDED:
            d.out[k].write(bytes(len(outs_b[k])))
        ev = d.call(cname)
        assert d.lin.to_host() == lin_b and {k: d.out[k].to_host() for k in BLINDED} == outs_b
        assert [dec(c, e)[0] for e in ev] == want_ev
        # every subset of the blinded outputs: lin the same, the given ones written, the others untouched
        for mask in itertools.product([False, True], repeat=4):
            given = {k: d.out[k] for k, on in zip(BLINDED, mask) if on}
            d.lin.write(bytes(32 * (n + 3)))
            for k in BLINDED:
                d.out[k].write(b"\x5a" * len(outs_b[k]))
            assert d.call(cname, blinded=given or None) == ev
            assert d.lin.to_host() == lin_b, mask
            for k, on in zip(BLINDED, mask):
                assert d.out[k].to_host() == (outs_b[k] if on else b"\x5a" * len(outs_b[k])), (mask, k)
        gm_ctx.trim()
        d.lin.write(bytes(32 * (n + 3)))
        assert d.call(cname) == ev
        assert d.lin.to_host() == lin_b and {k: d.out[k].to_host() for k in BLINDED} == outs_b
    finally:
        d.free()


# ---------------------------------------------------------------------------
# 7. refusals: every one on the host, before a launch
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("cname", CURVES)
def test_linearize_refusals(gm_ctx, cname):
    import gnark_mi355x as gm
    c = pyref.CURVES[cname]
    n = 16
    inst = Inst(c, n, 1, 0x7700, True)
    # 32 bytes of slack, so that a pointer moved by 8 bytes still has its elements behind it
    d = Dev(gm_ctx, inst, slack=32)
    blinds = {k: enc(c, v) for k, v in inst.b.items()}
    mark = lambda b, byte: b.write(bytes([byte]) * b.nbytes)
    view = lambda b, off, elems: gm.DeviceBuffer(gm_ctx, b.ptr + off, 32 * elems)
    cases = {"n = 12": dict(n=12), "n = 4": dict(n=4)}
    for k in POLYS:
        cases["null " + k] = dict(polys=dict(d.p, **{k: None}))
    cases["null h"] = dict(h=None)
    cases["null lin"] = dict(lin=None)
    for k in blinds:
        cases["null " + k] = dict(blinds=dict(blinds, **{k: None}))
    for k in ("alpha", "beta", "gamma", "zeta"):
        cases["null " + k] = {k: None}
    cases.update({
        "nb_bsb = 1, null qcp table": dict(qcp=None),
        "nb_bsb = 1, null pi2 table": dict(pi2=None),
        "nb_bsb = 1, null qcp entry": dict(qcp=[None]),
        "nb_bsb = 1, null pi2 entry": dict(pi2=[None]),
        "qo off by 8": dict(polys=dict(d.p, qo=view(d.p["qo"], 8, n))),
        "pi2 off by 8": dict(pi2=[view(d.pi2[0], 8, n)]),
        "h off by 8": dict(h=view(d.h, 8, 4 * n)),
        "lin off by 8": dict(lin=view(d.lin, 8, n + 3)),
        "o_blinded off by 8": dict(blinded=dict(d.out, o_blinded=view(d.out["o_blinded"], 8, n + 2))),
        "lin overlapping z": dict(lin=view(d.p["z"], 0, n)),
        "lin overlapping h": dict(lin=view(d.h, 32 * (4 * n - 1), 1)),
        "lin overlapping qcp": dict(lin=view(d.qcp[0], 0, n)),
        "z_blinded overlapping lin": dict(blinded=dict(d.out, z_blinded=view(d.lin, 32 * (n + 2), 1))),
        "l_blinded overlapping r_blinded": dict(blinded=dict(d.out, l_blinded=view(d.out["r_blinded"], 32, n))),
        "r_blinded overlapping s1": dict(blinded=dict(d.out, r_blinded=view(d.p["s1"], 32 * (n - 1), 1))),
    })
    try:
        outs = [d.lin] + list(d.out.values())
        for b in outs:
            mark(b, 0xa5)
        snapshot = [b.to_host() for b in d.inputs()]
        for name, over in cases.items():
            with pytest.raises(gm.GmError) as e:
                d.call(cname, **over)
            # GM_ERR_INVALID, with this call's own message
            assert "error -1: plonk linearize" in str(e.value), name
            assert all(b.to_host() == b"\xa5" * b.nbytes for b in outs), name
            assert [b.to_host() for b in d.inputs()] == snapshot, name
        # a NULL evals, through the structs themselves
        a, o = gm._PlonkLinearizeIn(), gm._PlonkLinearizeOut()
        a.n = n
        for k in POLYS:
            setattr(a, k, d.p[k].ptr)
        a.nb_bsb = 0
        keep = {k: gm._buf(v) for k, v in dict(blinds, alpha=enc(c, [inst.alpha]), beta=enc(c, [inst.beta]),
                                               gamma=enc(c, [inst.gamma]), zeta=enc(c, [inst.zeta])).items()}
        for k, v in keep.items():
            setattr(a, k, v.ctypes.data)
        a.h, o.lin, o.evals = d.h.ptr, d.lin.ptr, None
        L = gm.load_library()
        assert L.gm_plonk_linearize(gm_ctx.handle, gm.curve_id(cname), ctypes.byref(a), ctypes.byref(o)) == -1
        assert L.gm_last_error().decode().startswith("plonk linearize")
        assert all(b.to_host() == b"\xa5" * b.nbytes for b in outs)
        # and the call as it should be made, on the same context
        got = d.results(d.call(cname))
        assert got == model(inst)
    finally:
        d.free()
