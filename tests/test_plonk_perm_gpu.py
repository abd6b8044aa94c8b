"""gm_plonk_perm_z: resident wires and permutation values in, the copy-constraint
accumulator Z out (backend/plonk/bls12-377/prove.go buildRatioCopyConstraint).

The expected Z comes from a model written here in Python integers from the
definition in include/gnark_mi355x.h: running products of the numerators and
denominators and one pow(D, -1, r) per row (inv0: a zero D gives 0).  It knows
nothing of the library's chunks, carries or its single inversion.
"""
import functools
import random

import pytest

import pyref

pytestmark = pytest.mark.gpu

CURVES = ("bn254", "bls12377")
POLYS = ("l", "r", "o", "s1", "s2", "s3")


# ---------------------------------------------------------------------------
# inputs and the model
# ---------------------------------------------------------------------------
class Inst:
    """One input of the call, as integers (Lagrange values, regular order)."""

    def __init__(self, c, n, seed):
        rng = random.Random(seed)
        self.c, self.n = c, n
        self.p = {k: [rng.randrange(c.r) for _ in range(n)] for k in POLYS}
        self.beta, self.gamma = rng.randrange(c.r), rng.randrange(c.r)


def factors(inst):
    """(num_i, den_i) for every row i < n, from the definition."""
    c, r, n = inst.c, inst.c.r, inst.n
    g, w = c.coset_gen, pyref.domain_generator(c, n)
    be, ga = inst.beta, inst.gamma
    p = inst.p
    num, den = [], []
    x = 1
    for i in range(n):
        num.append((p["l"][i] + be * x + ga) * (p["r"][i] + be * g * x + ga) % r
                   * (p["o"][i] + be * g * g * x + ga) % r)
        den.append((p["l"][i] + be * p["s1"][i] + ga) * (p["r"][i] + be * p["s2"][i] + ga) % r
                   * (p["o"][i] + be * p["s3"][i] + ga) % r)
        x = x * w % r
    return num, den


def products(inst):
    """The running products N_i, D_i for i < n - 1."""
    r, n = inst.c.r, inst.n
    num, den = factors(inst)
    N, D = [], []
    a = b = 1
    for i in range(n - 1):
        a, b = a * num[i] % r, b * den[i] % r
        N.append(a)
        D.append(b)
    return N, D


def model(inst):
    """Z, and the running products it was built from: one inversion per row."""
    r = inst.c.r
    N, D = products(inst)
    return [1] + [a * pow(b, -1, r) % r if b else 0 for a, b in zip(N, D)], N, D


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


def canon_int(c, ev):
    """Lagrange regular -> canonical regular, integer inverse FFT."""
    return pyref.bit_reverse(pyref.fft_inverse(c, ev, "DIF"))


def canon_oracle(oracle, cname, ev):
    """The same through the oracle's inverse FFT (the larger sizes)."""
    c = pyref.CURVES[cname]
    return pyref.bit_reverse(dec(c, oracle.fft(cname, enc(c, ev), True, False, False)))


def upload(ctx, inst):
    return {k: ctx.copy_to_device(enc(inst.c, inst.p[k])) for k in POLYS}


def call_device(ctx, cname, inst, bufs, zl, zc, n=None):
    c = inst.c
    ctx.plonk_perm_z(cname, inst.n if n is None else n, bufs, enc(c, [inst.beta]), enc(c, [inst.gamma]), zl, zc)


def run_device(ctx, cname, inst, canonical=True):
    """Uploads inst, runs the call, returns (Z Lagrange, Z canonical or None) as integers."""
    c, n = inst.c, inst.n
    bufs = upload(ctx, inst)
    zl = ctx.malloc(32 * n)
    zc = ctx.malloc(32 * n) if canonical else None
    try:
        call_device(ctx, cname, inst, bufs, zl, zc)
        return dec(c, zl.to_host()), (dec(c, zc.to_host()) if canonical else None)
    finally:
        for b in list(bufs.values()) + [zl] + ([zc] if canonical else []):
            b.free()


@functools.lru_cache(maxsize=None)
def random_case(cname, n):
    """A random input and its model, computed once per size."""
    inst = Inst(pyref.CURVES[cname], n, 0x6100 + n)
    return inst, model(inst)


def test_enc_dec_are_pyref_s():
    for cname in CURVES:
        c = pyref.CURVES[cname]
        vals = [0, 1, c.r - 1, 0x1234567 << 200]
        assert enc(c, vals) == b"".join(pyref.encode_fr(c, v) for v in vals)
        assert dec(c, enc(c, vals)) == vals == [pyref.decode_fr(c, pyref.encode_fr(c, v)) for v in vals]


# ---------------------------------------------------------------------------
# 1. n = 8, every value of both outputs
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("cname", CURVES)
def test_perm_n8_against_the_integer_model(gm_ctx, cname):
    c = pyref.CURVES[cname]
    inst, (want, _, D) = random_case(cname, 8)
    assert all(D)
    zl, zc = run_device(gm_ctx, cname, inst)
    assert zl == want
    assert zc == canon_int(c, want)


# ---------------------------------------------------------------------------
# 2. one chunk, two chunks, two tiles of the carry scan
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("cname", CURVES)
@pytest.mark.parametrize("chunks", [1, 2])
def test_perm_one_and_two_chunks(gm_ctx, oracle, cname, chunks):
    """n - 1 rows: n = one chunk fills it short of a row, n = two chunks needs
    both.  Every element of Z against the model, and the canonical form against
    the inverse FFT of the model's Z."""
    import gnark_mi355x as gm
    n = chunks * gm.PLONK_PERM_CHUNK
    inst, (want, N, D) = random_case(cname, n)
    assert all(D) and all(N)  # random inputs: no zero factor anywhere
    zl, zc = run_device(gm_ctx, cname, inst)
    bad = [i for i in range(n) if zl[i] != want[i]]
    assert not bad, (len(bad), bad[:8])
    assert zc == canon_oracle(oracle, cname, want)


@pytest.mark.parametrize("cname", CURVES)
def test_perm_two_carry_tiles(gm_ctx, oracle, cname):
    """The smallest n whose chunks span two tiles of the carry scan.  n
    inversions would take seconds here, so every row is checked as
    Z[i+1] D_i == N_i with the model's own products and D_i != 0 (which pins
    Z[i+1], a reduced value, to N_i / D_i), and the first and last 64 rows of every
    chunk with the inverse itself."""
    import gnark_mi355x as gm
    chunk, tile = gm.PLONK_PERM_CHUNK, gm.PLONK_PERM_CARRY_TILE
    n = 2 * tile * chunk
    assert n <= 1 << 17 and (n - 1 + chunk - 1) // chunk > tile
    c = pyref.CURVES[cname]
    r = c.r
    inst = Inst(c, n, 0x6200)
    N, D = products(inst)
    assert all(D) and all(N)
    zl, zc = run_device(gm_ctx, cname, inst)
    assert zl[0] == 1
    bad = [i for i in range(n - 1) if zl[i + 1] * D[i] % r != N[i]]
    assert not bad, (len(bad), bad[:8])
    for i in range(n - 1):
        if i % chunk < 64 or i % chunk >= chunk - 64:
            assert zl[i + 1] == N[i] * pow(D[i], -1, r) % r, i
    # zl is the model's Z by the above
    assert zc == canon_oracle(oracle, cname, zl)


# ---------------------------------------------------------------------------
# 3. zero denominators and numerators (inv0)
# ---------------------------------------------------------------------------
def _zero_rows():
    import gnark_mi355x as gm
    e, chunk = gm.PLONK_PERM_E, gm.PLONK_PERM_CHUNK
    # the second-to-last row of a run inside the first chunk; the rows either side
    # of the chunk edge; a row of the second chunk
    return [37 * e + e - 2, chunk - 1, chunk, chunk + 5 * e + 1]


@pytest.mark.parametrize("cname", CURVES)
@pytest.mark.parametrize("kind", ["den", "num"])
@pytest.mark.parametrize("which", [0, 1, 2, 3])
def test_perm_zero_factor(gm_ctx, cname, kind, which):
    """gamma chosen so that one factor of den_j (of num_j) is zero at exactly one
    row j: Z[i] is the model's for i <= j and 0 for i > j."""
    import gnark_mi355x as gm
    c = pyref.CURVES[cname]
    r = c.r
    n = 2 * gm.PLONK_PERM_CHUNK
    j = _zero_rows()[which]
    assert j < n - 1
    inst = Inst(c, n, 0x6300 + which)
    if kind == "den":
        inst.gamma = -(inst.p["l"][j] + inst.beta * inst.p["s1"][j]) % r
    else:
        inst.gamma = -(inst.p["l"][j] + inst.beta * pow(pyref.domain_generator(c, n), j, r)) % r
    num, den = factors(inst)
    zeros = [i for i in range(n - 1) if (den if kind == "den" else num)[i] == 0]
    assert zeros == [j] and all((num if kind == "den" else den)[:n - 1])
    want, _, _ = model(inst)
    assert all(want[:j + 1]) and not any(want[j + 1:])
    zl, zc = run_device(gm_ctx, cname, inst)
    assert zl[:j + 1] == want[:j + 1]
    assert zl[j + 1:] == [0] * (n - 1 - j)
    assert zc == canon_int(c, want)


@pytest.mark.parametrize("cname", CURVES)
def test_perm_two_zero_denominators(gm_ctx, cname):
    """Zero denominators in both chunks: the first one decides, and the values
    before it are the model's (a backwards walk from a zero would lose them)."""
    import gnark_mi355x as gm
    c = pyref.CURVES[cname]
    r = c.r
    n = 2 * gm.PLONK_PERM_CHUNK
    j, j2 = 3 * gm.PLONK_PERM_E + 1, gm.PLONK_PERM_CHUNK + 9
    inst = Inst(c, n, 0x6310)
    inst.gamma = -(inst.p["l"][j] + inst.beta * inst.p["s1"][j]) % r
    inst.p["r"][j2] = -(inst.beta * inst.p["s2"][j2] + inst.gamma) % r
    _, den = factors(inst)
    assert [i for i in range(n - 1) if den[i] == 0] == [j, j2]
    want, _, _ = model(inst)
    zl, _ = run_device(gm_ctx, cname, inst, canonical=False)
    assert zl == want and all(zl[:j + 1]) and not any(zl[j + 1:])


# ---------------------------------------------------------------------------
# 4. a satisfying instance, through the quotient and the commit
# ---------------------------------------------------------------------------
QPOLYS = ("ql", "qr", "qm", "qo", "qk", "s1", "s2", "s3", "l", "r", "o", "z")


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


class _Sat:
    """Multiplication gates l r = o with shared wires (a permutation that is not
    the identity), Z by the running product, non-zero blinding: the Lagrange
    values for gm_plonk_perm_z and the canonical polynomials for the quotient."""

    def __init__(self, c, n):
        r = c.r
        rng = random.Random(0x6400)
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
        self.bl, self.br, self.bo, self.bz = rnd(2), rnd(2), rnd(2), rnd(3)
        self.alpha, self.beta, self.gamma = rnd(3)
        be, ga = self.beta, self.gamma
        z = [1] * n
        self.num, self.den = [], []
        for i in range(n):
            num = den = 1
            for col, wv in enumerate((lv, rv, ov)):
                num = num * (wv[i] + be * ids[col * n + i] + ga) % r
                den = den * (wv[i] + be * s[col * n + i] + ga) % r
            self.num.append(num)
            self.den.append(den)
            if i + 1 < n:
                z[i + 1] = z[i] * num * pow(den, -1, r) % r
        self.z = z
        self.lagrange = {"l": lv, "r": rv, "o": ov, "s1": s[:n], "s2": s[n:2 * n], "s3": s[2 * n:]}
        canon = lambda ev: canon_int(c, ev)
        self.p = {"ql": [0] * n, "qr": [0] * n, "qm": canon([1] * n), "qo": canon([r - 1] * n), "qk": [0] * n,
                  "s1": canon(s[:n]), "s2": canon(s[n:2 * n]), "s3": canon(s[2 * n:]),
                  "l": canon(lv), "r": canon(rv), "o": canon(ov), "z": canon(z)}


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


def _numerator_poly(inst):
    """T of gm_plonk_quotient as a coefficient list, by integer polynomial arithmetic."""
    c, r, n = inst.c, inst.c.r, inst.n
    g = c.coset_gen
    w0 = pyref.domain_generator(c, n)
    bl = _blinded(inst)
    P = {k: bl.get(k, inst.p[k]) for k in QPOLYS}
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


def test_perm_of_a_satisfying_instance_feeds_the_quotient_and_the_commit(gm_ctx, oracle):
    import gnark_mi355x as gm
    cname, n = "bls12377", 64
    c = pyref.CURVES[cname]
    r = c.r
    sat = _Sat(c, n)
    lag = {k: gm_ctx.copy_to_device(enc(c, sat.lagrange[k])) for k in POLYS}
    zl, zc, h = gm_ctx.malloc(32 * n), gm_ctx.malloc(32 * n), gm_ctx.malloc(32 * 4 * n)
    qbufs, srs = {}, None
    try:
        gm_ctx.plonk_perm_z(cname, n, lag, enc(c, [sat.beta]), enc(c, [sat.gamma]), zl, zc)
        zlb = zl.to_host()
        z = dec(c, zlb)
        # the running product, and it closes
        assert z == sat.z
        assert z[n - 1] * sat.num[n - 1] % r == sat.den[n - 1]
        assert dec(c, zc.to_host()) == sat.p["z"]
        # z_canonical, where it lies, is the quotient's z
        qbufs = {k: gm_ctx.copy_to_device(enc(c, sat.p[k])) for k in QPOLYS if k != "z"}
        blinds = {"bl": enc(c, sat.bl), "br": enc(c, sat.br), "bo": enc(c, sat.bo), "bz": enc(c, sat.bz)}
        gm_ctx.plonk_quotient(cname, n, dict(qbufs, z=zc), [], [], blinds, enc(c, [sat.alpha]), enc(c, [sat.beta]),
                              enc(c, [sat.gamma]), h)
        got = dec(c, h.to_host())
        assert not any(got[3 * n + 6:])
        assert any(got[2 * n + 4:3 * n + 6])
        t = _numerator_poly(sat)
        hz = _poly_add(r, [0] * n + got[:3 * n + 6], got[:3 * n + 6], -1)
        m = max(len(t), len(hz))
        assert hz + [0] * (m - len(hz)) == t + [0] * (m - len(t))
        # z_lagrange, where it lies, goes into the commit over the Lagrange SRS:
        # L_i(tau) = (tau^n - 1) w^i / (n (tau - w^i))
        tau = pyref.random_scalars(c, 1, 0x6402)[0]
        w = pyref.domain_generator(c, n)
        zh = (pow(tau, n, r) - 1) % r
        lis = [zh * pow(w, i, r) % r * pow(n * (tau - pow(w, i, r)) % r, -1, r) % r for i in range(n)]
        assert sum(lis) % r == 1
        points = oracle.batch_mul_base(cname, False, gm.generator(cname), enc(c, lis))
        srs = gm_ctx.points_upload(cname, points)
        _, aff = gm_ctx.msm_prepared(cname, zl, srs, n)
        assert aff == oracle.msm(cname, False, zlb, points)
    finally:
        for b in list(lag.values()) + list(qbufs.values()) + [zl, zc, h] + ([srs] if srs is not None else []):
            b.free()


# ---------------------------------------------------------------------------
# 5. inputs unchanged, repeatability, NULL canonical output, gm_trim
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("cname", CURVES)
def test_perm_leaves_inputs_and_repeats(gm_ctx, cname):
    import gnark_mi355x as gm
    n = 2 * gm.PLONK_PERM_CHUNK
    inst, (want, _, _) = random_case(cname, n)
    c = inst.c
    bufs = upload(gm_ctx, inst)
    zl, zc = gm_ctx.malloc(32 * n), gm_ctx.malloc(32 * n)
    try:
        call_device(gm_ctx, cname, inst, bufs, zl, zc)
        first_l, first_c = zl.to_host(), zc.to_host()
        assert dec(c, first_l) == want
        for k in POLYS:
            assert bufs[k].to_host() == enc(c, inst.p[k]), k
        zl.write(bytes(32 * n))
        zc.write(bytes(32 * n))
        call_device(gm_ctx, cname, inst, bufs, zl, zc)
        assert zl.to_host() == first_l and zc.to_host() == first_c
        # without the canonical output: z_lagrange the same, zc untouched
        zl.write(bytes(32 * n))
        zc.write(b"\x5a" * (32 * n))
        call_device(gm_ctx, cname, inst, bufs, zl, None)
        assert zl.to_host() == first_l and zc.to_host() == b"\x5a" * (32 * n)
        gm_ctx.trim()
        zl.write(bytes(32 * n))
        call_device(gm_ctx, cname, inst, bufs, zl, zc)
        assert zl.to_host() == first_l and zc.to_host() == first_c
    finally:
        for b in list(bufs.values()) + [zl, zc]:
            b.free()


# ---------------------------------------------------------------------------
# 6. refusals: every one on the host, before a launch
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("cname", CURVES)
def test_perm_refusals(gm_ctx, cname):
    import gnark_mi355x as gm
    c = pyref.CURVES[cname]
    n = 16
    inst = Inst(c, n, 0x6600)
    # 32 bytes of slack, so that a pointer moved by 8 bytes still has n elements behind it
    bufs = {k: gm_ctx.copy_to_device(enc(c, inst.p[k]) + bytes(32)) for k in POLYS}
    zl, zc = gm_ctx.malloc(32 * n + 32), gm_ctx.malloc(32 * n + 32)
    marks = b"\xa5" * (32 * n + 32), b"\x3c" * (32 * n + 32)
    zl.write(marks[0])
    zc.write(marks[1])
    off = lambda b, d: gm.DeviceBuffer(gm_ctx, b.ptr + d, 32 * n)
    cases = {
        "null member": (dict(bufs, s2=None), zl, zc, n),
        "null z_lagrange": (bufs, None, zc, n),
        "n = 4": (bufs, zl, zc, 4),
        "n = 24": (bufs, zl, zc, 24),
        "input off by 8": (dict(bufs, o=off(bufs["o"], 8)), zl, zc, n),
        "z_lagrange off by 8": (bufs, off(zl, 8), zc, n),
        "z_canonical off by 8": (bufs, zl, off(zc, 8), n),
        "z_lagrange aliasing l": (bufs, off(bufs["l"], 0), zc, n),
        "z_canonical aliasing s3": (bufs, zl, off(bufs["s3"], 0), n),
        "z_canonical inside r": (bufs, zl, off(bufs["r"], 32), n),
        "outputs aliasing each other": (bufs, zl, off(zl, 0), n),
        "outputs overlapping": (bufs, off(zl, 32), off(zl, 0), n),
    }
    try:
        for name, (b, l_out, c_out, nn) in cases.items():
            with pytest.raises(gm.GmError):
                call_device(gm_ctx, cname, inst, b, l_out, c_out, n=nn)
            assert zl.to_host() == marks[0] and zc.to_host() == marks[1], name
            for k in POLYS:
                assert bufs[k].to_host(32 * n) == enc(c, inst.p[k]), (name, k)
        # a NULL beta or gamma, through the struct itself
        a = gm._PlonkPermIn()
        a.n = n
        for k in POLYS:
            setattr(a, k, bufs[k].ptr)
        import ctypes
        keep = gm._buf(enc(c, [inst.beta]))
        a.beta, a.gamma = keep.ctypes.data, None
        assert gm.load_library().gm_plonk_perm_z(gm_ctx.handle, gm.curve_id(cname), ctypes.byref(a), zl.ptr,
                                                 zc.ptr) == -1
        assert zl.to_host() == marks[0] and zc.to_host() == marks[1]
        # and the call as it should be made
        call_device(gm_ctx, cname, inst, bufs, zl, zc)
        want, _, _ = model(inst)
        assert dec(c, zl.to_host(32 * n)) == want
        assert dec(c, zc.to_host(32 * n)) == canon_int(c, want)
    finally:
        for b in list(bufs.values()) + [zl, zc]:
            b.free()
