"""Inputs and the Python-integer oracle of the point-check tests
(test_points_check_gpu.py, test_points_check_abi.py).

The oracle classes a point from its stored bytes with integers only: a limb
string >= p is NOT_REDUCED, all zero is the infinity (OK), then the curve
equation, then pyref.Group.mul(P, r) being infinity.  Cases are built as raw
limb integers (the Montgomery residues as stored), so that non-reduced inputs can
be expressed; `case` names what a point is meant to be and the oracle decides
what it is."""
import functools
import os
import random
import sys

import pyref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if os.path.join(ROOT, "tools") not in sys.path:
    sys.path.insert(0, os.path.join(ROOT, "tools"))
import subgroup_constants as sub  # noqa: E402

OK, NOT_REDUCED, OFF_CURVE, OFF_SUBGROUP = 0, 1, 2, 3
CURVE_NAMES = ("bn254", "bls12377", "bls12381")
GROUPS = [(c, g2) for c in CURVE_NAMES for g2 in (False, True)]


def params(cname):
    return sub.curve_params(cname)


@functools.lru_cache(maxsize=None)
def derived(cname):
    """The tool's derivation of one curve (its assertions run once)."""
    return sub.derive(cname)


# ---- pyref's exceptional cases, confirmed where the oracle relies on them -----------
def group_law_handles_exceptions(c, g2, T2=None):
    """P + (-P) = infinity, and doubling a point with y = 0 gives infinity."""
    G = pyref.Group(c, g2)
    P = G.generator()
    ok = G.add(P, G.neg(P)) is None and G.add(None, P) == P and G.mul(P, 0) is None
    if T2 is not None:
        ok = ok and G.add(T2, T2) is None and G.mul(T2, 2) is None and G.mul(T2, 3) == T2
    return ok


# ---- raw encodings -----------------------------------------------------------------
def mont(c, x):
    return x % c.p * (1 << (64 * c.fp_limbs)) % c.p


def raw_of_point(c, P, g2):
    """The stored limb integers of an affine point (None = infinity): 2 or 4 of them."""
    if P is None:
        return (0,) * (4 if g2 else 2)
    if g2:
        return (mont(c, P[0][0]), mont(c, P[0][1]), mont(c, P[1][0]), mont(c, P[1][1]))
    return (mont(c, P[0]), mont(c, P[1]))


def raw_bytes(c, raw):
    return b"".join(v.to_bytes(8 * c.fp_limbs, "little") for v in raw)


@functools.lru_cache(maxsize=None)
def _classify(cname, g2, raw):
    c = params(cname)
    if any(v >= c.p for v in raw):
        return NOT_REDUCED, False
    if not any(raw):
        return OK, True
    rinv = pow(1 << (64 * c.fp_limbs), -1, c.p)
    v = [x * rinv % c.p for x in raw]
    P = ((v[0], v[1]), (v[2], v[3])) if g2 else (v[0], v[1])
    G = pyref.Group(c, g2)
    if not G.on_curve(P):
        return OFF_CURVE, False
    return (OK if G.mul(P, c.r) is None else OFF_SUBGROUP), False


def classify(cname, g2, raw):
    """(class, is_infinity) of stored limb integers, by the definition."""
    return _classify(cname, bool(g2), tuple(raw))


def decode(c, g2, raw):
    rinv = pow(1 << (64 * c.fp_limbs), -1, c.p)
    v = [x * rinv % c.p for x in raw]
    return ((v[0], v[1]), (v[2], v[3])) if g2 else (v[0], v[1])


def endomorphism_test(cname, g2, P):
    """The device's subgroup test in Python integers, for P on the curve and not
    infinity: the equation of DESIGN.md section 3.9 with the tool's constants."""
    c = params(cname)
    d = derived(cname)
    G = pyref.Group(c, g2)
    u = abs(d["u"])
    if not g2:
        if d["bn"]:
            return True
        T = G.add(G.mul(G.mul(P, u), u), G.neg(P))
        return T == (d["beta"] * P[0] % c.p, P[1])
    img = sub.psi(c, d["psi_x"], d["psi_y"], P)
    if d["bn"]:
        return G.mul(G.mul(G.mul(P, u), u), 6) == img
    return G.mul(P, u) == (G.neg(img) if d["u"] < 0 else img)


# ---- case lists ----------------------------------------------------------------------
def small_prime_factors(h, bound=1 << 16):
    out, q = [], 2
    while q < bound and h > 1:
        if h % q == 0:
            out.append(q)
            while h % q == 0:
                h //= q
        q += 1
    return out


def point_of_order(c, g2, q, h, seed):
    """A point of order q: [h r / q^k]P' (q^k the power of q in h) for random
    curve points P' until it is not infinity, then multiplied by q while the
    result stays finite.  Equals [h r / q]P' where the q-part of the group is
    cyclic, and still finds order q where it is not."""
    G = pyref.Group(c, g2)
    qk = 1
    while h % (qk * q) == 0:
        qk *= q
    for P in sub.random_curve_points(c, g2, 40, seed):
        T = G.mul(P, h * c.r // qk)
        while T is not None:
            nxt = G.mul(T, q)
            if nxt is None:
                return T
            T = nxt
    raise AssertionError("no point of order %d found" % q)


@functools.lru_cache(maxsize=None)
def cases(cname, g2):
    """[(name, raw limbs, intended class)] for one curve and group."""
    c = params(cname)
    d = derived(cname)
    p, r = c.p, c.r
    h = d["h2"] if g2 else d["h1"]
    G = pyref.Group(c, g2)
    F = G.F
    rng = random.Random(0x9C0 + 2 * CURVE_NAMES.index(cname) + int(g2))
    gen = G.generator()
    enc = lambda P: raw_of_point(c, P, g2)
    out = []

    # valid
    mult = [G.mul(gen, rng.randrange(1, r)) for _ in range(3)]
    out.append(("generator", enc(gen), OK))
    out += [("multiple%d" % i, enc(P), OK) for i, P in enumerate(mult)]
    out.append(("[r-1]G", enc(G.mul(gen, r - 1)), OK))
    out += [("P", enc(mult[0]), OK), ("-P", enc(G.neg(mult[0])), OK), ("infinity", enc(None), OK)]

    # not reduced: the stored words, no arithmetic
    words = 1 << (64 * c.fp_limbs)
    good = enc(mult[1])
    assert good[0] + p < words
    ones = words - 1
    out.append(("x+p", (good[0] + p,) + good[1:], NOT_REDUCED))
    out.append(("x=p", (p,) + good[1:], NOT_REDUCED))
    out.append(("all-ones x", (ones,) + good[1:], NOT_REDUCED))
    out.append(("all-ones y", good[:-1] + (ones,), NOT_REDUCED))
    out.append(("all-ones", (ones,) * len(good), NOT_REDUCED))
    out.append(("(0,p)", (0,) * (len(good) - (2 if g2 else 1)) + ((p, 0) if g2 else (p,)), NOT_REDUCED))
    if g2:
        out.append(("x.a1+p", (good[0], good[1] + p) + good[2:], NOT_REDUCED))
        out.append(("y.a1=p", good[:3] + (p,), NOT_REDUCED))
        out.append(("(0,(0,p))", (0, 0, 0, p), NOT_REDUCED))

    # off the curve
    x, y = mult[2]
    zero, one = G.zero, G.one
    out.append(("(x,y+1)", enc((x, F.add(y, one))), OFF_CURVE))
    out.append(("swapped", enc((y, x)), OFF_CURVE))
    out.append(("(x,0)", enc((x, zero)), OFF_CURVE))
    out.append(("(0,y)", enc((zero, y)), OFF_CURVE))

    # on the curve, off the subgroup
    if h > 1:
        rnd = sub.random_curve_points(c, g2, 3, 0x9D0 + len(cname) + int(g2))
        out += [("random curve point %d" % i, enc(P), OFF_SUBGROUP) for i, P in enumerate(rnd)]
        cof = G.mul(rnd[0], r)
        out.append(("[r]P'", enc(cof), OFF_SUBGROUP))
        if not g2 and cname == "bls12377":
            out.append(("(0,1) order 3", enc((0, 1)), OFF_SUBGROUP))
        if not g2 and cname == "bls12381":
            out.append(("(0,2) order 3", enc((0, 2)), OFF_SUBGROUP))
        small = []
        for q in small_prime_factors(h):
            T = point_of_order(c, g2, q, h, 0x9E0 + q)
            small.append(T)
            if q == 2:
                assert F.is_zero(T[1]) and group_law_handles_exceptions(c, g2, T)
            out.append(("order %d" % q, enc(T), OFF_SUBGROUP))
        # BLS12-377's G2 cofactor has no prime factor below 2^16: T is the cofactor point there
        for i, T in enumerate(small or [cof]):
            out.append(("P+T%d" % i, enc(G.add(mult[i % 3], T)), OFF_SUBGROUP))
    assert group_law_handles_exceptions(c, g2)
    return out
