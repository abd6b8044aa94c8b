"""Derives the GLV constants of csrc/msm_impl.hpp (GlvBn254, GlvBls377, GlvBls381)
and checks them against the oracle's group law (test infrastructure, not product
code).  BN254 G1:

phi(x, y) = (beta x, y) = [lambda] P; short basis of the lattice
{(a, b): a + b lambda = 0 mod r} from the extended Euclid on (r, lambda);
c1 = floor(k g1 / 2^384), c2 = floor(k g2 / 2^384) with g1 = floor(2^384 b2 / r),
g2 = floor(2^384 |b1| / r); k1 = k - c1 a1 - c2 a2 in [0, 2^127),
k2 = c1 |b1| - c2 b2 in (-2^127, 2^127).  Run: python tools/glv_constants.py
"""
import os
import random
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "oracle"))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))
import pyref  # noqa: E402
import bls12381_params  # noqa: E402

SH = 384


def cube_roots(m):
    for g in range(2, 100):
        w = pow(g, (m - 1) // 3, m)
        if w != 1:
            return [w, w * w % m]


def short_basis(r, lam):
    """Two short vectors (a, b) with a + b lam = 0 mod r (GLV, sec. 4)."""
    r0, r1, t0, t1 = r, lam, 0, 1
    hist = [(r0, t0), (r1, t1)]
    while r1 * r1 >= r:
        q = r0 // r1
        r0, r1 = r1, r0 - q * r1
        t0, t1 = t1, t0 - q * t1
        hist.append((r1, t1))
    rm, tm = hist[-2]
    rm1, tm1 = hist[-1]
    q = r0 // r1
    rn, tn = r0 - q * r1, t0 - q * t1
    v1 = (rm1, -tm1)
    v2 = (rm, -tm) if rm * rm + tm * tm <= rn * rn + tn * tn else (rn, -tn)
    return v1, v2


def derive():
    c = pyref.BN254
    p, r = c.p, c.r
    G = pyref.Group(c, False)
    P0 = G.generator()
    lam = beta = None
    for l_ in cube_roots(r):
        for b_ in cube_roots(p):
            if G.mul(P0, l_) == (b_ * P0[0] % p, P0[1]):
                lam, beta = l_, b_
    (a1, b1), (a2, b2) = short_basis(r, lam)
    assert a1 * b2 - a2 * b1 == r and a1 > 0 and a2 > 0 and b1 < 0 and b2 > 0
    assert a2 == -b1
    g1 = (b2 << SH) // r
    g2 = ((-b1) << SH) // r
    return dict(p=p, r=r, lam=lam, beta=beta, a1=a1, b1=b1, a2=a2, b2=b2, g1=g1, g2=g2)


def split(k, d):
    M = (1 << 128) - 1
    c1 = (k * d["g1"]) >> SH
    c2 = (k * d["g2"]) >> SH
    k1 = (k - c1 * d["a1"] - c2 * d["a2"]) & M
    k2 = (c1 * (-d["b1"]) - c2 * d["b2"]) & M
    k2 = k2 - (1 << 128) if k2 >> 127 else k2
    return k1, k2


def derive_bls12377():
    """BLS12-377: lambda = x^2 - 1 (x = 0x8508c00000000001 the curve seed) is a
    cube root of unity of r with lambda^2 < r < (lambda + 1)^2, so the split is a
    plain division: k2 = floor(k / lambda) < 2^127, k1 = k - k2 lambda < lambda
    (both unsigned).  Device: q = floor(k g / 2^384), g = floor(2^384 / lambda),
    undershoots k / lambda by < 1, then one conditional correction."""
    c = pyref.BLS12_377 if hasattr(pyref, "BLS12_377") else pyref.CURVES["bls12377"]
    p, r = c.p, c.r
    x = 0x8508c00000000001
    lam = x * x - 1
    assert (lam * lam + lam + 1) % r == 0 and lam < (1 << 127) and lam * lam < r < (lam + 1) ** 2
    G1, G2 = pyref.Group(c, False), pyref.Group(c, True)
    P, Q = G1.generator(), G2.generator()
    b1 = [b for b in cube_roots(p) if G1.mul(P, lam) == (b * P[0] % p, P[1])]
    LQ = G2.mul(Q, lam)
    b2 = [b for b in cube_roots(p) if LQ == ((Q[0][0] * b % p, Q[0][1] * b % p), Q[1])]
    assert len(b1) == 1 and len(b2) == 1 and b2[0] == b1[0] * b1[0] % p
    return dict(p=p, r=r, lam=lam, beta=b1[0], beta_g2=b2[0], g=(1 << SH) // lam)


def split_bls12377(k, d):
    M = (1 << 128) - 1
    q = (k * d["g"]) >> SH
    k1 = (k - q * d["lam"]) & M
    if k1 >= d["lam"]:
        k1 -= d["lam"]
        q += 1
    return k1, q


def main_bls12377():
    d = derive_bls12377()
    r, lam = d["r"], d["lam"]
    rng = random.Random(8)
    specials = [0, 1, 2, r - 1, r - 2, lam, lam - 1, lam + 1, lam * lam, lam * lam - 1, lam * lam + lam,
                r - lam, (r - 1) // 2, 1 << 252]
    for t in range(200000):
        k = specials[t] if t < len(specials) else rng.randrange(r)
        k1, k2 = split_bls12377(k, d)
        assert 0 <= k1 < lam and 0 <= k2 < (1 << 127) and k1 + k2 * lam == k
    c = pyref.CURVES["bls12377"]
    G1 = pyref.Group(c, False)
    for P in pyref.random_points(c, 3, 12):
        assert G1.mul(P, lam) == (d["beta"] * P[0] % d["p"], P[1])

    def l64(x, n):
        return ", ".join("0x%016xull" % ((x >> (64 * i)) & (2 ** 64 - 1)) for i in range(n))

    def r29(v):
        vi = v * (1 << (29 * 14)) % d["p"]
        return ", ".join("0x%08xu" % ((vi >> (29 * i)) & (2 ** 29 - 1)) for i in range(14))
    print("BLS12-377 g", l64(d["g"], 5))
    print("BLS12-377 lambda", l64(lam, 2))
    print("BLS12-377 beta29 (G1)", r29(d["beta"]))
    print("BLS12-377 beta29 (G2 twist, beta^2)", r29(d["beta_g2"]))
    print("BLS12-377 split checked on 200000 scalars; phi checked on G1 and G2 generators")


# ---------------------------------------------------------------------------
# BLS12-381: lambda = x^2 - 1 (x = -0xd201000000010000) ~ 2^127.43, so the halves
# of the unsigned division split (up to lambda) do not fit the digit geometry's
# GLV_HALF_BITS = 127.  Signed, balanced split instead:
#   k > r/2:  k <- r - k and both halves change sign (flip);
#   k2 = round(k / lambda), k1 = k - k2 lambda:  |k1| <= (lambda - 1) / 2,
#   0 <= k2 <= (lambda + 1) / 2 + 1, both below 2^126.44.
# Device arithmetic (split_bls12381 models it word for word): q = floor(k g /
# 2^384) with g = floor(2^384 / lambda) is floor(k / lambda), or one less when
# lambda divides k (k g / 2^384 undershoots k / lambda by less than 2^-130 and a
# non-zero fraction of k / lambda is at least 1 / lambda > 2^-128); so
# r0 = k - q lambda lies in [0, lambda] and is exact in 128-bit wrap-around
# arithmetic (lambda < 2^128).  r0 > (lambda - 1) / 2 rounds up: k1 = r0 - lambda.
# ---------------------------------------------------------------------------
GLV_HALF_BITS = 127  # csrc/msm.hpp: the bits a GLV half's digits cover


def derive_bls12381():
    c = bls12381_params.BLS12_381
    p, r = c.p, c.r
    lam = bls12381_params.LAMBDA
    assert (lam * lam + lam + 1) == r and pow(lam, 3, r) == 1 and (1 << 127) < lam < (1 << 128) and lam & 1
    G1, G2 = pyref.Group(c, False), pyref.Group(c, True)
    P, Q = G1.generator(), G2.generator()
    b1 = [b for b in cube_roots(p) if G1.mul(P, lam) == (b * P[0] % p, P[1])]
    LQ = G2.mul(Q, lam)
    b2 = [b for b in cube_roots(p) if LQ == ((Q[0][0] * b % p, Q[0][1] * b % p), Q[1])]
    assert len(b1) == 1 and len(b2) == 1 and b2[0] == b1[0] * b1[0] % p
    return dict(p=p, r=r, lam=lam, beta=b1[0], beta_g2=b2[0], g=(1 << SH) // lam, half=(r - 1) // 2)


def split_bls12381(k, d):
    """(|k1|, neg1, |k2|, neg2) with k = (-1)^neg1 |k1| + (-1)^neg2 |k2| lambda mod r."""
    M = (1 << 128) - 1
    lam = d["lam"]
    flip = 1 if k > d["half"] else 0
    kk = d["r"] - k if flip else k
    q = (kk * d["g"]) >> SH
    assert q <= M
    r0 = (kk - q * lam) & M
    assert r0 == kk - q * lam  # exact: the true value lies in [0, lambda]
    neg1 = 0
    if r0 > (lam >> 1):
        r0 = (lam - r0) & M
        q = (q + 1) & M
        neg1 = 1
    return r0, neg1 ^ flip, q, flip


def check_split_bls12381(k, d):
    k1, n1, k2, n2 = split_bls12381(k, d)
    assert 0 <= k1 < (1 << GLV_HALF_BITS) and 0 <= k2 < (1 << GLV_HALF_BITS)
    assert k1 <= (d["lam"] - 1) // 2 and k2 <= (d["lam"] + 1) // 2 + 1
    assert ((-k1 if n1 else k1) + (-k2 if n2 else k2) * d["lam"] - k) % d["r"] == 0
    return k1, n1, k2, n2


def specials_bls12381(d):
    """The special scalars of the split: the field's ends, the flip threshold,
    multiples of lambda, the rounding threshold of k1 on both sides and with both
    flips (each half at its largest magnitude, every sign combination)."""
    r, lam = d["r"], d["lam"]
    h = lam >> 1  # (lambda - 1) / 2: the largest |k1|
    m = (lam + 1) // 2  # about the largest k2 of an unflipped scalar
    ks = [0, 1, 2, r - 1, r - 2, (r - 1) // 2, (r + 1) // 2, lam, lam - 1, lam + 1, lam * lam, lam * lam - 1,
          lam * lam + lam, r - lam, 1 << 254,
          h, h + 1, lam + h, lam + h + 1,                  # k1 = +h, -h (k2 = 0/1, 1/2)
          (m - 1) * lam + h, (m - 1) * lam + h + 1,        # large k2 with k1 = +-h
          (r - 1) // 2 - h, (r + 1) // 2 + h]
    ks += [r - k for k in ks if 0 < k < r]                 # the flipped side
    return [k % r for k in ks]


def main_bls12381(count=200000):
    d = derive_bls12381()
    r, lam = d["r"], d["lam"]
    rng = random.Random(9)
    sp = specials_bls12381(d)
    seen = set()
    big1 = big2 = 0
    for t in range(count):
        k = sp[t] if t < len(sp) else rng.randrange(r)
        k1, n1, k2, n2 = check_split_bls12381(k, d)
        seen.add((n1, n2))
        big1, big2 = max(big1, k1), max(big2, k2)
    assert seen == {(0, 0), (0, 1), (1, 0), (1, 1)} and big1 == lam >> 1
    c = bls12381_params.BLS12_381
    G1 = pyref.Group(c, False)
    for P in pyref.random_points(c, 3, 12):
        assert G1.mul(P, lam) == (d["beta"] * P[0] % d["p"], P[1])

    def l64(x, n):
        return ", ".join("0x%016xull" % ((x >> (64 * i)) & (2 ** 64 - 1)) for i in range(n))

    def r29(v):
        vi = v * (1 << (29 * 14)) % d["p"]
        return ", ".join("0x%08xu" % ((vi >> (29 * i)) & (2 ** 29 - 1)) for i in range(14))
    print("BLS12-381 g", l64(d["g"], 5))
    print("BLS12-381 lambda", l64(lam, 2))
    print("BLS12-381 (r - 1) / 2", l64(d["half"], 4))
    print("BLS12-381 r", l64(r, 4))
    print("BLS12-381 beta29 (G1)", r29(d["beta"]))
    print("BLS12-381 beta29 (G2 twist)", r29(d["beta_g2"]))
    print("BLS12-381 largest |k1| 2^%.2f, k2 2^%.2f (GLV_HALF_BITS = %d)" %
          (__import__("math").log2(big1), __import__("math").log2(big2), GLV_HALF_BITS))
    print("BLS12-381 split checked on %d scalars; phi checked on G1 and G2 generators" % count)


def main():
    d = derive()
    r, lam = d["r"], d["lam"]
    specials = [0, 1, 2, r - 1, r - 2, lam, r - lam, lam + 1, lam - 1, d["a1"], d["b2"], r - d["b2"],
                (r - 1) // 2, (r + 1) // 2, 1 << 253]
    rng = random.Random(7)
    for t in range(200000):
        k = specials[t] if t < len(specials) else rng.randrange(r)
        k1, k2 = split(k, d)
        assert 0 <= k1 < (1 << 127) and abs(k2) < (1 << 127)
        assert (k1 + k2 * lam - k) % r == 0
    # group-law check of phi on random points
    G = pyref.Group(pyref.BN254, False)
    for P in pyref.random_points(pyref.BN254, 4, 11):
        assert G.mul(P, lam) == (d["beta"] * P[0] % d["p"], P[1])

    def l64(x, n):
        return ", ".join("0x%016xull" % ((x >> (64 * i)) & (2 ** 64 - 1)) for i in range(n))
    bi = d["beta"] * (1 << 261) % d["p"]
    print("g1", l64(d["g1"], 5))
    print("g2", l64(d["g2"], 4))
    print("a1", l64(d["a1"], 2), " a2=|b1|", l64(d["a2"], 1), " b2", l64(d["b2"], 2))
    print("beta29", ", ".join("0x%08xu" % ((bi >> (29 * i)) & (2 ** 29 - 1)) for i in range(9)))
    print("split checked on 200000 scalars; phi checked on 4 points")


if __name__ == "__main__":
    main()
    main_bls12377()
    main_bls12381()
