#!/usr/bin/env python3
"""Derives the constants of the device point check (csrc/points_check.hip) and
writes them as csrc/subgroup_constants.hpp.  Every constant is checked against
the oracle's group law (pyref) and every closing identity of DESIGN.md section
3.9 is asserted on integers before anything is printed.

Per curve (seed u):
  BN254       p = 36u^4 + 36u^3 + 24u^2 + 6u + 1, r = p + 1 - t, t = 6u^2 + 1
  BLS12-377 / BLS12-381
              r = u^4 - u^2 + 1, p = (u - 1)^2 r / 3 + u, t = u + 1

Tests (P on the curve already):
  BLS12 G1    phi(P) = [lambda]P, phi(x, y) = (beta x, y), lambda = u^2 - 1:
              phi^2 + phi + 1 = 0 on E and lambda^2 + lambda + 1 = r.
  BN254 G2    psi(Q) = [t - 1]Q = [6u^2]Q: psi^2 - t psi + p = 0 on E'(Fp2)
              gives [(t-1)^2 - t(t-1) + p]Q = [p + 1 - t]Q = [r]Q.
  BLS12 G2    psi(Q) = [u]Q (u = t - 1): the same substitution gives
              [h1 r]Q = 0 with h1 = (u - 1)^2 / 3; #E'(Fp2) = h2 r and
              gcd(h1, h2) = 1, so the order of Q divides r.
psi(x, y) = (gx conj(x), gy conj(y)) is the untwist-Frobenius-twist map.

Run:  python tools/subgroup_constants.py          (rewrites the header)
      python tools/subgroup_constants.py --print  (header on stdout)
"""
import math
import os
import random
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import pyref  # noqa: E402
import bls12381_params  # noqa: E402

HEADER = os.path.join(ROOT, "gnark-icicle_amd", "csrc", "subgroup_constants.hpp")
RADIX = 29
SEEDS = {"bn254": 4965661367192848881, "bls12377": 0x8508c00000000001, "bls12381": -0xd201000000010000}
TAGS = {"bn254": "BN254", "bls12377": "BLS12377", "bls12381": "BLS12381"}


def curve_params(name):
    return bls12381_params.BLS12_381 if name == "bls12381" else pyref.CURVES[name]


# ---- square roots (test inputs: random curve points) --------------------------
def sqrt_fp(a, p):
    """A square root of a mod p, or None (Tonelli-Shanks; p = 3 mod 4 shortcut)."""
    a %= p
    if a == 0:
        return 0
    if pow(a, (p - 1) // 2, p) != 1:
        return None
    if p % 4 == 3:
        return pow(a, (p + 1) // 4, p)
    q, s = p - 1, 0
    while q % 2 == 0:
        q //= 2
        s += 1
    z = 2
    while pow(z, (p - 1) // 2, p) != p - 1:
        z += 1
    m, c, t, x = s, pow(z, q, p), pow(a, q, p), pow(a, (q + 1) // 2, p)
    while t != 1:
        i, t2 = 0, t
        while t2 != 1:
            t2 = t2 * t2 % p
            i += 1
        b = pow(c, 1 << (m - i - 1), p)
        m, c = i, b * b % p
        t, x = t * c % p, x * b % p
    return x


def sqrt_fp2(a, c):
    """A square root of a = (a0, a1) in Fp[u]/(u^2 - beta), or None."""
    p, beta = c.p, c.beta
    F = pyref.F2(c)
    a0, a1 = a[0] % p, a[1] % p
    if a1 == 0:
        s = sqrt_fp(a0, p)
        if s is not None:
            return (s, 0)
        s = sqrt_fp(a0 * pow(beta, -1, p), p)
        return None if s is None else (0, s)
    n = sqrt_fp(a0 * a0 - beta * a1 * a1, p)  # the norm's root
    if n is None:
        return None
    half = pow(2, -1, p)
    for cand in ((a0 + n) * half % p, (a0 - n) * half % p):
        x0 = sqrt_fp(cand, p)
        if x0 is None or x0 == 0:
            continue
        x = (x0, a1 * pow(2 * x0, -1, p) % p)
        if F.mul(x, x) == (a0, a1):
            return x
    return None


def random_curve_points(c, g2, count, seed):
    """Points of E(Fp) / E'(Fp2) by x-coordinate sampling: almost never in the
    r-torsion when the cofactor is not 1."""
    G = pyref.Group(c, g2)
    F = G.F
    rng = random.Random(seed)
    out = []
    while len(out) < count:
        x = (rng.randrange(c.p), rng.randrange(c.p)) if g2 else rng.randrange(c.p)
        rhs = F.add(F.mul(F.mul(x, x), x), G.b)
        y = sqrt_fp2(rhs, c) if g2 else sqrt_fp(rhs, c.p)
        if y is None:
            continue
        if rng.randrange(2):
            y = F.neg(y)
        assert G.on_curve((x, y))
        out.append((x, y))
    return out


def f2_pow(F, a, e):
    r = (1, 0)
    while e:
        if e & 1:
            r = F.mul(r, a)
        a = F.mul(a, a)
        e >>= 1
    return r


def conj(c, a):
    return (a[0] % c.p, (-a[1]) % c.p)


def psi(c, gx, gy, Q):
    F = pyref.F2(c)
    return (F.mul(gx, conj(c, Q[0])), F.mul(gy, conj(c, Q[1])))


# ---- derivation ---------------------------------------------------------------
def derive(name):
    c = curve_params(name)
    p, r, u = c.p, c.r, SEEDS[name]
    bn = name == "bn254"
    d = dict(name=name, c=c, u=u, bn=bn)
    if bn:
        assert p == 36 * u ** 4 + 36 * u ** 3 + 24 * u ** 2 + 6 * u + 1
        t = 6 * u * u + 1
        assert r == p + 1 - t                      # cofactor 1: the curve equation is the G1 test
        h1, h2 = 1, p - 1 + t                      # #E'(Fp2) = (p - 1 + t) r
        d["g2_scalar"] = t - 1
        assert d["g2_scalar"] == 6 * u * u and d["g2_scalar"] > 0
    else:
        assert r == u ** 4 - u ** 2 + 1 and (u - 1) ** 2 % 3 == 0
        h1 = (u - 1) ** 2 // 3
        assert p == h1 * r + u
        t = u + 1
        lam = u * u - 1
        assert lam * lam + lam + 1 == r            # G1 closing identity
        num = u ** 8 - 4 * u ** 7 + 5 * u ** 6 - 4 * u ** 4 + 6 * u ** 3 - 4 * u ** 2 - 4 * u + 13
        assert num % 9 == 0
        h2 = num // 9
        assert math.gcd(h1, h2) == 1               # G2 closing condition
        d["lam"] = lam
        d["g2_scalar"] = u                         # = t - 1, negative for BLS12-381
    assert p + 1 - t == h1 * r                     # #E(Fp) = h1 r
    assert h1 % r and h2 % r                       # the r-torsion of E(Fp) and of E'(Fp2) is cyclic of order r
    # psi^2 - t psi + p = 0 with psi = [k]: (k^2 - t k + p) = h1 r when k = t - 1
    k = t - 1
    assert k * k - t * k + p == h1 * r
    assert (k - p) % r == 0                        # psi acts as p on G2: the test holds on the subgroup
    d.update(t=t, h1=h1, h2=h2)

    G1, G2 = pyref.Group(c, False), pyref.Group(c, True)
    F2 = pyref.F2(c)
    # #E'(Fp2) = h2 r on random twist points, #E(Fp) = h1 r on random curve points
    for Q in random_curve_points(c, True, 3, 0x5B0 + len(name)):
        assert G2.mul(Q, h2 * r) is None
    for P in random_curve_points(c, False, 3, 0x5B1 + len(name)):
        assert G1.mul(P, h1 * r) is None

    if not bn:
        betas = []
        for g in range(2, 100):
            w = pow(g, (p - 1) // 3, p)
            if w != 1:
                betas = [w, w * w % p]
                break
        P0 = G1.generator()
        LP = G1.mul(P0, d["lam"] % r)
        ok = [b for b in betas if LP == (b * P0[0] % p, P0[1])]
        assert len(ok) == 1
        d["beta"] = ok[0]
        assert (ok[0] * ok[0] + ok[0] + 1) % p == 0   # phi^2 + phi + 1 = 0 on all of E

    # the twist's xi from b' (D-twist: b' = b / xi; M-twist: b' = b xi), psi's two constants
    b_fp2 = (c.b % p, 0)
    xis = [F2.mul(b_fp2, F2.inv(c.b2)), F2.mul(c.b2, F2.inv(b_fp2))]
    Q0 = G2.generator()
    want = G2.mul(Q0, p % r)
    sample = random_curve_points(c, True, 3, 0x5B2 + len(name))
    found = []
    for xi in xis:
        gx0, gy0 = f2_pow(F2, xi, (p - 1) // 3), f2_pow(F2, xi, (p - 1) // 2)
        for gx in (gx0, F2.inv(gx0)):
            for gy in (gy0, F2.inv(gy0)):
                if not all(G2.on_curve(psi(c, gx, gy, Q)) for Q in sample + [Q0]):
                    continue
                if psi(c, gx, gy, Q0) == want and (gx, gy) not in found:
                    found.append((gx, gy))
    assert len(found) == 1, found
    d["psi_x"], d["psi_y"] = found[0]
    # psi satisfies its characteristic equation on all of E'(Fp2), off the subgroup too
    for Q in sample:
        p2 = psi(c, d["psi_x"], d["psi_y"], psi(c, d["psi_x"], d["psi_y"], Q))
        tp = G2.mul(psi(c, d["psi_x"], d["psi_y"], Q), t % (h2 * r))
        assert G2.add(p2, G2.mul(Q, p)) == tp
    return d


def hamming(k):
    return bin(abs(k)).count("1")


def op_counts(d, g2):
    """(doublings, additions) per point of the device test of this group."""
    u = abs(d["u"])
    ladder = (u.bit_length() - 1, hamming(u) - 1)
    if d["bn"]:
        # [6]([u]([u]Q)): two ladders, then 2T, 2T + T, 2(3T)
        return (2 * ladder[0] + 2, 2 * ladder[1] + 1) if g2 else (0, 0)
    if g2:
        return ladder
    return (2 * ladder[0], 2 * ladder[1] + 1)     # [u]([u]P) - P


# ---- header -------------------------------------------------------------------
def n29(c):
    return 9 if c.fp_limbs == 4 else 14


def fe29(c, v):
    n = n29(c)
    vi = v % c.p * (1 << (RADIX * n)) % c.p
    return "{" + ", ".join("0x%08xu" % ((vi >> (RADIX * i)) & ((1 << RADIX) - 1)) for i in range(n)) + "}"


def header():
    out = ["// Generated by tools/subgroup_constants.py -- do not edit.",
           "// Constants of the device point check (points_check.hip): curve coefficients and",
           "// endomorphism constants as radix-2^29 internal Montgomery limbs (x * 2^(29 N) mod p),",
           "// the seed u as magnitude and sign.  The tool asserts the closing identities",
           "// (DESIGN.md section 3.9) before it prints.", "#pragma once", ""]
    for name in ("bn254", "bls12377", "bls12381"):
        d = derive(name)
        c, tag = d["c"], "GM_SUB_" + TAGS[name]
        out.append("// %s: u = %s0x%x" % (TAGS[name], "-" if d["u"] < 0 else "", abs(d["u"])))
        out.append("#define %s_U_ABS 0x%016xull" % (tag, abs(d["u"])))
        out.append("#define %s_U_NEG %d" % (tag, 1 if d["u"] < 0 else 0))
        out.append("#define %s_B %s" % (tag, fe29(c, c.b)))
        out.append("#define %s_B2_A0 %s" % (tag, fe29(c, c.b2[0])))
        out.append("#define %s_B2_A1 %s" % (tag, fe29(c, c.b2[1])))
        if not d["bn"]:
            out.append("// phi(x, y) = (beta x, y) = [u^2 - 1](x, y) on G1")
            out.append("#define %s_BETA %s" % (tag, fe29(c, d["beta"])))
        out.append("// psi(x, y) = (PSI_X conj(x), PSI_Y conj(y)) = [%s](x, y) on G2" % ("6u^2" if d["bn"] else "u"))
        out.append("#define %s_PSI_X_A0 %s" % (tag, fe29(c, d["psi_x"][0])))
        out.append("#define %s_PSI_X_A1 %s" % (tag, fe29(c, d["psi_x"][1])))
        out.append("#define %s_PSI_Y_A0 %s" % (tag, fe29(c, d["psi_y"][0])))
        out.append("#define %s_PSI_Y_A1 %s" % (tag, fe29(c, d["psi_y"][1])))
        for g2 in (False, True):
            dbl, add = op_counts(d, g2)
            out.append("// %s test: %d doublings, %d additions per point" % ("G2" if g2 else "G1", dbl, add))
        out.append("")
    return "\n".join(out)


def main():
    text = header()
    if "--print" in sys.argv[1:]:
        sys.stdout.write(text)
        return
    with open(HEADER, "w") as f:
        f.write(text)
    print("wrote", os.path.relpath(HEADER, ROOT))


if __name__ == "__main__":
    main()
