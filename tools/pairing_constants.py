#!/usr/bin/env python3
"""Derives the constants of the device pairing (csrc/pairing_impl.hpp) and writes
them as csrc/pairing_constants.hpp.  Every identity the kernels rely on is
asserted on Python integers before anything is printed.

Tower: Fp6 = Fp2[v]/(v^3 - xi), Fp12 = Fp6[w]/(w^2 - v), so w^6 = xi;
xi = 9 + u (BN254), u (BLS12-377), 1 + u (BLS12-381).

  Frobenius     (sum c_i w^i)^(p^k) = sum conj^k(c_i) xi^(i (p^k - 1) / 6) w^i
  loop counter  6u + 2 (BN254, then the lines through pi(Q) and -pi^2(Q)); |u| on
                the BLS12 curves (BLS12-381: u < 0, the Miller value is conjugated)
  hard part     BLS12:  3 (p^4 - p^2 + 1) / r = (u - 1)^2 (u + p) (u^2 + p^2 - 1) + 3
                BN254:  2u (6u^2 + 3u + 1) (p^4 - p^2 + 1) / r
                          = l0 + l1 p + l2 p^2 + l3 p^3

Run:  python tools/pairing_constants.py          (rewrites the header)
      python tools/pairing_constants.py --print  (header on stdout)
      python tools/pairing_constants.py --check  (also runs the kernels' formulas,
            restated below on integers, against tests/pairing_model.py)
"""
import math
import os
import random
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import pyref  # noqa: E402

HEADER = os.path.join(ROOT, "gnark-icicle_amd", "csrc", "pairing_constants.hpp")
RADIX = 29
NAMES = ("bn254", "bls12377", "bls12381")
SEEDS = {"bn254": 4965661367192848881, "bls12377": 0x8508c00000000001, "bls12381": -0xd201000000010000}
TAGS = {"bn254": "BN254", "bls12377": "BLS12377", "bls12381": "BLS12381"}
XI = {"bn254": (9, 1), "bls12377": (0, 1), "bls12381": (1, 1)}


def f2_pow(F, a, e):
    r = (1, 0)
    while e:
        if e & 1:
            r = F.mul(r, a)
        a = F.mul(a, a)
        e >>= 1
    return r


def derive(name):
    c = pyref.CURVES[name]
    p, r, u = c.p, c.r, SEEDS[name]
    F2 = pyref.F2(c)
    bn = name == "bn254"
    xi = XI[name]
    d = dict(name=name, c=c, u=u, bn=bn, xi=xi)
    # xi is no square and no cube in Fp2, so w^6 - xi is irreducible over Fp2
    assert f2_pow(F2, xi, (p * p - 1) // 2) != (1, 0) and f2_pow(F2, xi, (p * p - 1) // 3) != (1, 0)
    # twist type from b'
    b = (c.b % p, 0)
    if F2.mul(b, F2.inv(xi)) == (c.b2[0] % p, c.b2[1] % p):
        d["m_twist"] = False
    else:
        assert F2.mul(b, xi) == (c.b2[0] % p, c.b2[1] % p)
        d["m_twist"] = True
    assert d["m_twist"] == (name == "bls12381")
    # Frobenius constants
    assert (p - 1) % 6 == 0
    d["frob"] = {}
    for k in (1, 2, 3):
        g = f2_pow(F2, xi, (p ** k - 1) // 6)
        row, acc = [], (1, 0)
        for _ in range(5):
            acc = F2.mul(acc, g)
            row.append(acc)
        d["frob"][k] = row
    assert all(x[1] == 0 for x in d["frob"][2])        # xi^((p^2 - 1) i / 6) lies in Fp
    # group orders and the loop counter
    phi12 = p ** 4 - p ** 2 + 1
    assert phi12 % r == 0
    if bn:
        assert p == 36 * u ** 4 + 36 * u ** 3 + 24 * u ** 2 + 6 * u + 1
        assert r == 36 * u ** 4 + 36 * u ** 3 + 18 * u ** 2 + 6 * u + 1
        d["loop"] = 6 * u + 2
        assert d["loop"] == 29793968203157093288
        s = 2 * u * (6 * u * u + 3 * u + 1)
        l0 = 12 * u ** 3 + 12 * u ** 2 + 6 * u + 1
        l1 = 12 * u ** 3 + 6 * u ** 2 + 4 * u
        l2 = 12 * u ** 3 + 6 * u ** 2 + 6 * u
        l3 = 12 * u ** 3 + 6 * u ** 2 + 4 * u - 1
        assert s * (phi12 // r) == l0 + l1 * p + l2 * p ** 2 + l3 * p ** 3
        # the chain of pairing_impl.hpp: a = f^l1, then l0 = l1 + 6u^2 + 2u + 1, l2 = l1 + 2u, l3 = l1 - 1
        assert l0 == l1 + 6 * u * u + 2 * u + 1 and l2 == l1 + 2 * u and l3 == l1 - 1
    else:
        assert r == u ** 4 - u ** 2 + 1 and p == (u - 1) ** 2 * r // 3 + u
        d["loop"] = abs(u)
        s = 3
        assert s * (phi12 // r) == (u - 1) ** 2 * (u + p) * (u * u + p * p - 1) + 3
    assert math.gcd(s, r) == 1
    d["s"] = s
    assert (p ** 12 - 1) == (p ** 6 - 1) * (p ** 2 + 1) * phi12      # easy part times the cyclotomic part
    assert abs(u) < 1 << 64 and d["loop"].bit_length() <= 65
    return d


# ---- the kernels' formulas on integers (the --check run) ------------------------
class Dev:
    """pairing_impl.hpp restated: the tower as nested tuples ((b0, b1, b2), (b0, b1, b2))."""

    def __init__(self, d):
        self.d = d
        self.c = d["c"]
        self.F = pyref.F2(self.c)
        self.p = self.c.p
        self.xi = d["xi"]
        self.u = d["u"]

    # Fp2
    def mxi(self, a):
        return self.F.mul(a, self.xi)

    def conj2(self, a):
        return (a[0] % self.p, (-a[1]) % self.p)

    # Fp6
    def add6(self, a, b):
        return tuple(self.F.add(x, y) for x, y in zip(a, b))

    def sub6(self, a, b):
        return tuple(self.F.sub(x, y) for x, y in zip(a, b))

    def neg6(self, a):
        return tuple(self.F.neg(x) for x in a)

    def mul6(self, a, b):
        F = self.F
        t0, t1, t2 = F.mul(a[0], b[0]), F.mul(a[1], b[1]), F.mul(a[2], b[2])
        c0 = F.add(t0, self.mxi(F.sub(F.sub(F.mul(F.add(a[1], a[2]), F.add(b[1], b[2])), t1), t2)))
        c1 = F.add(F.sub(F.sub(F.mul(F.add(a[0], a[1]), F.add(b[0], b[1])), t0), t1), self.mxi(t2))
        c2 = F.add(F.sub(F.sub(F.mul(F.add(a[0], a[2]), F.add(b[0], b[2])), t0), t2), t1)
        return (c0, c1, c2)

    def mulv6(self, a):
        return (self.mxi(a[2]), a[0], a[1])

    def mul6_01(self, a, b0, b1):
        F = self.F
        return (F.add(F.mul(a[0], b0), self.mxi(F.mul(a[2], b1))),
                F.add(F.mul(a[0], b1), F.mul(a[1], b0)),
                F.add(F.mul(a[1], b1), F.mul(a[2], b0)))

    def mul6_1(self, a, b1):
        F = self.F
        return (self.mxi(F.mul(a[2], b1)), F.mul(a[0], b1), F.mul(a[1], b1))

    def inv6(self, a):
        F = self.F
        A = F.sub(F.mul(a[0], a[0]), self.mxi(F.mul(a[1], a[2])))
        B = F.sub(self.mxi(F.mul(a[2], a[2])), F.mul(a[0], a[1]))
        C = F.sub(F.mul(a[1], a[1]), F.mul(a[0], a[2]))
        Fd = F.add(F.mul(a[0], A), self.mxi(F.add(F.mul(a[2], B), F.mul(a[1], C))))
        if F.is_zero(Fd):
            return ((0, 0),) * 3
        fi = F.inv(Fd)
        return (F.mul(A, fi), F.mul(B, fi), F.mul(C, fi))

    # Fp12
    def one(self):
        z = (0, 0)
        return (((1, 0), z, z), (z, z, z))

    def mul(self, a, b):
        t0, t1 = self.mul6(a[0], b[0]), self.mul6(a[1], b[1])
        c1 = self.sub6(self.sub6(self.mul6(self.add6(a[0], a[1]), self.add6(b[0], b[1])), t0), t1)
        return (self.add6(t0, self.mulv6(t1)), c1)

    def sqr(self, a):
        t = self.mul6(a[0], a[1])
        c0 = self.mul6(self.add6(a[0], a[1]), self.add6(a[0], self.mulv6(a[1])))
        c0 = self.sub6(self.sub6(c0, t), self.mulv6(t))
        return (c0, self.add6(t, t))

    def conj(self, a):
        return (a[0], self.neg6(a[1]))

    def inv(self, a):
        t = self.sub6(self.mul6(a[0], a[0]), self.mulv6(self.mul6(a[1], a[1])))
        ti = self.inv6(t)
        return (self.mul6(a[0], ti), self.neg6(self.mul6(a[1], ti)))

    def frob(self, a, k):
        F, g = self.F, self.d["frob"][k]
        cj = (lambda x: self.conj2(x)) if k % 2 else (lambda x: x)
        (c0, c2, c4), (c1, c3, c5) = a
        return ((cj(c0), F.mul(cj(c2), g[1]), F.mul(cj(c4), g[3])),
                (F.mul(cj(c1), g[0]), F.mul(cj(c3), g[2]), F.mul(cj(c5), g[4])))

    def cyc_sqr(self, a):
        F = self.F
        (x0, x1, x2), (x3, x4, x5) = a        # C0.B0, C0.B1, C0.B2, C1.B0, C1.B1, C1.B2

        def sq(x):
            return F.mul(x, x)
        t0, t1 = sq(x4), sq(x0)
        t6 = F.sub(F.sub(sq(F.add(x4, x0)), t0), t1)
        t2, t3 = sq(x2), sq(x3)
        t7 = F.sub(F.sub(sq(F.add(x2, x3)), t2), t3)
        t4, t5 = sq(x5), sq(x1)
        t8 = self.mxi(F.sub(F.sub(sq(F.add(x5, x1)), t4), t5))
        t0 = F.add(self.mxi(t0), t1)
        t2 = F.add(self.mxi(t2), t3)
        t4 = F.add(self.mxi(t4), t5)

        def m3s2(t, x):    # 3t - 2x
            d_ = F.sub(t, x)
            return F.add(F.add(d_, d_), t)

        def m3a2(t, x):    # 3t + 2x
            s_ = F.add(t, x)
            return F.add(F.add(s_, s_), t)
        return ((m3s2(t0, x0), m3s2(t2, x1), m3s2(t4, x2)), (m3a2(t8, x3), m3a2(t6, x4), m3a2(t7, x5)))

    def exp_abs_u(self, a):
        r = a
        for bit in bin(abs(self.u))[3:]:
            r = self.cyc_sqr(r)
            if bit == "1":
                r = self.mul(r, a)
        return r

    def exp_u(self, a):
        r = self.exp_abs_u(a)
        return self.conj(r) if self.u < 0 else r

    # lines: (ly, lx, lc) = the coefficients of yP, of -lambda xP and the constant
    def line_mul(self, f, ly, lx, lc):
        f0, f1 = f
        if not self.d["m_twist"]:
            # ly + lx w + lc w^3: A = (ly, 0, 0), B = (lx, lc, 0)
            t0 = tuple(self.F.mul(x, ly) for x in f0)
            t1 = self.mul6_01(f1, lx, lc)
            c1 = self.sub6(self.sub6(self.mul6_01(self.add6(f0, f1), self.F.add(ly, lx), lc), t0), t1)
        else:
            # lc + lx w^2 + ly w^3: A = (lc, lx, 0), B = (0, ly, 0)
            t0 = self.mul6_01(f0, lc, lx)
            t1 = self.mul6_1(f1, ly)
            c1 = self.sub6(self.sub6(self.mul6_01(self.add6(f0, f1), lc, self.F.add(lx, ly)), t0), t1)
        return (self.add6(t0, self.mulv6(t1)), c1)

    def scale(self, a, k):
        return (a[0] * k % self.p, a[1] * k % self.p)

    def dbl_step(self, T, P):
        F = self.F
        X, Y, Z = T
        xx = F.mul(X, X)
        W = F.add(F.add(xx, xx), xx)
        S = F.mul(Y, Z)
        yy = F.mul(Y, Y)
        # line, scaled by 2 Y Z^2: ly = 2 Y Z^2, lx = -3 X^2 Z, lc = 3 X^3 - 2 Y^2 Z
        sz = F.mul(S, Z)
        ly = self.scale(F.add(sz, sz), P[1])
        lx = self.scale(F.neg(F.mul(W, Z)), P[0])
        yyz = F.mul(yy, Z)
        lc = F.sub(F.mul(W, X), F.add(yyz, yyz))
        # the point
        R = F.mul(Y, S)
        B = F.mul(X, R)
        B4 = F.add(F.add(B, B), F.add(B, B))
        H = F.sub(F.mul(W, W), F.add(B4, B4))
        HS = F.mul(H, S)
        X3 = F.add(HS, HS)
        RR = F.mul(R, R)
        RR8 = F.add(RR, RR)
        RR8 = F.add(RR8, RR8)
        RR8 = F.add(RR8, RR8)
        Y3 = F.sub(F.mul(W, F.sub(B4, H)), RR8)
        S3 = F.mul(F.mul(S, S), S)
        Z3 = F.add(S3, S3)
        Z3 = F.add(Z3, Z3)
        Z3 = F.add(Z3, Z3)
        return (X3, Y3, Z3), (ly, lx, lc)

    def add_step(self, T, Q, P):
        F = self.F
        X, Y, Z = T
        x2, y2 = Q
        th = F.sub(F.mul(y2, Z), Y)
        mu = F.sub(F.mul(x2, Z), X)
        # line through Q with slope th / mu, scaled by mu
        ly = self.scale(mu, P[1])
        lx = self.scale(F.neg(th), P[0])
        lc = F.sub(F.mul(th, x2), F.mul(mu, y2))
        vv = F.mul(mu, mu)
        vvv = F.mul(vv, mu)
        R = F.mul(vv, X)
        A = F.sub(F.sub(F.mul(F.mul(th, th), Z), vvv), F.add(R, R))
        X3 = F.mul(mu, A)
        Y3 = F.sub(F.mul(th, F.sub(R, A)), F.mul(vvv, Y))
        Z3 = F.mul(vvv, Z)
        return (X3, Y3, Z3), (ly, lx, lc)

    def psi(self, Q, gx, gy):
        return (self.F.mul(gx, self.conj2(Q[0])), self.F.mul(gy, self.conj2(Q[1])))

    def miller(self, P, Q, psi_consts=None):
        if P is None or Q is None:
            return self.one()
        f, T = self.one(), (Q[0], Q[1], (1, 0))
        for bit in bin(self.d["loop"])[3:]:
            f = self.sqr(f)
            T, l = self.dbl_step(T, P)
            f = self.line_mul(f, *l)
            if bit == "1":
                T, l = self.add_step(T, Q, P)
                f = self.line_mul(f, *l)
        if self.d["bn"]:
            gx, gy = psi_consts
            Q1 = self.psi(Q, gx, gy)
            Q2 = self.psi(Q1, gx, gy)
            Q2 = (Q2[0], self.F.neg(Q2[1]))
            T, l = self.add_step(T, Q1, P)
            f = self.line_mul(f, *l)
            T, l = self.add_step(T, Q2, P)
            f = self.line_mul(f, *l)
        elif self.u < 0:
            f = self.conj(f)
        return f

    def final_exp(self, f):
        f = self.mul(self.conj(f), self.inv(f))           # p^6 - 1
        f = self.mul(self.frob(f, 2), f)                   # p^2 + 1
        if self.d["bn"]:
            fu = self.exp_u(f)
            fu2 = self.exp_u(fu)
            fu3 = self.exp_u(fu2)
            t2 = self.cyc_sqr(fu)
            t4 = self.cyc_sqr(t2)
            s2 = self.cyc_sqr(fu2)
            s6 = self.mul(self.cyc_sqr(s2), s2)
            v4 = self.cyc_sqr(self.cyc_sqr(fu3))
            v12 = self.mul(self.cyc_sqr(v4), v4)
            a = self.mul(self.mul(v12, s6), t4)
            y0 = self.mul(self.mul(self.mul(a, s6), t2), f)
            y2 = self.mul(a, t2)
            y3 = self.mul(a, self.conj(f))
            return self.mul(self.mul(y0, self.frob(a, 1)), self.mul(self.frob(y2, 2), self.frob(y3, 3)))
        a = self.mul(self.exp_u(f), self.conj(f))          # f^(u - 1)
        a = self.mul(self.exp_u(a), self.conj(a))          # ^(u - 1)
        b = self.mul(self.exp_u(a), self.frob(a, 1))       # ^(u + p)
        c = self.mul(self.mul(self.exp_u(self.exp_u(b)), self.frob(b, 2)), self.conj(b))   # ^(u^2 + p^2 - 1)
        return self.mul(c, self.mul(self.cyc_sqr(f), f))   # + 3


def check(name):
    import pairing_model
    import subgroup_constants
    d = derive(name)
    m = pairing_model.model(name)
    dev = Dev(d)
    rng = random.Random(0x9A1 + len(name))
    p = d["c"].p

    def to_dev(a):
        return ((a[0], a[2], a[4]), (a[1], a[3], a[5]))

    def to_model(t):
        (c0, c2, c4), (c1, c3, c5) = t
        return [c0, c1, c2, c3, c4, c5]

    def rnd():
        return [(rng.randrange(p), rng.randrange(p)) for _ in range(6)]
    a, b = rnd(), rnd()
    assert to_model(dev.mul(to_dev(a), to_dev(b))) == m.mul(a, b)
    assert to_model(dev.sqr(to_dev(a))) == m.sqr(a)
    assert to_model(dev.inv(to_dev(a))) == m.inv(a)
    assert to_model(dev.conj(to_dev(a))) == m.conj(a)
    for k in (1, 2, 3):
        assert to_model(dev.frob(to_dev(a), k)) == m.frob(a, k)
    assert m.frob(a, 1) == m.pow(a, p)
    e = m.mul(m.conj(a), m.inv(a))
    e = m.mul(m.frob(e, 2), e)                              # in the cyclotomic subgroup
    assert to_model(dev.cyc_sqr(to_dev(e))) == m.sqr(e)
    assert to_model(dev.exp_abs_u(to_dev(e))) == m.pow(e, abs(d["u"]))
    l = [(rng.randrange(p), rng.randrange(p)) for _ in range(3)]
    z = (0, 0)
    full = [l[2], z, l[1], l[0], z, z] if d["m_twist"] else [l[0], l[1], z, l[2], z, z]
    assert to_model(dev.line_mul(to_dev(a), *l)) == m.mul(a, full)
    psi_consts = None
    if d["bn"]:
        sd = subgroup_constants.derive(name)
        psi_consts = (sd["psi_x"], sd["psi_y"])
    x, y = rng.randrange(1, d["c"].r), rng.randrange(1, d["c"].r)
    P, Q = m.G1.mul(m.G1.generator(), x), m.G2.mul(m.G2.generator(), y)
    got = dev.final_exp(dev.miller(P, Q, psi_consts))
    want = m.pair(P, Q)
    assert to_model(got) == want, name
    assert not m.is_one(want) and m.is_one(m.pow(want, d["c"].r))
    print("checked", name)


# ---- header -------------------------------------------------------------------
def n29(c):
    return 9 if c.fp_limbs == 4 else 14


def fe29(c, v):
    n = n29(c)
    vi = v % c.p * (1 << (RADIX * n)) % c.p
    return "{" + ", ".join("0x%08xu" % ((vi >> (RADIX * i)) & ((1 << RADIX) - 1)) for i in range(n)) + "}"


def header():
    out = ["// Generated by tools/pairing_constants.py -- do not edit.",
           "// Constants of the device pairing (pairing_impl.hpp): the Miller loop counter and the",
           "// Frobenius constants xi^(i (p^k - 1) / 6), i = 1..5, k = 1..3, as radix-2^29 internal",
           "// Montgomery limbs (x * 2^(29 N) mod p).  The tool asserts the identities of DESIGN.md",
           "// section 3.11 before it prints.", "#pragma once", ""]
    for name in NAMES:
        d = derive(name)
        c, tag = d["c"], "GM_PAIR_" + TAGS[name]
        loop = d["loop"]
        out.append("// %s: xi = %d + %d u, %s-twist, loop counter 0x%x (%d bits), s = %s" % (
            TAGS[name], d["xi"][0], d["xi"][1], "M" if d["m_twist"] else "D", loop, loop.bit_length(),
            "2u(6u^2 + 3u + 1)" if d["bn"] else "3"))
        out.append("#define %s_M_TWIST %d" % (tag, 1 if d["m_twist"] else 0))
        out.append("#define %s_LOOP_BITS %d" % (tag, loop.bit_length()))
        out.append("// the bits of the loop counter below its top bit")
        out.append("#define %s_LOOP_LOW 0x%016xull" % (tag, loop - (1 << (loop.bit_length() - 1))))
        for k in (1, 2, 3):
            for i, g in enumerate(d["frob"][k]):
                out.append("#define %s_FROB%d_%d_A0 %s" % (tag, k, i + 1, fe29(c, g[0])))
                out.append("#define %s_FROB%d_%d_A1 %s" % (tag, k, i + 1, fe29(c, g[1])))
        out.append("")
    return "\n".join(out)


def main():
    if "--check" in sys.argv[1:]:
        for name in NAMES:
            check(name)
        return
    text = header()
    if "--print" in sys.argv[1:]:
        sys.stdout.write(text)
        return
    with open(HEADER, "w") as f:
        f.write(text)
    print("wrote", os.path.relpath(HEADER, ROOT))


if __name__ == "__main__":
    main()
