"""A plain-integer model of the optimal ate pairing on BN254, BLS12-377 and
BLS12-381, independent of the device's formulas (csrc/pairing_impl.hpp).

  * Fp12 = Fp2[w]/(w^6 - xi): an element is a list of six Fp2 pairs c0..c5,
    sum c_i w^i; products are schoolbook, the inverse is a 6 x 6 linear solve.
    The device's tower (Fp6 = Fp2[v]/(v^3 - xi), Fp12 = Fp6[w]/(w^2 - v)) holds
    the same element as C0 = (c0, c2, c4), C1 = (c1, c3, c5).
  * Q is untwisted into E(Fp12): (x w^2, y w^3) for the D-twists (BN254,
    BLS12-377), (x / w^2, y / w^3) for BLS12-381's M-twist; the Miller loop is
    the textbook affine one over E(Fp12) with the curve's loop counter, and the
    final exponentiation is one pow by s (p^12 - 1) / r with gnark-crypto's s
    (3 on the BLS12 curves, 2u(6u^2 + 3u + 1) on BN254).
Slow on purpose: a second or two per pairing."""
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "oracle"))
import pyref  # noqa: E402

SEEDS = {"bn254": 4965661367192848881, "bls12377": 0x8508c00000000001, "bls12381": -0xd201000000010000}
XI = {"bn254": (9, 1), "bls12377": (0, 1), "bls12381": (1, 1)}
M_TWIST = {"bn254": False, "bls12377": False, "bls12381": True}
CURVE_IDS = {"bn254": 0, "bls12377": 1, "bls12381": 2}

# tower slot (E12 memory order C0.B0, C0.B1, C0.B2, C1.B0, C1.B1, C1.B2) of w^i
TOWER_SLOT = (0, 3, 1, 4, 2, 5)


class Model:
    def __init__(self, name):
        self.name = name
        self.c = c = pyref.CURVES[name]
        self.p, self.r, self.u = c.p, c.r, SEEDS[name]
        self.F2 = pyref.F2(c)
        self.xi = XI[name]
        self.m_twist = M_TWIST[name]
        self.bn = name == "bn254"
        self.G1, self.G2 = pyref.Group(c, False), pyref.Group(c, True)
        u = self.u
        self.loop = 6 * u + 2 if self.bn else abs(u)
        self.s = 2 * u * (6 * u * u + 3 * u + 1) if self.bn else 3
        assert (self.p ** 12 - 1) % self.r == 0
        self.final_exponent = self.s * ((self.p ** 12 - 1) // self.r)
        # the twist: b' = b / xi (D) or b xi (M)
        b = (c.b % c.p, 0)
        want = self.F2.mul(b, self.xi) if self.m_twist else self.F2.mul(b, self.F2.inv(self.xi))
        assert want == (c.b2[0] % c.p, c.b2[1] % c.p), name
        # w^p = gamma w, so (sum c_i w^i)^p = sum conj(c_i) gamma^i w^i
        assert (self.p - 1) % 6 == 0
        g = self.f2_pow(self.xi, (self.p - 1) // 6)
        self.gamma = [(1, 0)]
        for _ in range(5):
            self.gamma.append(self.F2.mul(self.gamma[-1], g))

    # ---- Fp2 ----------------------------------------------------------------
    def f2_pow(self, a, e):
        r = (1, 0)
        while e:
            if e & 1:
                r = self.F2.mul(r, a)
            a = self.F2.mul(a, a)
            e >>= 1
        return r

    def f2_conj(self, a):
        return (a[0] % self.p, (-a[1]) % self.p)

    # ---- Fp12 ---------------------------------------------------------------
    def zero(self):
        return [(0, 0)] * 6

    def one(self):
        return [(1, 0)] + [(0, 0)] * 5

    def from_fp(self, x):
        return [(x % self.p, 0)] + [(0, 0)] * 5

    def add(self, a, b):
        return [self.F2.add(x, y) for x, y in zip(a, b)]

    def sub(self, a, b):
        return [self.F2.sub(x, y) for x, y in zip(a, b)]

    def neg(self, a):
        return [self.F2.neg(x) for x in a]

    def mul(self, a, b):
        p, beta = self.p, self.c.beta
        acc = [[0, 0] for _ in range(11)]
        for i, (x0, x1) in enumerate(a):
            if x0 == 0 and x1 == 0:
                continue
            for j, (y0, y1) in enumerate(b):
                t = acc[i + j]
                t[0] += x0 * y0 + beta * x1 * y1
                t[1] += x0 * y1 + x1 * y0
        out = []
        for k in range(6):
            lo = (acc[k][0] % p, acc[k][1] % p)
            if k < 5:
                hi = self.F2.mul((acc[k + 6][0] % p, acc[k + 6][1] % p), self.xi)
                lo = self.F2.add(lo, hi)
            out.append(lo)
        return out

    def sqr(self, a):
        return self.mul(a, a)

    def is_one(self, a):
        return [tuple(x) for x in a] == self.one()

    def eq(self, a, b):
        return all(self.F2.is_zero(self.F2.sub(x, y)) for x, y in zip(a, b))

    def w_pow(self, k):
        """w^k for any integer k (w^6 = xi)."""
        q, i = divmod(k, 6)
        s = self.f2_pow(self.xi, q) if q >= 0 else self.f2_pow(self.F2.inv(self.xi), -q)
        out = [(0, 0)] * 6
        out[i] = s
        return out

    def inv(self, a):
        """1 / a by solving (multiplication by a) x = 1 over Fp2; 0 -> 0."""
        F = self.F2
        if all(F.is_zero(x) for x in a):
            return self.zero()
        cols = [self.mul(a, self.w_pow(j)) for j in range(6)]
        m = [[cols[j][i] for j in range(6)] + [(1, 0) if i == 0 else (0, 0)] for i in range(6)]
        for col in range(6):
            piv = next(i for i in range(col, 6) if not F.is_zero(m[i][col]))
            m[col], m[piv] = m[piv], m[col]
            pi = F.inv(m[col][col])
            m[col] = [F.mul(x, pi) for x in m[col]]
            for i in range(6):
                if i != col and not F.is_zero(m[i][col]):
                    f = m[i][col]
                    m[i] = [F.sub(x, F.mul(f, y)) for x, y in zip(m[i], m[col])]
        out = [m[i][6] for i in range(6)]
        assert self.is_one(self.mul(a, out))
        return out

    def pow(self, a, e):
        if e < 0:
            return self.pow(self.inv(a), -e)
        r = self.one()
        for bit in bin(e)[2:] if e else "":
            r = self.sqr(r)
            if bit == "1":
                r = self.mul(r, a)
        return r

    def conj(self, a):
        """a^(p^6): w -> -w."""
        return [x if i % 2 == 0 else self.F2.neg(x) for i, x in enumerate(a)]

    def frob(self, a, k=1):
        for _ in range(k):
            a = [self.F2.mul(self.f2_conj(x), g) for x, g in zip(a, self.gamma)]
        return a

    # ---- the tower's memory order -------------------------------------------
    def to_tower(self, a):
        """The twelve Fp integers in gnark-crypto's E12 order."""
        out = [0] * 12
        for i, x in enumerate(a):
            out[2 * TOWER_SLOT[i]], out[2 * TOWER_SLOT[i] + 1] = x[0] % self.p, x[1] % self.p
        return out

    def from_tower(self, v):
        return [(v[2 * TOWER_SLOT[i]] % self.p, v[2 * TOWER_SLOT[i] + 1] % self.p) for i in range(6)]

    def encode(self, a) -> bytes:
        return b"".join(pyref.encode_fp(self.c, x) for x in self.to_tower(a))

    def decode(self, b: bytes):
        n = 8 * self.c.fp_limbs
        return self.from_tower([pyref.mont_decode(b[i * n:(i + 1) * n], self.p, self.c.fp_limbs) for i in range(12)])

    # ---- pairing --------------------------------------------------------------
    def untwist(self, Q):
        x, y = Q
        if self.m_twist:
            return self.mul([x] + [(0, 0)] * 5, self.w_pow(-2)), self.mul([y] + [(0, 0)] * 5, self.w_pow(-3))
        return self.mul([x] + [(0, 0)] * 5, self.w_pow(2)), self.mul([y] + [(0, 0)] * 5, self.w_pow(3))

    def _step(self, T, S, P):
        """The line through T and S (the tangent when T = S) at P, and T + S."""
        (xt, yt), (xs, ys) = T, S
        if self.eq(xt, xs) and self.eq(yt, ys):
            x2 = self.sqr(xt)
            lam = self.mul(self.add(self.add(x2, x2), x2), self.inv(self.add(yt, yt)))
        else:
            lam = self.mul(self.sub(ys, yt), self.inv(self.sub(xs, xt)))
        line = self.sub(self.sub(self.from_fp(P[1]), yt), self.mul(lam, self.sub(self.from_fp(P[0]), xt)))
        x3 = self.sub(self.sub(self.sqr(lam), xt), xs)
        y3 = self.sub(self.mul(lam, self.sub(xt, x3)), yt)
        return line, (x3, y3)

    def miller(self, P, Q):
        """f_{loop, Q}(P) (with BN254's two closing lines); 1 when P or Q is infinity."""
        if P is None or Q is None:
            return self.one()
        Q12 = self.untwist(Q)
        T, f = Q12, self.one()
        for bit in bin(self.loop)[3:]:
            line, T = self._step(T, T, P)
            f = self.mul(self.sqr(f), line)
            if bit == "1":
                line, T = self._step(T, Q12, P)
                f = self.mul(f, line)
        if self.bn:
            Q1 = (self.frob(Q12[0]), self.frob(Q12[1]))
            Q2 = (self.frob(Q12[0], 2), self.neg(self.frob(Q12[1], 2)))
            line, T = self._step(T, Q1, P)
            f = self.mul(f, line)
            line, T = self._step(T, Q2, P)
            f = self.mul(f, line)
        elif self.u < 0:
            f = self.inv(f)
        return f

    def final_exp(self, f):
        return self.pow(f, self.final_exponent)

    def pair(self, P, Q):
        return self.final_exp(self.miller(P, Q))

    def pairing_check(self, pairs):
        f = self.one()
        for P, Q in pairs:
            f = self.mul(f, self.miller(P, Q))
        return self.is_one(self.final_exp(f))

    def groth16_verify(self, vk, proof, publics):
        """vk: dict alpha_g1, beta_g2, gamma_g2, delta_g2, k (list of G1); proof: (Ar, Bs, Krs)."""
        G1, G2 = self.G1, self.G2
        assert len(publics) + 1 == len(vk["k"])
        ksum = vk["k"][0]
        for x, K in zip(publics, vk["k"][1:]):
            ksum = G1.add(ksum, G1.mul(K, x % self.r))
        Ar, Bs, Krs = proof
        return self.pairing_check([(Ar, Bs), (Krs, G2.neg(vk["delta_g2"])), (ksum, G2.neg(vk["gamma_g2"])),
                                   (G1.neg(vk["alpha_g1"]), vk["beta_g2"])])


# ---- the bellman known answers (tests/golden/bellman_bls12381_verify.json) ------------
def bellman_vectors():
    """The twelve vectors as raw records: dict(vk=dict of compressed records
    alpha_g1, beta_g1, beta_g2, gamma_g2, delta_g1, delta_g2 and the list k,
    proof=(A, B, C) compressed records, inputs=[integers], ok=flag)."""
    import base64
    import json
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "bellman_bls12381_verify.json")
    out = []
    for v in json.load(open(path))["vectors"]:
        vk, proof, inputs = (base64.b64decode(v[k]) for k in ("vk", "proof", "inputs"))
        names = (("alpha_g1", 48), ("beta_g1", 48), ("beta_g2", 96), ("gamma_g2", 96), ("delta_g1", 48), ("delta_g2", 96))
        rec, off = {}, 0
        for name, size in names:
            rec[name] = vk[off:off + size]
            off += size
        count = int.from_bytes(vk[off:off + 4], "big")
        off += 4
        rec["k"] = [vk[off + 48 * i:off + 48 * (i + 1)] for i in range(count)]
        off += 48 * count
        assert vk[off:] == bytes(196) and len(proof) == 192 and len(inputs) == 32 * (count - 1)
        out.append(dict(vk=rec, proof=(proof[:48], proof[48:144], proof[144:]),
                        inputs=[int.from_bytes(inputs[i:i + 32], "big") for i in range(0, len(inputs), 32)],
                        ok=bool(v["ok"])))
    return out


_MODELS = {}


def model(name) -> Model:
    if name not in _MODELS:
        _MODELS[name] = Model(name)
    return _MODELS[name]
