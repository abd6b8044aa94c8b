"""Big-integer model of the lazily reduced radix-2^29 layer (field.hpp, curve.hpp,
pair_fp2.hpp) for the raw-limb test hooks: raw encode / decode, R', edge values
and representatives v + j p, and the XYZZ accumulator cases of the curve tests.
Plain Python integers throughout; no GPU needed to import or to self-check."""
import itertools
import random
import struct

import pyref

RADIX = 29
MASK = (1 << RADIX) - 1


class Field:
    """One prime field in the internal form: N limbs, R' = 2^(29 N)."""

    def __init__(self, cname: str, kind: int):
        c = pyref.CURVES[cname]
        self.cname, self.kind, self.c = cname, kind, c
        self.p = c.r if kind == 0 else c.p
        self.N = -(-self.p.bit_length() // RADIX)
        if self.N * RADIX < self.p.bit_length() + 7:  # R' > 128 p (field.hpp "Lazily reduced arithmetic")
            self.N += 1
        self.R = 1 << (RADIX * self.N)
        self.Rinv = pow(self.R, -1, self.p)
        self.beta = -1 if cname == "bn254" else -5

    # ---- raw limbs ---------------------------------------------------------
    def enc(self, x: int) -> bytes:
        """x as N limbs; the top limb keeps any excess (must fit 32 bits)."""
        assert x >= 0
        limbs = [(x >> (RADIX * i)) & MASK for i in range(self.N - 1)] + [x >> (RADIX * (self.N - 1))]
        assert limbs[-1] < 1 << 32, "value does not fit the limbs"
        return struct.pack("<%dI" % self.N, *limbs)

    def enc_all(self, xs) -> bytes:
        return b"".join(self.enc(x) for x in xs)

    def limbs(self, b: bytes):
        n = len(b) // (4 * self.N)
        w = struct.unpack("<%dI" % (n * self.N), b)
        return [w[i * self.N:(i + 1) * self.N] for i in range(n)]

    @staticmethod
    def val(limbs) -> int:
        return sum(v << (RADIX * i) for i, v in enumerate(limbs))

    def dec_all(self, b: bytes):
        return [self.val(l) for l in self.limbs(b)]

    def normalised(self, limbs, top_excess=False) -> bool:
        return all(v <= MASK for v in (limbs[:-1] if top_excess else limbs))

    # ---- Montgomery form ---------------------------------------------------
    def to_mont(self, x: int) -> int:
        return x * self.R % self.p

    def from_mont(self, x: int) -> int:
        return x * self.Rinv % self.p

    def redc(self, t: int) -> int:
        """residue of a Montgomery reduction of the integer t"""
        return t * self.Rinv % self.p

    def redc_exact(self, t: int) -> int:
        """the integer an unsigned Montgomery reduction of t >= 0 returns without
        its final subtraction: (t + M p) / R' with M = -t / p mod R', the only
        M < R' that makes the sum divisible (whatever the order of the columns)"""
        M = (-t * pow(self.p, -1, self.R)) % self.R
        q, rem = divmod(t + M * self.p, self.R)
        assert rem == 0
        return q

    def cube_root(self, c: int):
        """a cube root of c mod p, or None (p = 1 mod 3 for all four fields)"""
        p = self.p
        if c % p == 0:
            return 0
        if pow(c, (p - 1) // 3, p) != 1:
            return None
        e, m = 0, p - 1
        while m % 3 == 0:
            e, m = e + 1, m // 3
        r0 = pow(c, pow(3, -1, m), p)            # r0^3 = c * (an element of 3-power order)
        z = 2
        while pow(z, (p - 1) // 3, p) == 1:
            z += 1
        h = pow(z, m, p)                         # generates the 3-Sylow subgroup, order 3^e
        for i in range(3 ** e):
            r = r0 * pow(h, i, p) % p
            if pow(r, 3, p) == c % p:
                return r
        return None

    # ---- inputs ------------------------------------------------------------
    def edge_values(self):
        p = self.p
        m = (p.bit_length() - 1) // RADIX          # index of p's highest non-zero limb
        pm = p >> (RADIX * m)
        ones = ((pm - 1) << (RADIX * m)) | ((1 << (RADIX * m)) - 1)   # low limbs all 2^29 - 1
        zeros = pm << (RADIX * m)                                      # low limbs all 0
        assert ones < p and zeros < p
        return [0, 1, 2, p - 1, p - 2, (p - 1) // 2, ones, zeros]

    def values(self, seed: int, nrand: int = 24):
        rng = random.Random(seed)
        return self.edge_values() + [rng.randrange(self.p) for _ in range(nrand)]


def lifted(F: Field, jmaxes, seed: int, per_combo: int = None, cap: int = 1024):
    """Operand tuples for a function whose k-th operand is < jmaxes[k] * p: every
    combination of multiples j_k < jmaxes[k] (a seeded sample of `cap` of them
    plus the corners when there are more), each with `per_combo` value tuples
    drawn round-robin from the edge and random values, plus every operand at its
    maximum (v = p - 1, j = jmax - 1) and at zero together (per_combo None: as many
    as bring the call to a few hundred elements).  Returns a list of
    tuples of integers."""
    rng = random.Random(seed)
    vals = [F.values(seed + 17 * k) for k in range(len(jmaxes))]
    for k, v in enumerate(vals):          # decorrelate the operands' edge values
        r = (3 * k) % len(v)
        vals[k] = v[r:] + v[:r]
    combos = list(itertools.product(*[range(j) for j in jmaxes]))
    if len(combos) > cap:
        corners = list(itertools.product(*[sorted({0, j - 1}) for j in jmaxes]))
        combos = corners + rng.sample(combos, cap - len(corners))
    if per_combo is None:                 # a few hundred elements, every value met several times
        per_combo = max(1, 320 // len(combos))
    out, t = [], 0
    for js in combos:
        for _ in range(per_combo):
            out.append(tuple(vals[k][(t + 5 * k * (t // len(vals[k]))) % len(vals[k])] + j * F.p
                             for k, j in enumerate(js)))
            t += 1
    # every j of every operand against the others' extremes and the edge values
    for k, jm in enumerate(jmaxes):
        for j in range(jm):
            for v in F.edge_values():
                out.append(tuple((v + j * F.p) if q == k else (F.p - 1 + (jq - 1) * F.p)
                                 for q, jq in enumerate(jmaxes)))
    out.append(tuple(j * F.p - 1 for j in jmaxes))
    out.append(tuple(0 for _ in jmaxes))
    return out


def covers_every_j(rows, jmaxes, p) -> bool:
    return all({r[k] // p for r in rows} == set(range(jm)) for k, jm in enumerate(jmaxes))


# ---- Fp2 on integers (components are plain residues or lazy representatives) --
def f2_mul(F: Field, a, b):
    return ((a[0] * b[0] + F.beta * a[1] * b[1]), (a[0] * b[1] + a[1] * b[0]))


# ---- XYZZ accumulators -------------------------------------------------------
class GroupModel:
    """XYZZ accumulators of one group in the internal Montgomery form.  A
    coordinate is an integer (G1) or a pair (G2); `lift` adds j p per component."""

    def __init__(self, cname: str, g2: bool):
        self.F = Field(cname, 1)
        self.g2 = g2
        self.G = pyref.Group(self.F.c, g2)
        self.K = pyref.F2(self.F.c) if g2 else pyref.F1(self.F.c)
        self.ncomp = 2 if g2 else 1

    def _comps(self, x):
        return list(x) if self.g2 else [x]

    def acc_from(self, Q, s):
        """(x zz, y zzz, zz = s^2, zzz = s^3) for the affine point Q, canonical
        Montgomery components, as a flat list of 4 * ncomp integers."""
        K, F = self.K, self.F
        zz = K.mul(s, s)
        zzz = K.mul(zz, s)
        coords = [K.mul(Q[0], zz), K.mul(Q[1], zzz), zz, zzz]
        return [F.to_mont(v) for co in coords for v in self._comps(co)]

    def acc_inf(self):
        """an infinite accumulator: zz = zzz = 0, x = y = 1 as xyzz_inf sets it"""
        F = self.F
        one = [F.to_mont(1)] + [0] * (self.ncomp - 1)
        return one + one + [0] * (2 * self.ncomp)

    def enc(self, flat) -> bytes:
        return self.F.enc_all(flat)

    def dec(self, b: bytes):
        """list of flat accumulators (4 * ncomp integers each) and their limbs"""
        w = 4 * self.ncomp
        L = self.F.limbs(b)
        return [[Field.val(l) for l in L[i:i + w]] for i in range(0, len(L), w)], \
               [L[i:i + w] for i in range(0, len(L), w)]

    def coords(self, flat):
        """flat lazy accumulator -> four field elements (canonical, out of Montgomery form)"""
        F = self.F
        v = [F.from_mont(x) for x in flat]
        if self.g2:
            return [(v[2 * k], v[2 * k + 1]) for k in range(4)]
        return v

    def is_inf(self, flat) -> bool:
        """infinity as the device reads it: every limb of zz zero (fe_is_zero(zz))"""
        return all(x == 0 for x in flat[2 * self.ncomp:3 * self.ncomp])

    def affine(self, flat):
        """the affine point of a lazy accumulator (None for infinity) and whether zz^3 = zzz^2"""
        K = self.K
        x, y, zz, zzz = self.coords(flat)
        ok = K.mul(K.mul(zz, zz), zz) == K.mul(zzz, zzz)
        if K.is_zero(zz):
            return None, ok
        return (K.mul(x, K.inv(zz)), K.mul(y, K.inv(zzz))), ok

    def lift(self, flat, js):
        """adds js[k] * p to the k-th integer of the flat accumulator"""
        return [v + j * self.F.p for v, j in zip(flat, js)]

    def acc_with_y(self, Q, ym: int, start: int = 0):
        """G1: an accumulator of Q whose y coordinate (Montgomery form) is ym - k
        for the smallest k >= start that allows it (y s^3 = target needs a cube
        root of target / y); returns (flat, k)."""
        assert not self.g2
        F = self.F
        for k in range(start, start + 64):
            c = F.from_mont(ym - k) * pow(Q[1], -1, F.p) % F.p
            s = F.cube_root(c)
            if s:
                flat = self.acc_from(Q, s)
                assert flat[1] == ym - k
                return flat, k
        raise AssertionError("no cube root in 64 tries")

    def random_s(self, rng):
        p = self.F.p
        return (rng.randrange(1, p), rng.randrange(p)) if self.g2 else rng.randrange(1, p)

    def one(self):
        return (1, 0) if self.g2 else 1
