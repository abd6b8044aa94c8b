"""BLS12-381 (curve id 2) for the tests: the curve's published constants, the
pyref.CurveParams the oracles hold for it (pyref.CURVES["bls12381"], checked
against those constants here) and the small encoders and circuit builders the
test_bls12381_* files share.  Their expectations come from pyref and from
points of known discrete log, independently of the C++ oracle."""
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "oracle"))
import pyref  # noqa: E402

P = 0x1a0111ea397fe69a4b1ba7b6434bacd764774b84f38512bf6730d2a0f6b0f6241eabfffeb153ffffb9feffffffffaaab
R = 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001
SEED = -0xd201000000010000            # the curve seed x
LAMBDA = SEED * SEED - 1              # cube root of unity of Fr: r = lambda^2 + lambda + 1
TWO_ADICITY = 32
COSET_GEN = 7                         # fr FrMultiplicativeGen
OMEGA_MAX = pow(COSET_GEN, (R - 1) >> TWO_ADICITY, R)

CURVE_ID = 2
FP_BYTES = 48
FR_BITS = 255

# the published generators (canonical coordinates); the oracles' own copies are
# held equal to these by tests/test_oracle.py
G1_GEN = (0x17f1d3a73197d7942695638c4fa9ac0fc3688c4f9774b905a14e3a3f171bac586c55e83ff97a1aeffb3af00adb22c6bb,
          0x08b3f481e3aaa0f1a09e30ed741d8ae4fcf5e095d5d00af600db18cb2c04b3edd03cc744a2888ae40caa232946c5e7e1)
G2_GEN = ((0x024aa2b2f08f0a91260805272dc51051c6e47ad4fa403b02b4510b647ae3d1770bac0326a805bbefd48056c8c121bdb8,
           0x13e02b6052719f607dacd3a088274f65596bd0d09920b61ab5da61bbdc7f5049334cf11213945d57e5ac7d055d042b7e),
          (0x0ce5d527727d6e118cc9cdc6da2e351aadfd9baa8cbdd3a76d429a695160d12c923ac9cc3baca289e193548608b82801,
           0x0606c4a02ea734cc32acd2b02bc28b99cb3e287e85a763af267492ab572e99ab3f370d275cec1da1aaa9075ff05f79be))

BLS12_381 = pyref.CURVES["bls12381"]
assert (BLS12_381.p, BLS12_381.r, BLS12_381.g1, BLS12_381.g2) == (P, R, G1_GEN, G2_GEN)
assert (BLS12_381.coset_gen, BLS12_381.omega_max, BLS12_381.two_adicity) == (COSET_GEN, OMEGA_MAX, TWO_ADICITY)

C = BLS12_381
NAME = "bls12381"


# ---- encoders / small builders shared by the BLS12-381 tests ------------------
def enc_fr(vals) -> bytes:
    return b"".join(pyref.encode_fr(C, v % R) for v in vals)


def dec_fr(b: bytes):
    return [pyref.decode_fr(C, b[i:i + 32]) for i in range(0, len(b), 32)]


def enc_points(points, g2: bool) -> bytes:
    return b"".join(pyref.encode_point(C, P_, g2) for P_ in points)


def multiples(g2: bool, count: int):
    """[1]G .. [count]G (affine) by repeated addition: points with known discrete
    logarithms, so an MSM's expected value is one scalar multiplication."""
    G = pyref.Group(C, g2)
    g = G.generator()
    out, acc = [], None
    for _ in range(count):
        acc = G.add(acc, g)
        out.append(acc)
    return out


def squaring_chain(k: int, x: int = 2):
    """The squaring-chain circuit of tests/r1cs.py for this curve: (constraints,
    nb_wires, nb_public, witness)."""
    cons = [([(2 + j, 1)], [(2 + j, 1)], [(3 + j, 1)]) for j in range(k)]
    cons.append(([(0, 1)], [(2 + k, 1)], [(1, 1)]))
    W = [1, 0, x % R]
    v = x % R
    for _ in range(k):
        v = v * v % R
        W.append(v)
    W[1] = v
    return cons, 3 + k, 2, W


def cubic_circuit():
    cons = [([(2, 1)], [(2, 1)], [(3, 1)]), ([(3, 1)], [(2, 1)], [(4, 1)]),
            ([(0, 1)], [(1, 1)], [(4, 1), (2, 1), (0, 5)])]
    return cons, 5, 2, [1, 35, 3, 9, 27]


def solve_abc(cons, W):
    return tuple([sum(W[w] * co for w, co in row[m]) % R for row in cons] for m in range(3))


def pk_bytes(pk: dict) -> dict:
    """pyref.g16_setup's key as the gnark-layout byte arrays gm.ProvingKey takes."""
    import numpy as np
    out = {k: enc_points([pk[k]], k.startswith("g2")) for k in ("g1_alpha", "g1_beta", "g1_delta", "g2_beta", "g2_delta")}
    for k in ("g1_A", "g1_B", "g1_Z", "g1_K", "g2_B"):
        out[k] = enc_points(pk[k], k.startswith("g2")) or bytes(4 * FP_BYTES)
    out["infA"] = np.array(pk["infA"], dtype=np.uint8)
    out["infB"] = np.array(pk["infB"], dtype=np.uint8)
    return out
