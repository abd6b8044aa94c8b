#!/usr/bin/env python3
"""Generate the Montgomery constants for the six prime fields on the hot path.

Fields (gnark-crypto memory layout: little-endian 64-bit limbs, Montgomery form
x*R mod p with R = 2^(64*limbs)):

  bn254.fp      254-bit, 4 x u64   
  bn254.fr      254-bit, 4 x u64
  bls12377.fp   377-bit, 6 x u64
  bls12377.fr   253-bit, 4 x u64
  bls12381.fp   381-bit, 6 x u64
  bls12381.fr   255-bit, 4 x u64

Writes two independent headers so that the product (device + host code) and
the test oracle never share a source file:

  gnark-icicle_amd/csrc/field_constants.hpp   (product)
  oracle/oracle_constants.h                   (test oracle)

Run:  python tools/gen_field_constants.py
"""
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

FIELDS = {
    "BN254_FP": (21888242871839275222246405745257275088696311157297823662689037894645226208583, 4),
    "BN254_FR": (21888242871839275222246405745257275088548364400416034343698204186575808495617, 4),
    "BLS12377_FP": (258664426012969094010652733694893533536393512754914660539884262666720468348340822774968888139573360124440321458177, 6),
    "BLS12377_FR": (8444461749428370424248824938781546531375899335154063827935233455917409239041, 4),
    "BLS12381_FP": (0x1a0111ea397fe69a4b1ba7b6434bacd764774b84f38512bf6730d2a0f6b0f6241eabfffeb153ffffb9feffffffffaaab, 6),
    "BLS12381_FR": (0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001, 4),
}
# the fields and generators the test oracle's header carries
ORACLE_FIELDS = ("BN254_FP", "BN254_FR", "BLS12377_FP", "BLS12377_FR", "BLS12381_FP", "BLS12381_FR")
ORACLE_GENERATORS = ("BN254_G1", "BN254_G2", "BLS12377_G1", "BLS12377_G2", "BLS12381_G1", "BLS12381_G2")


# curve generators, canonical coordinates (gnark-crypto curve.Generators())
GENERATORS = {
    "BN254_G1": (("BN254_FP", 4), [1, 2]),
    "BN254_G2": (("BN254_FP", 4), [
        10857046999023057135944570762232829481370756359578518086990519993285655852781,
        11559732032986387107991004021392285783925812861821192530917403151452391805634,
        8495653923123431417604973247489272438418190587263600148770280649306958101930,
        4082367875863433681332203403145435568316851327593401208105741076214120093531]),
    "BLS12377_G1": (("BLS12377_FP", 6), [
        0x008848defe740a67c8fc6225bf87ff5485951e2caa9d41bb188282c8bd37cb5cd5481512ffcd394eeab9b16eb21be9ef,
        0x01914a69c5102eff1f674f5d30afeec4bd7fb348ca3e52d96d182ad44fb82305c2fe3d3634a9591afd82de55559c8ea6]),
    "BLS12377_G2": (("BLS12377_FP", 6), [
        233578398248691099356572568220835526895379068987715365179118596935057653620464273615301663571204657964920925606294,
        140913150380207355837477652521042157274541796891053068589147167627541651775299824604154852141315666357241556069118,
        63160294768292073209381361943935198908131692476676907196754037919244929611450776219210369229519898517858833747423,
        149157405641012693445398062341192467754805999074082136895788947234480009303640899064710353187729182149407503257491]),
    "BLS12381_G1": (("BLS12381_FP", 6), [
        0x17f1d3a73197d7942695638c4fa9ac0fc3688c4f9774b905a14e3a3f171bac586c55e83ff97a1aeffb3af00adb22c6bb,
        0x08b3f481e3aaa0f1a09e30ed741d8ae4fcf5e095d5d00af600db18cb2c04b3edd03cc744a2888ae40caa232946c5e7e1]),
    "BLS12381_G2": (("BLS12381_FP", 6), [
        0x024aa2b2f08f0a91260805272dc51051c6e47ad4fa403b02b4510b647ae3d1770bac0326a805bbefd48056c8c121bdb8,
        0x13e02b6052719f607dacd3a088274f65596bd0d09920b61ab5da61bbdc7f5049334cf11213945d57e5ac7d055d042b7e,
        0x0ce5d527727d6e118cc9cdc6da2e351aadfd9baa8cbdd3a76d429a695160d12c923ac9cc3baca289e193548608b82801,
        0x0606c4a02ea734cc32acd2b02bc28b99cb3e287e85a763af267492ab572e99ab3f370d275cec1da1aaa9075ff05f79be]),
}


def gen_mont_words(name):
    (field, n64), coords = GENERATORS[name]
    p = FIELDS[field][0]
    R = 1 << (64 * n64)
    out = []
    for x in coords:
        out += limbs(x * R % p, n64, 64)
    return out


def limbs(x, n, bits):
    m = (1 << bits) - 1
    return [(x >> (bits * i)) & m for i in range(n)]


def consts(p, n64):
    R = 1 << (64 * n64)
    return {
        "p": p,
        "one": R % p,
        "r2": (R * R) % p,
        "inv32": (-pow(p, -1, 1 << 32)) % (1 << 32),
        "inv64": (-pow(p, -1, 1 << 64)) % (1 << 64),
        "bits": p.bit_length(),
    }


def fmt_arr(vals, bits):
    w = 8 if bits == 32 else 16
    return ", ".join("0x%0*xu" % (w, v) + ("ll" if bits == 64 else "") for v in vals)


# radix-2^29 internal representation (device): limb counts chosen so that
# R' = 2^(29*N) > 4p and a FIPS column of 2N products of 58-bit terms fits in
# 64 bits (2N * 2^58 < 2^64  <=>  N <= 31).
RADIX = 29
N29 = {"BN254_FP": 9, "BN254_FR": 9, "BLS12377_FP": 14, "BLS12377_FR": 9,
       "BLS12381_FP": 14, "BLS12381_FR": 9}


def headroom(name):
    """floor(R' / p): a lazily reduced product a b with a b < k p^2 stays below
    R' p, and a representative below k p fits the limbs, exactly when
    k <= headroom.  The kernels assert their stated bounds against it."""
    p = FIELDS[name][0]
    return (1 << (RADIX * N29[name])) // p


def consts29(p, n64, n29):
    Rg = 1 << (64 * n64)
    Rp = 1 << (RADIX * n29)
    assert Rp > 4 * p and 2 * n29 * (1 << 58) < (1 << 64)
    return {
        "p": p, "inv": (-pow(p, -1, 1 << RADIX)) % (1 << RADIX),
        "one": Rp % p,                       # internal 1
        "r2": Rp * Rp % p,                   # canonical -> internal
        "kin": Rp * Rp * pow(Rg, -1, p) % p,  # gnark Montgomery -> internal
        "kout": Rg % p,                      # internal -> gnark Montgomery
        "kcan": Rp * pow(Rg, -1, p) % p,     # gnark Montgomery -> canonical
        "kgn": Rg * Rp % p,                  # canonical -> gnark Montgomery
    }


def product_header():
    out = ["// Generated by tools/gen_field_constants.py -- do not edit.",
           "// Montgomery constants, gnark-crypto layout (R = 2^(64*limbs)).",
           "#pragma once", "#include <cstdint>", "", "namespace gm {", ""]
    for name, (p, n64) in FIELDS.items():
        c = consts(p, n64)
        n32 = 2 * n64
        out.append("// %s: %d-bit modulus, %d x u32 limbs" % (name, c["bits"], n32))
        out.append("#define GM_%s_P32 {%s}" % (name, fmt_arr(limbs(p, n32, 32), 32)))
        out.append("#define GM_%s_ONE32 {%s}" % (name, fmt_arr(limbs(c["one"], n32, 32), 32)))
        out.append("#define GM_%s_R2_32 {%s}" % (name, fmt_arr(limbs(c["r2"], n32, 32), 32)))
        out.append("#define GM_%s_INV32 0x%08xu" % (name, c["inv32"]))
        out.append("#define GM_%s_P64 {%s}" % (name, fmt_arr(limbs(p, n64, 64), 64)))
        out.append("#define GM_%s_ONE64 {%s}" % (name, fmt_arr(limbs(c["one"], n64, 64), 64)))
        out.append("#define GM_%s_R2_64 {%s}" % (name, fmt_arr(limbs(c["r2"], n64, 64), 64)))
        out.append("#define GM_%s_INV64 0x%016xull" % (name, c["inv64"]))
        out.append("#define GM_%s_BITS %d" % (name, c["bits"]))
        n29 = N29[name]
        c29 = consts29(p, n64, n29)
        out.append("#define GM_%s_N29 %d" % (name, n29))
        out.append("#define GM_%s_NG %d" % (name, n32))
        out.append("#define GM_%s_INV29 0x%08xu" % (name, c29["inv"]))
        out.append("#define GM_%s_HEADROOM %dull" % (name, headroom(name)))
        for key in ("p", "one", "r2", "kin", "kout", "kcan", "kgn"):
            out.append("#define GM_%s_%s29 {%s}" % (name, key.upper(), fmt_arr(limbs(c29[key], n29, RADIX), 32)))
        out.append("")
    for g in GENERATORS:
        out.append("// %s generator, gnark layout (Montgomery, u64 limbs, X then Y)" % g)
        out.append("#define GM_%s_GEN64 {%s}" % (g, fmt_arr(gen_mont_words(g), 64)))
    out.append("")
    out.append("}  // namespace gm")
    return "\n".join(out) + "\n"


def oracle_header():
    out = ["/* Generated by tools/gen_field_constants.py -- do not edit.",
           " * TEST ORACLE ONLY: constants for the CPU restatement in oracle/. */",
           "#ifndef ORACLE_CONSTANTS_H", "#define ORACLE_CONSTANTS_H", "#include <stdint.h>", ""]
    for name in ORACLE_FIELDS:
        p, n64 = FIELDS[name]
        c = consts(p, n64)
        out.append("#define O_%s_P {%s}" % (name, fmt_arr(limbs(p, n64, 64), 64)))
        out.append("#define O_%s_ONE {%s}" % (name, fmt_arr(limbs(c["one"], n64, 64), 64)))
        out.append("#define O_%s_R2 {%s}" % (name, fmt_arr(limbs(c["r2"], n64, 64), 64)))
        out.append("#define O_%s_INV 0x%016xull" % (name, c["inv64"]))
        out.append("")
    for g in ORACLE_GENERATORS:
        out.append("#define O_%s_GEN {%s}" % (g, fmt_arr(gen_mont_words(g), 64)))
    out.append("")
    out.append("#endif")
    return "\n".join(out) + "\n"


if __name__ == "__main__":
    with open(os.path.join(ROOT, "gnark-icicle_amd", "csrc", "field_constants.hpp"), "w") as f:
        f.write(product_header())
    with open(os.path.join(ROOT, "oracle", "oracle_constants.h"), "w") as f:
        f.write(oracle_header())
    print("ok")
