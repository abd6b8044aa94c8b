"""BLS12-381 (curve id 2) without a device: the constants' self-checks, the
constants generator against the committed headers, the host entries against
pyref with the BLS12-381 CurveParams, the refusals of the deferred entries and
the GLV split model of tools/glv_constants.py."""
import ctypes
import os
import random
import sys

import numpy as np
import pytest

import pyref
import bls12381_params as bp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

C = bp.C
ERR_INVALID, ERR_UNSUPPORTED = -1, -4


@pytest.fixture(scope="module")
def gm():
    import gnark_mi355x as gm
    gm.load_library()
    return gm


def _is_prime(n):  # Miller-Rabin by pow, fixed bases
    d, s = n - 1, 0
    while d % 2 == 0:
        d, s = d // 2, s + 1
    for a in (2, 3, 5, 7, 11, 13, 17, 19, 23, 29, 31, 37):
        x = pow(a, d, n)
        if x in (1, n - 1):
            continue
        for _ in range(s - 1):
            x = x * x % n
            if x == n - 1:
                break
        else:
            return False
    return True


def test_constants():
    assert _is_prime(bp.P) and _is_prime(bp.R)
    assert bp.P.bit_length() == 381 and bp.R.bit_length() == 255 == bp.FR_BITS
    G1, G2 = pyref.Group(C, False), pyref.Group(C, True)
    assert G1.on_curve(C.g1) and G2.on_curve(C.g2)
    assert G1.mul(C.g1, C.r) is None and G2.mul(C.g2, C.r) is None
    assert (bp.R - 1) % (1 << 32) == 0 and (bp.R - 1) % (1 << 33) != 0
    w = bp.OMEGA_MAX
    assert w == 10238227357739495823651030575849232062558860180284477541189508159991286009131
    assert pow(w, 1 << 32, bp.R) == 1 and pow(w, 1 << 31, bp.R) != 1
    # the same rule gives pyref's omega_max of the two existing curves
    for c in pyref.CURVES.values():
        assert pow(c.coset_gen, (c.r - 1) >> c.two_adicity, c.r) == c.omega_max
    assert pow(bp.LAMBDA, 3, bp.R) == 1 and bp.LAMBDA ** 2 + bp.LAMBDA + 1 == bp.R


def test_generated_headers_match_committed():
    import gen_field_constants as g
    with open(os.path.join(ROOT, "oracle", "oracle_constants.h")) as f:
        assert g.oracle_header() == f.read()
    with open(os.path.join(ROOT, "gnark-icicle_amd", "csrc", "field_constants.hpp")) as f:
        assert g.product_header() == f.read()
    assert g.headroom("BLS12381_FR") == 70 and g.headroom("BN254_FR") == 169 and g.headroom("BLS12377_FR") == 438
    assert g.headroom("BLS12381_FP") >> 25 == 1


def test_python_mirror(gm):
    assert gm.BLS12_381 == 2 and gm.CURVES["bls12381"] == 2 and gm.FP_BYTES[2] == 48
    assert gm.point_bytes(2, False) == 96 and gm.point_bytes(2, True) == 192


def _jac(gm, P, g2):
    """affine point -> the library's Jacobian bytes (Z = 1; infinity (1, 1, 0))"""
    if P is None:
        return gm.jac_infinity(bp.NAME, g2)
    one = pyref.encode_fp(C, 1) + (bytes(48) if g2 else b"")
    return bp.enc_points([P], g2) + one


@pytest.mark.parametrize("g2", [False, True])
def test_host_group_helpers(gm, g2):
    G = pyref.Group(C, g2)
    g = G.generator()
    assert gm.generator(bp.NAME, g2) == bp.enc_points([g], g2)
    P, Q = G.mul(g, 0x1234567890abcdef1234567), G.mul(g, bp.R - 77)
    aff = lambda a, b: gm.jac_to_affine(bp.NAME, g2, gm.jac_add(bp.NAME, g2, _jac(gm, a, g2), _jac(gm, b, g2)))
    enc = lambda X: bp.enc_points([X], g2)
    assert aff(P, Q) == enc(G.add(P, Q))
    assert aff(P, P) == enc(G.add(P, P))
    assert aff(P, G.neg(P)) == enc(None)
    assert aff(P, None) == enc(P) and aff(None, Q) == enc(Q)
    # a sum with Z != 1 goes through the Jacobian add again
    j = gm.jac_add(bp.NAME, g2, _jac(gm, P, g2), _jac(gm, Q, g2))
    j = gm.jac_add(bp.NAME, g2, j, j)
    assert gm.jac_to_affine(bp.NAME, g2, j) == enc(G.mul(G.add(P, Q), 2))


def test_precompute_layout(gm):
    L = gm.load_library()
    c, w = ctypes.c_int(), ctypes.c_int()
    assert L.gm_precompute_layout(2, 1000, 9, ctypes.byref(c), ctypes.byref(w)) == 0
    assert (c.value, w.value) == (9, 29)  # ceil(256 / 9)
    assert L.gm_precompute_layout(2, 1000, 16, ctypes.byref(c), ctypes.byref(w)) == 0 and w.value == 16
    assert L.gm_precompute_layout(3, 1000, 9, ctypes.byref(c), ctypes.byref(w)) == ERR_INVALID
    assert gm.g16_partial_bytes(2) == 4 * 3 * 48 + 3 * 2 * 48


def test_g16_finish(gm):
    """gm_g16_finish on a hand-made set of sums: the blinding of prove.go in Python."""
    G1, G2 = pyref.Group(C, False), pyref.Group(C, True)
    rng = random.Random(381)
    k = lambda: rng.randrange(1, bp.R)
    alpha, beta, delta = (G1.mul(C.g1, k()) for _ in range(3))
    beta2, delta2 = G2.mul(C.g2, k()), G2.mul(C.g2, k())
    A, B, K, Z = (G1.mul(C.g1, k()) for _ in range(4))
    B2 = G2.mul(C.g2, k())
    r_, s_ = k(), k()
    ar = G1.add(G1.add(A, alpha), G1.mul(delta, r_))
    bs1 = G1.add(G1.add(B, beta), G1.mul(delta, s_))
    krs = G1.add(G1.add(K, Z), G1.mul(delta, (-r_ * s_) % bp.R))
    krs = G1.add(G1.add(krs, G1.mul(ar, s_)), G1.mul(bs1, r_))
    bs = G2.add(G2.add(B2, G2.mul(delta2, s_)), beta2)
    keep = {n: np.frombuffer(bp.enc_points([v], n.startswith("g2")), np.uint8).copy()
            for n, v in (("g1_alpha", alpha), ("g1_beta", beta), ("g1_delta", delta), ("g2_beta", beta2),
                         ("g2_delta", delta2))}
    h = gm._PkHost()
    for n, v in keep.items():
        setattr(h, n, v.ctypes.data)
    sums = b"".join(_jac(gm, X, False) for X in (A, B, K, Z)) + _jac(gm, B2, True)
    assert len(sums) == gm.g16_partial_bytes(2)
    got = gm.g16_finish(2, h, sums, bp.enc_fr([r_]), bp.enc_fr([s_]))
    assert got == (bp.enc_points([ar], False), bp.enc_points([bs], True), bp.enc_points([krs], False))


def deferred_calls(L, ctx=None, multi=None, fd=-1):
    """(name, call(curve)) of every deferred entry that takes a curve id.  ctx None:
    NULL for the context and every pointer (the capability check comes first, so
    no device is needed); with a live context handle: that handle, real host
    buffers and a throw-away file descriptor, so that a refusal that came too
    late would allocate, upload or launch."""
    out = ctypes.c_void_p()
    o = ctypes.byref(out)
    sz = ctypes.c_size_t
    if ctx is None:
        z = zq = zp = zl = zo = zpk = zs = None
        perm = None
    else:
        keep = ctypes.create_string_buffer(4096)
        z = ctypes.cast(keep, ctypes.c_void_p)
        import gnark_mi355x as gm
        zq, zp, zl, zo = gm._PlonkQuotientIn(), gm._PlonkPermIn(), gm._PlonkLinearizeIn(), gm._PlonkLinearizeOut()
        zpk, zs = gm._PlonkPkHost(), gm._PlonkSetupHost()
        zq, zp, zl, zo, zpk, zs = (ctypes.byref(x) for x in (zq, zp, zl, zo, zpk, zs))
        perm = (ctypes.c_int64 * 24)(*range(24))
        deferred_calls.keep = (keep, perm)
    calls = [
        ("gm_plonk_quotient", lambda cv: L.gm_plonk_quotient(ctx, cv, zq, z)),
        ("gm_plonk_perm_z", lambda cv: L.gm_plonk_perm_z(ctx, cv, zp, z, z)),
        ("gm_plonk_linearize", lambda cv: L.gm_plonk_linearize(ctx, cv, zl, zo)),
        ("gm_plonk_pk_upload", lambda cv: L.gm_plonk_pk_upload(ctx, cv, zpk, 0, o)),
        ("gm_kzg_srs_lagrange", lambda cv: L.gm_kzg_srs_lagrange(ctx, cv, z, sz(8), z)),
        ("gm_plonk_sigma", lambda cv: L.gm_plonk_sigma(ctx, cv, sz(8), perm, z, z, z)),
        ("gm_plonk_pk_setup", lambda cv: L.gm_plonk_pk_setup(ctx, cv, zs, 0, o, z, z)),
        ("gm_plonk_sigma_wires", lambda cv: L.gm_plonk_sigma_wires(ctx, cv, z, z, z, z)),
        ("gm_plonk_pk_setup_wires", lambda cv: L.gm_plonk_pk_setup_wires(ctx, cv, zs, z, 0, o, z, z)),
        ("gm_batch_mul_base", lambda cv: L.gm_batch_mul_base(ctx, cv, 0, z, z, sz(1), z)),
        ("gm_batch_mul_fixed", lambda cv: L.gm_batch_mul_fixed(ctx, cv, 0, z, z, sz(1), z)),
        ("gm_r1cs_upload", lambda cv: L.gm_r1cs_upload(ctx, cv, sz(1), sz(1), z, z, z, z, sz(2), o)),
        ("gm_g16_pk_upload_shard", lambda cv: L.gm_g16_pk_upload_shard(ctx, cv, z, 0, 0, 1, o)),
        ("gm_g16_pk_upload_multi", lambda cv: L.gm_g16_pk_upload_multi(multi, cv, z, 0, o)),
        ("gm_g16_pk_upload_dump", lambda cv: L.gm_g16_pk_upload_dump(ctx, cv, z, fd, 0, 0, None, o)),
        ("gm_g16_pk_upload_dump_shard", lambda cv: L.gm_g16_pk_upload_dump_shard(ctx, cv, z, fd, 0, 0, 0, 1, None, o)),
        ("gm_icicle_generate_twiddles", lambda cv: L.gm_icicle_generate_twiddles(ctx, cv, sz(8), 0, o)),
        ("gm_icicle_intt_on_device", lambda cv: L.gm_icicle_intt_on_device(ctx, cv, z, sz(8), 0, o)),
        ("gm_icicle_ntt_on_device", lambda cv: L.gm_icicle_ntt_on_device(ctx, cv, z, z, sz(8), 0)),
        ("gm_icicle_poly_ops", lambda cv: L.gm_icicle_poly_ops(ctx, cv, z, z, z, z, sz(8))),
    ]
    return calls


def check_refusals(L, calls):
    for name, call in calls:
        assert call(2) == ERR_UNSUPPORTED, name
        msg = L.gm_last_error().decode()
        assert "BLS12-381" in msg and "curve id 2" in msg, (name, msg)
        # the dump entry without a rank is the shard entry's rank 0 of 1
        assert name in msg or (name == "gm_g16_pk_upload_dump" and "gm_g16_pk_upload_dump_shard" in msg), (name, msg)


def test_deferred_entries_refuse_bls12381(gm):
    L = gm.load_library()
    calls = deferred_calls(L)
    check_refusals(L, calls)
    for name, call in calls:
        assert call(3) == ERR_INVALID, name
        assert "unknown curve id" in L.gm_last_error().decode(), name
        assert call(-1) == ERR_INVALID, name


def test_in_scope_host_entries_know_three_curves(gm):
    L = gm.load_library()
    buf = ctypes.create_string_buffer(4 * 48 * 3)
    for cv in (0, 1, 2):
        assert L.gm_generator(cv, 1, buf) == 0
    for cv in (3, -1, 7):
        assert L.gm_generator(cv, 0, buf) == ERR_INVALID
        assert L.gm_jac_add(cv, 0, buf, buf, buf) == ERR_INVALID
        assert L.gm_jac_to_affine(cv, 0, buf, buf) == ERR_INVALID
        assert L.gm_g16_partial_bytes(cv, None) == ERR_INVALID


def test_glv_split_model():
    """The balanced split of tools/glv_constants.py (the device code's model) on
    the special scalars and 20,000 random ones: halves below 2^127, every sign
    combination, k = +-k1 +- k2 lambda mod r."""
    import glv_constants as glv
    d = glv.derive_bls12381()
    assert d["lam"] == bp.LAMBDA and glv.GLV_HALF_BITS == 127
    rng = random.Random(5)
    ks = glv.specials_bls12381(d) + [rng.randrange(bp.R) for _ in range(20000)]
    signs = set()
    for k in ks:
        k1, n1, k2, n2 = glv.check_split_bls12381(k, d)
        signs.add((n1, n2))
    assert signs == {(0, 0), (0, 1), (1, 0), (1, 1)}
    # each half reaches its largest magnitude on the specials
    sp = [glv.split_bls12381(k, d) for k in glv.specials_bls12381(d)]
    assert max(s[0] for s in sp) == bp.LAMBDA >> 1 and max(s[2] for s in sp) >= (bp.LAMBDA + 1) // 2
    # phi on both groups with the printed betas
    G1, G2 = pyref.Group(C, False), pyref.Group(C, True)
    P, Q = G1.mul(C.g1, 12345), G2.mul(C.g2, 6789)
    assert G1.mul(P, bp.LAMBDA) == (d["beta"] * P[0] % bp.P, P[1])
    assert G2.mul(Q, bp.LAMBDA) == ((Q[0][0] * d["beta_g2"] % bp.P, Q[0][1] * d["beta_g2"] % bp.P), Q[1])


def test_msm_geometry_half_width(gm):
    """GLV plans of this curve: 127-bit halves, 8 windows at c = 16"""
    g = gm.msm_geometry(2, False, 1 << 20, 16, gm.TGEOM_GLV)
    assert g["W"] == 8 and g["n"] == 2 << 20
    g = gm.msm_geometry(2, False, 1 << 20, 16, gm.TGEOM_PLAIN)
    assert g["W"] == 16  # 256 bits of digits for the 255-bit field
