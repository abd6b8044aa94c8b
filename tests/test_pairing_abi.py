"""Pairing-product checks and Groth16 verification without a GPU: the generated
constants, the integer model proving itself (tests/pairing_model.py), the
model's verdict on three of the external bellman vectors, the symbols, and the
refusals that are decided before any device call."""
import ctypes
import os
import random
import re
import sys

import pytest

import pyref
import pairing_model as pm
import points_codec_model as codec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
CURVES = ("bn254", "bls12377", "bls12381")
ERR_INVALID = -1
NEW_SYMBOLS = ("gm_pairing_check", "gm_pairing_check_device", "gm_g16_vk_upload", "gm_g16_vk_free",
               "gm_g16_verify_batch")


def test_constants_header_is_what_the_tool_generates():
    import pairing_constants
    assert open(pairing_constants.HEADER).read() == pairing_constants.header()


@pytest.mark.parametrize("name", CURVES)
def test_model_proves_itself(name):
    m = pm.model(name)
    g1, g2 = m.G1.generator(), m.G2.generator()
    e = m.pair(g1, g2)
    assert not m.is_one(e)
    assert m.is_one(m.pow(e, m.r))
    rng = random.Random(0xE11 + len(name))
    for _ in range(2):
        a, b = rng.randrange(1, m.r), rng.randrange(1, m.r)
        assert m.pair(m.G1.mul(g1, a), m.G2.mul(g2, b)) == m.pow(e, a * b % m.r)
    # the Frobenius the model builds from w^p = gamma w is the p-th power
    x = [(rng.randrange(m.p), rng.randrange(m.p)) for _ in range(6)]
    assert m.frob(x) == m.pow(x, m.p)
    assert m.pair(None, g2) == m.one() and m.pair(g1, None) == m.one()


def bellman_decoded(v):
    """The vector's points by the codec model (None where a record does not
    decode), as (vk dict for Model.groth16_verify, proof, inputs)."""
    def dec(rec, g2):
        cls, inf, P = codec.decode("bls12381", g2, rec, codec.COMPRESSED)
        if cls != codec.OK:
            raise ValueError("record does not decode")
        return None if inf else P
    vk = v["vk"]
    key = dict(alpha_g1=dec(vk["alpha_g1"], False), beta_g2=dec(vk["beta_g2"], True), gamma_g2=dec(vk["gamma_g2"], True),
               delta_g2=dec(vk["delta_g2"], True), k=[dec(r, False) for r in vk["k"]])
    A, B, C = v["proof"]
    return key, (dec(A, False), dec(B, True), dec(C, False)), v["inputs"]


def test_bellman_fixture_shape():
    vs = pm.bellman_vectors()
    assert len(vs) == 12
    assert [v["ok"] for v in vs] == [True, False, False, True, True, True, True, True, False, False, False, False]
    assert sorted({len(v["inputs"]) for v in vs}) == [0, 1, 15, 16, 17]


@pytest.mark.parametrize("idx", [0, 1, 3])
def test_model_verdict_on_bellman_vectors(idx):
    v = pm.bellman_vectors()[idx]
    m = pm.model("bls12381")
    try:
        key, proof, inputs = bellman_decoded(v)
        got = m.groth16_verify(key, proof, inputs)
    except ValueError:
        got = False
    assert got == v["ok"]


def _declared(header):
    return set(re.findall(r"\b(gm_[a-z0-9_]+)\s*\(", open(os.path.join(ROOT, "include", header)).read()))


@pytest.fixture(scope="module")
def lib():
    import gnark_mi355x as gm
    return gm.load_library()


def test_symbols(lib):
    import gnark_mi355x as gm
    for s in NEW_SYMBOLS:
        assert s in gm.SYMBOLS and s in _declared("gnark_mi355x.h") and hasattr(lib, s), s
    assert "gm_test_pairing_op" in gm.TEST_SYMBOLS and "gm_test_pairing_op" in _declared("gnark_mi355x_testhooks.h")
    assert not hasattr(lib, "gm_test_pairing_op")
    assert hasattr(gm.load_testhooks(), "gm_test_pairing_op")


def test_refusals_before_any_device_call(lib):
    """Decided from the arguments alone; the context pointer is never followed
    (a zeroed block stands in for it where a non-NULL one is needed)."""
    import gnark_mi355x as gm
    err = lambda: lib.gm_last_error().decode()
    fake = ctypes.create_string_buffer(4096)
    ctx = ctypes.cast(fake, ctypes.c_void_p)
    pts = ctypes.create_string_buffer(1024)
    ok = ctypes.create_string_buffer(b"\xEE" * 8, 8)
    for entry in (lib.gm_pairing_check, lib.gm_pairing_check_device):
        for bad in (-1, 3, 7):
            assert entry(ctx, bad, pts, pts, 1, 1, ok) == ERR_INVALID and "unknown curve id" in err()
        for curve in (0, 1, 2):
            assert entry(None, curve, pts, pts, 1, 1, ok) == ERR_INVALID and "NULL" in err()
            assert entry(ctx, curve, None, pts, 1, 1, ok) == ERR_INVALID and "NULL" in err()
            assert entry(ctx, curve, pts, None, 1, 1, ok) == ERR_INVALID
            assert entry(ctx, curve, pts, pts, 1, 1, None) == ERR_INVALID
            assert entry(ctx, curve, pts, pts, 1, 0, ok) == ERR_INVALID and "k must be" in err()
            assert entry(ctx, curve, pts, pts, 1 << 40, 1 << 40, ok) == ERR_INVALID and "address space" in err()
            assert entry(ctx, curve, pts, pts, 0, 3, ok) == 0          # nothing to do, nothing written
    assert ok.raw == b"\xEE" * 8
    mis = ctypes.c_void_p(ctypes.addressof(pts) + 8 - ctypes.addressof(pts) % 16)
    assert lib.gm_pairing_check_device(ctx, 0, mis, pts, 1, 1, ok) == ERR_INVALID and "aligned" in err()
    # the verifying key
    h = ctypes.c_void_p()
    mk = lambda **kw: gm._G16VkHost(**{**dict(alpha_g1=ctypes.addressof(pts), beta_g2=ctypes.addressof(pts),
                                              gamma_g2=ctypes.addressof(pts), delta_g2=ctypes.addressof(pts),
                                              k_g1=ctypes.addressof(pts), nb_k=1), **kw})
    assert lib.gm_g16_vk_upload(ctx, 5, ctypes.byref(mk()), ctypes.byref(h)) == ERR_INVALID and "unknown curve id" in err()
    assert lib.gm_g16_vk_upload(None, 0, ctypes.byref(mk()), ctypes.byref(h)) == ERR_INVALID
    assert lib.gm_g16_vk_upload(ctx, 0, None, ctypes.byref(h)) == ERR_INVALID
    assert lib.gm_g16_vk_upload(ctx, 0, ctypes.byref(mk()), None) == ERR_INVALID
    for member in ("alpha_g1", "beta_g2", "gamma_g2", "delta_g2", "k_g1"):
        assert lib.gm_g16_vk_upload(ctx, 2, ctypes.byref(mk(**{member: None})), ctypes.byref(h)) == ERR_INVALID, member
        assert "NULL" in err()
    assert lib.gm_g16_vk_upload(ctx, 1, ctypes.byref(mk(nb_k=0)), ctypes.byref(h)) == ERR_INVALID and "nb_k" in err()
    assert lib.gm_g16_vk_free(ctx, None) == ERR_INVALID
    assert lib.gm_g16_verify_batch(ctx, None, pts, pts, 1, ok, None) == ERR_INVALID
    assert lib.gm_g16_verify_batch(None, None, pts, pts, 1, ok, None) == ERR_INVALID
