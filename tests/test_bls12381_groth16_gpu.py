"""BLS12-381 (curve id 2) Groth16 prover against pyref.g16_setup / g16_prove with
the curve's CurveParams: proof bytes identical for host and device inputs, plain
and precomputed keys; and the deferred entries' refusals on a live context."""
import ctypes
import os
import struct

import numpy as np
import pytest

import pyref
import bls12381_params as bp
from test_bls12381_abi import deferred_calls, check_refusals, ERR_UNSUPPORTED

pytestmark = pytest.mark.gpu
C, R = bp.C, bp.R
TOXIC = [0x1D5A2B3C4D5E6F708192A3B4C5D6E7F8091A2B3C4D5E6F708192A3B4C5D6E7,
         0x2E6B3C4D5E6F708192A3B4C5D6E7F8091A2B3C4D5E6F708192A3B4C5D6E7F8,
         0x3F7C4D5E6F708192A3B4C5D6E7F8091A2B3C4D5E6F708192A3B4C5D6E7F809,
         0x0A8D5E6F708192A3B4C5D6E7F8091A2B3C4D5E6F708192A3B4C5D6E7F8091A,
         0x1B9E6F708192A3B4C5D6E7F8091A2B3C4D5E6F708192A3B4C5D6E7F8091A2B]
CIRCUITS = {"cubic": bp.cubic_circuit, "chain15": lambda: bp.squaring_chain(15), "chain63": lambda: bp.squaring_chain(63, 3)}


@pytest.fixture(scope="module")
def keys():
    """circuit -> (pyref key, its byte arrays, witness, a, b, c, expected proof bytes)"""
    out = {}
    for name, make in CIRCUITS.items():
        cons, nb_wires, nb_public, W = make()
        a, b, c = bp.solve_abc(cons, W)
        assert all(x * y % R == z for x, y, z in zip(a, b, c))
        pk = pyref.g16_setup(C, cons, nb_wires, nb_public, TOXIC)
        rr, ss = 0xABCDEF0123 + len(cons), R - 0x13579BDF
        ar, bs, krs = pyref.g16_prove(C, pk, W, a, b, c, rr, ss)
        exp = (bp.enc_points([ar], False), bp.enc_points([bs], True), bp.enc_points([krs], False))
        out[name] = dict(pk=pk, pkb=bp.pk_bytes(pk), W=W, abc=(a, b, c), rs=(rr, ss), exp=exp, nb_wires=nb_wires,
                         nb_public=nb_public)
    return out


@pytest.mark.parametrize("precompute", [False, True, "auto"])
@pytest.mark.parametrize("name", list(CIRCUITS))
def test_prove(gm_ctx, keys, name, precompute):
    import gnark_mi355x as gm
    k = keys[name]
    enc = bp.enc_fr
    a, b, c = k["abc"]
    rb, sb = enc([k["rs"][0]]), enc([k["rs"][1]])
    dpk = gm.ProvingKey(gm_ctx, 2, k["pkb"], k["pk"]["n"], k["nb_wires"], k["nb_public"], precompute=precompute)
    try:
        if precompute is True:
            assert dpk.precomputed
        for _ in range(3):  # three proofs leave the key unchanged
            assert dpk.prove(enc(k["W"]), enc(a), enc(b), enc(c), rb, sb) == k["exp"], (name, precompute, "host")
        n = k["pk"]["n"]
        Wd = gm_ctx.copy_to_device(enc(k["W"]))
        bufs = [gm_ctx.malloc(32 * n) for _ in range(3)]
        try:
            for B_, v in zip(bufs, (a, b, c)):
                B_.write(enc(v))
            assert dpk.prove_device(Wd, *bufs, len(a), rb, sb) == k["exp"], (name, precompute, "device")
        finally:
            for x in bufs + [Wd]:
                x.free()
    finally:
        dpk.free()


def _bn254_cubic_key():
    c = pyref.BN254
    cons, nb_wires, nb_public, _ = bp.cubic_circuit()
    pk = pyref.g16_setup(c, cons, nb_wires, nb_public, TOXIC)
    enc = lambda pts, g2: b"".join(pyref.encode_point(c, P, g2) for P in pts)
    out = {k: enc([pk[k]], k.startswith("g2")) for k in ("g1_alpha", "g1_beta", "g1_delta", "g2_beta", "g2_delta")}
    for k in ("g1_A", "g1_B", "g1_Z", "g1_K", "g2_B"):
        out[k] = enc(pk[k], k.startswith("g2"))
    out["infA"] = np.array(pk["infA"], dtype=np.uint8)
    out["infB"] = np.array(pk["infB"], dtype=np.uint8)
    return out, pk["n"], nb_wires, nb_public


def test_deferred_entries_refuse_on_live_context(gm_ctx, keys, tmp_path):
    """Every deferred entry, called with the live context, real host buffers and a
    throw-away file, answers GM_ERR_UNSUPPORTED for curve 2 and names it; so do the
    key-bound ones for a BLS12-381 key and the cache loader for a cache whose
    header says curve 2.  Nothing is written to the file, and the context works
    afterwards."""
    import gnark_mi355x as gm
    L = gm.load_library()
    scratch = tmp_path / "never_written"
    fd = os.open(scratch, os.O_RDWR | os.O_CREAT, 0o600)
    dev = ctypes.c_int(0)
    multi = ctypes.c_void_p()
    assert L.gm_multi_init(ctypes.byref(dev), 1, ctypes.byref(multi)) == 0
    k = keys["cubic"]
    dpk = gm.ProvingKey(gm_ctx, 2, k["pkb"], k["pk"]["n"], k["nb_wires"], k["nb_public"])
    try:
        check_refusals(L, deferred_calls(L, gm_ctx.handle, multi, fd))
        h = ctypes.c_void_p()
        out = ctypes.create_string_buffer(gm.g16_partial_bytes(2))
        check_refusals(L, (
            ("gm_g16_stage_begin", lambda cv: L.gm_g16_stage_begin(gm_ctx.handle, dpk.handle, 3, ctypes.byref(h))),
            ("gm_g16_pk_save_cache", lambda cv: L.gm_g16_pk_save_cache(gm_ctx.handle, dpk.handle, fd)),
            ("gm_g16_prove_partial", lambda cv: L.gm_g16_prove_partial(gm_ctx.handle, dpk.handle, None, None, None,
                                                                       None, 3, out))))
        with pytest.raises(gm.GmError):
            gm.ProvingKey(gm_ctx, 2, k["pkb"], k["pk"]["n"], k["nb_wires"], k["nb_public"], shard=(0, 1))
        assert os.fstat(fd).st_size == 0
        # a BN254 key's cache with the header's curve field (offset 12) set to 2
        pkb, n, nw, npub = _bn254_cubic_key()
        bn = gm.ProvingKey(gm_ctx, 0, pkb, n, nw, npub)
        try:
            path = str(tmp_path / "bn254.cache")
            bn.save_cache(path)
        finally:
            bn.free()
        raw = bytearray(open(path, "rb").read())
        assert struct.unpack_from("<I", raw, 12)[0] == 0
        struct.pack_into("<I", raw, 12, 2)
        open(path, "wb").write(raw)
        cfd = os.open(path, os.O_RDONLY)
        try:
            check_refusals(L, (("gm_g16_pk_load_cache",
                                lambda cv: L.gm_g16_pk_load_cache(gm_ctx.handle, cfd, ctypes.byref(h))),))
        finally:
            os.close(cfd)
        a, b, c = k["abc"]
        enc = bp.enc_fr
        got = dpk.prove(enc(k["W"]), enc(a), enc(b), enc(c), enc([k["rs"][0]]), enc([k["rs"][1]]))
        assert got == k["exp"]
    finally:
        dpk.free()
        os.close(fd)
        L.gm_multi_destroy(multi)
    # the context still serves the other curves
    data = b"".join(pyref.encode_fr(pyref.BN254, v) for v in (1, 2, 3, 4))
    X = gm_ctx.copy_to_device(data)
    try:
        gm_ctx.ntt(0, X, 4, False, False, False)
        gm_ctx.ntt(0, X, 4, True, True, False)
        assert X.to_host() == data
    finally:
        X.free()
