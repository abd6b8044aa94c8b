"""The point codec without a GPU: the Python model of gnark-crypto's encodings
(points_codec_model) on the point-check corpus, the generated square-root
constants, the entries through header, library, binding and Makefile, and every
refusal that needs no device."""
import ctypes
import os
import subprocess
import sys

import pytest

import points_check_cases as pc
import points_codec_model as m
import pyref
from points_check_cases import sub

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import sqrt_constants as sq  # noqa: E402

HEADER = os.path.join(ROOT, "include", "gnark_mi355x.h")
NAMES = ("gm_points_decode", "gm_points_decode_host", "gm_points_encode", "gm_g16_pk_upload_encoded")
OK, ERR_INVALID = 0, -1
WIDTHS = (m.COMPRESSED, m.RAW)


@pytest.mark.parametrize("cname,g2", pc.GROUPS)
def test_model_round_trips_every_valid_point(cname, g2):
    c = pc.params(cname)
    G = pyref.Group(c, g2)
    valid = m.corpus_points(cname, g2, pc.OK)
    assert len(valid) >= 7
    for width in WIDTHS:
        for name, P in valid + [("-" + n, G.neg(P)) for n, P in valid]:
            rec = m.encode(cname, g2, P, width)
            assert len(rec) == m.record_bytes(c, g2, width)
            assert m.decode(cname, g2, rec, width) == (m.OK, False, P), (name, width)
            assert m.decode(cname, g2, rec, width, m.NO_SUBGROUP_CHECK) == (m.OK, False, P), (name, width)
        assert m.decode(cname, g2, m.encode(cname, g2, None, width), width) == (m.OK, True, None)
    # the compressed flag follows y: P and -P differ in the flag bit alone
    _, P = valid[0]
    a, b = m.encode(cname, g2, P, m.COMPRESSED), m.encode(cname, g2, G.neg(P), m.COMPRESSED)
    assert a[1:] == b[1:] and a[0] ^ b[0] == 1 << (8 - m.flag_bits(cname))


def test_raw_infinity_records_are_the_oracles():
    for cname in ("bn254", "bls12377"):
        c = pyref.CURVES[cname]
        assert m.encode(cname, False, None, m.RAW) == pyref.marshal_g1(c, None)
        P = pyref.Group(c, False).generator()
        assert m.encode(cname, False, P, m.RAW) == pyref.marshal_g1(c, P)
    import bls12381_params as bp
    assert m.encode("bls12381", False, None, m.RAW) == pyref.marshal_g1(bp.C, None)


def test_bls12381_generator_compresses_to_the_zcash_vector():
    import bls12381_params as bp
    G = pyref.Group(bp.C, False)
    want = bytes.fromhex("97f1d3a73197d7942695638c4fa9ac0fc3688c4f9774b905a14e3a3f171bac58"
                         "6c55e83ff97a1aeffb3af00adb22c6bb")
    assert m.encode("bls12381", False, G.generator(), m.COMPRESSED) == want
    assert m.decode("bls12381", False, want, m.COMPRESSED) == (m.OK, False, G.generator())


@pytest.mark.parametrize("cname,g2", pc.GROUPS)
def test_every_case_is_what_its_name_says(cname, g2):
    """The model decides the class; the case lists state the intent.  The coverage
    the GPU test relies on is asserted here too: every kind is present wherever
    the curve admits it."""
    for width in WIDTHS:
        cs = m.decode_cases(cname, g2, width)
        for kind, name, rec, want in cs:
            assert m.decode(cname, g2, rec, width)[0] == want, (kind, name, width)
        kinds = {k for k, _, _, _ in cs}
        expect = {"valid", "infinity", "other width", "not reduced"}
        expect |= {"flip", "no root"} if width == m.COMPRESSED else {"off curve"}
        if g2:
            expect |= {"not reduced a1", "not reduced a0"}
        if not m.is_bn(cname):
            expect |= {"invalid flag", "stray"}          # BN254 uses all four flags
        elif width == m.COMPRESSED:
            expect |= {"stray"}                          # BN254's raw infinity has no flag to stray from
        if (cname, g2) != ("bn254", False):
            expect |= {"off subgroup"}                   # BN254 G1 has cofactor 1
        assert kinds - {"y = 0"} == expect, (width, kinds ^ expect)


def test_y_zero_cases_are_there_exactly_where_the_group_has_even_order():
    """A point with y = 0 is a point of order 2, so the curve (or twist) has one
    exactly when its group order h r is even (r is odd); such a point is never in
    the subgroup, which is why the cases come from the off-subgroup corpus.  The
    case lists must hold one for every such pair, in both widths, and cannot for
    the others.  Of the six pairs only BLS12-377 G1 has even order (u is odd, so
    h1 = (u - 1)^2 / 3 is even; every other cofactor is odd)."""
    even = {}
    for cname, g2 in pc.GROUPS:
        d = pc.derived(cname)
        c = d["c"]
        order = (d["h2"] if g2 else d["h1"]) * c.r
        G = pyref.Group(c, g2)
        for P in sub.random_curve_points(c, g2, 2, 0xE0 + int(g2)):
            assert G.mul(P, order) is None               # h r is the group's order
        even[(cname, g2)] = order % 2 == 0
        for width in WIDTHS:
            cs = m.decode_cases(cname, g2, width)
            y0 = [rec for k, _, rec, _ in cs if k == "y = 0"]
            assert bool(y0) == even[(cname, g2)], (cname, g2, width)
            assert len(y0) == (0 if not y0 else (2 if width == m.COMPRESSED else 1))   # both flags when compressed
            for rec in y0:
                P = m.decode(cname, g2, rec, width, m.NO_SUBGROUP_CHECK)[2]
                assert G.F.is_zero(P[1]) and G.on_curve(P) and G.mul(P, 2) is None
    assert even == {(c, g): (c, g) == ("bls12377", False) for c, g in pc.GROUPS}


def test_no_subgroup_check_keeps_the_three_encoding_classes():
    for cname, g2 in pc.GROUPS:
        for width in WIDTHS:
            for kind, name, rec, want in m.decode_cases(cname, g2, width):
                got = m.decode(cname, g2, rec, width, m.NO_SUBGROUP_CHECK)[0]
                assert got == (want if want in (m.BAD_ENCODING, m.NOT_REDUCED, m.NO_ROOT) else m.OK), (kind, name)


@pytest.mark.parametrize("cname", pc.CURVE_NAMES)
def test_square_root_constants(cname):
    """derive() asserts the identities; they are restated here on its results."""
    d = sq.derive(cname)
    p, S, s = d["p"], d["S"], d["s"]
    assert p - 1 == s << S and s & 1
    assert (S == 1) == (p % 4 == 3) and (cname == "bls12377") == (S == 46)
    assert pow(d["root"], 1 << (S - 1), p) == p - 1
    assert d["exp"] == ((p + 1) // 4 if S == 1 else (s - 1) // 2)
    assert 2 * d["half_p"] + 1 == p and 2 * d["inv2"] % p == 1
    assert d["beta_inv"] * d["c"].beta % p == 1 and d["exp"] < 1 << (32 * d["exp_words"])
    # every order 2^k of a^s occurs among squares: root^(2^(S - k)) has order 2^k
    if S > 1:
        for k in (0, 1, S - 1):
            t = pow(d["root"], 1 << (S - k), p)
            assert pow(t, 1 << k, p) == 1 and (k == 0 or pow(t, 1 << (k - 1), p) != 1)


def test_generated_header_is_what_the_tool_prints():
    text = open(sq.HEADER).read()
    assert text == sq.header()
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "sqrt_constants.py"), "--print"],
                         capture_output=True, text=True, check=True).stdout
    assert out == text


def test_header_library_binding_and_makefile_have_the_entries():
    import gnark_mi355x as gm
    src = open(HEADER).read()
    lo, hi = src.index("---- point encodings"), src.index("---- staged prover inputs")
    for name in NAMES:
        assert lo < src.index("int %s(" % name) < hi
    assert "GM_POINT_BAD_ENCODING = 4, GM_POINT_NO_ROOT = 5" in src and "} gm_points_decode_report;" in src
    # the existing classes and report are untouched
    assert "GM_POINT_OK = 0, GM_POINT_NOT_REDUCED = 1, GM_POINT_OFF_CURVE = 2, GM_POINT_OFF_SUBGROUP = 3" in src
    assert ctypes.sizeof(gm._PointsReport) == 56 and ctypes.sizeof(gm._PointsDecodeReport) == 72
    assert ctypes.sizeof(gm._G16PkDecodeReport) == 728 and "} gm_g16_pk_decode_report;" in src
    assert callable(gm.ProvingKey.from_encoded)
    L = gm.load_library()
    for name in NAMES:
        assert name in gm.SYMBOLS and hasattr(L, name), name
    assert "gm_test_fe_sqrt" in gm.TEST_SYMBOLS and hasattr(gm.load_testhooks(), "gm_test_fe_sqrt")
    assert not hasattr(L, "gm_test_fe_sqrt")
    for method in ("points_decode", "points_decode_host", "points_encode"):
        assert callable(getattr(gm.Context, method))
    assert (gm.POINT_BAD_ENCODING, gm.POINT_NO_ROOT, gm.ENC_COMPRESSED, gm.ENC_RAW,
            gm.DECODE_NO_SUBGROUP_CHECK) == (4, 5, 0, 1, 0x100)
    assert (m.BAD_ENCODING, m.NO_ROOT, m.COMPRESSED, m.RAW, m.NO_SUBGROUP_CHECK) == (4, 5, 0, 1, 0x100)
    mk = open(os.path.join(ROOT, "gnark-icicle_amd", "Makefile")).read()
    srcs = mk[mk.index("SRCS :="):mk.index("OBJS :=")]
    for unit in ("points_codec", "points_codec_bn254", "points_codec_bls12377", "points_codec_bls12381"):
        assert "csrc/%s.hip" % unit in srcs
        assert os.path.exists(os.path.join(ROOT, "gnark-icicle_amd", "csrc", unit + ".hip"))
    for cname, g2 in pc.GROUPS:
        for width in WIDTHS:
            assert gm.record_bytes(cname, g2, width) == m.record_bytes(pc.params(cname), g2, width)


def test_refusals_before_any_device_call():
    """No context exists in this process and `x` is never dereferenced: a call that
    got past its refusal would fail with another code or not return at all."""
    import gnark_mi355x as gm
    L = gm.load_library()
    vp = ctypes.c_void_p
    x, y, odd = vp(0x10000), vp(0x80000), vp(0x10008)
    rep, bad = gm._PointsDecodeReport(), ctypes.c_uint64()
    r, b = ctypes.byref(rep), ctypes.byref(bad)
    null = "null"
    cases = [
        ("gm_points_decode", null, lambda: L.gm_points_decode(None, 0, 0, 0, 0, x, 4, y, None, r)),
        ("gm_points_decode", null, lambda: L.gm_points_decode(x, 0, 0, 0, 0, None, 4, y, None, r)),
        ("gm_points_decode", null, lambda: L.gm_points_decode(x, 0, 0, 0, 0, x, 4, None, None, r)),
        ("gm_points_decode", null, lambda: L.gm_points_decode(x, 0, 0, 0, 0, x, 4, y, None, None)),
        ("gm_points_decode", "g2", lambda: L.gm_points_decode(x, 0, 2, 0, 0, x, 4, y, None, r)),
        ("gm_points_decode", "encoding", lambda: L.gm_points_decode(x, 1, 1, 2, 0, x, 4, y, None, r)),
        ("gm_points_decode", "encoding", lambda: L.gm_points_decode(x, 1, 1, -1, 0, x, 4, y, None, r)),
        ("gm_points_decode", "flags", lambda: L.gm_points_decode(x, 2, 0, 1, 2, x, 4, y, None, r)),
        ("gm_points_decode", "aligned", lambda: L.gm_points_decode(x, 2, 0, 1, 0, odd, 4, y, None, r)),
        ("gm_points_decode", "aligned", lambda: L.gm_points_decode(x, 2, 0, 1, 0x100, x, 4, odd, None, r)),
        ("gm_points_decode", "overlap", lambda: L.gm_points_decode(x, 0, 0, 0, 0, x, 4, x, None, r)),
        ("gm_points_decode", "overlap", lambda: L.gm_points_decode(x, 0, 0, 0, 0, x, 4, vp(0x10000 + 96), None, r)),
        ("gm_points_decode", "overlap", lambda: L.gm_points_decode(x, 0, 0, 0, 0, x, 4, y, vp(0x80000 + 255), r)),
        ("gm_points_decode", "address space", lambda: L.gm_points_decode(x, 1, 1, 0, 0, x, 1 << 62, y, None, r)),
        ("gm_points_decode_host", null, lambda: L.gm_points_decode_host(None, 0, 0, 0, 0, x, 4, y, None, r)),
        ("gm_points_decode_host", null, lambda: L.gm_points_decode_host(x, 0, 0, 0, 0, None, 4, y, None, r)),
        ("gm_points_decode_host", null, lambda: L.gm_points_decode_host(x, 0, 0, 0, 0, x, 4, y, None, None)),
        ("gm_points_decode_host", "both null", lambda: L.gm_points_decode_host(x, 0, 0, 0, 0, x, 4, None, None, r)),
        ("gm_points_decode_host", "g2", lambda: L.gm_points_decode_host(x, 0, -1, 0, 0, x, 4, y, None, r)),
        ("gm_points_decode_host", "encoding", lambda: L.gm_points_decode_host(x, 0, 0, 7, 0, x, 4, y, None, r)),
        ("gm_points_decode_host", "flags", lambda: L.gm_points_decode_host(x, 0, 0, 0, 4, x, 4, y, None, r)),
        ("gm_points_decode_host", "aligned", lambda: L.gm_points_decode_host(x, 0, 0, 0, 0, x, 4, odd, None, r)),
        ("gm_points_decode_host", "overlap", lambda: L.gm_points_decode_host(x, 0, 0, 1, 0, x, 4, None, x, r)),
        ("gm_points_encode", null, lambda: L.gm_points_encode(None, 0, 0, 0, x, 4, y, b)),
        ("gm_points_encode", null, lambda: L.gm_points_encode(x, 0, 0, 0, None, 4, y, b)),
        ("gm_points_encode", null, lambda: L.gm_points_encode(x, 0, 0, 0, x, 4, None, b)),
        ("gm_points_encode", null, lambda: L.gm_points_encode(x, 0, 0, 0, x, 4, y, None)),
        ("gm_points_encode", "g2", lambda: L.gm_points_encode(x, 0, 3, 0, x, 4, y, b)),
        ("gm_points_encode", "encoding", lambda: L.gm_points_encode(x, 0, 0, 2, x, 4, y, b)),
        ("gm_points_encode", "aligned", lambda: L.gm_points_encode(x, 0, 0, 0, odd, 4, y, b)),
        ("gm_points_encode", "overlap", lambda: L.gm_points_encode(x, 0, 0, 0, x, 4, vp(0x10000 + 240), b)),
    ]
    h = gm._PkHost()
    h.domain_size, h.nbA, h.nbB, h.nbK = 8, 3, 2, 4
    hp, krep, end, pk = ctypes.byref(h), gm._G16PkDecodeReport(), ctypes.c_uint64(), ctypes.c_void_p()
    kr, pp = ctypes.byref(krep), ctypes.byref(pk)
    small = gm._PkHost()
    small.domain_size = 1
    enc = "gm_g16_pk_upload_encoded"
    cases += [
        (enc, null, lambda: L.gm_g16_pk_upload_encoded(None, 0, hp, 0, 0, 0, 0, x, kr, None, pp)),
        (enc, null, lambda: L.gm_g16_pk_upload_encoded(x, 0, None, 0, 0, 0, 0, x, kr, None, pp)),
        (enc, null, lambda: L.gm_g16_pk_upload_encoded(x, 0, hp, 0, 0, 0, 0, None, kr, None, pp)),
        (enc, null, lambda: L.gm_g16_pk_upload_encoded(x, 0, hp, 0, 0, 0, 0, x, None, None, pp)),
        (enc, null, lambda: L.gm_g16_pk_upload_encoded(x, 0, hp, 0, 0, 0, 0, x, kr, None, None)),
        (enc, "file descriptor", lambda: L.gm_g16_pk_upload_encoded(x, 1, hp, -1, 0, 0, 0, x, kr, None, pp)),
        (enc, "domain_size", lambda: L.gm_g16_pk_upload_encoded(x, 1, ctypes.byref(small), 0, 0, 0, 0, x, kr, None, pp)),
        (enc, "encoding", lambda: L.gm_g16_pk_upload_encoded(x, 0, hp, 0, 0, 2, 0, x, kr, None, pp)),
        (enc, "flags", lambda: L.gm_g16_pk_upload_encoded(x, 0, hp, 0, 0, 1, 4, x, kr, None, pp)),
        (enc, "flags", lambda: L.gm_g16_pk_upload_encoded(x, 0, hp, 0, 0, 1, 0x200, x, kr, None, pp)),
    ]
    for k, (entry, word, call) in enumerate(cases):
        assert call() == ERR_INVALID, (k, entry)
        msg = L.gm_last_error().decode()
        assert entry in msg and word.lower() in msg.lower(), (k, entry, msg)
    assert L.gm_g16_pk_upload_encoded(x, 2, hp, 0, 0, 0, 0, x, kr, None, pp) == -4
    assert "BLS12-381" in L.gm_last_error().decode()
    for curve in (3, -1):
        for call in (lambda: L.gm_points_decode(x, curve, 0, 0, 0, x, 4, y, None, r),
                     lambda: L.gm_points_decode_host(x, curve, 0, 0, 0, x, 4, y, None, r),
                     lambda: L.gm_points_encode(x, curve, 0, 0, x, 4, y, b)):
            assert call() == ERR_INVALID
            assert "unknown curve id" in L.gm_last_error().decode()


def test_empty_arrays_give_a_zero_report():
    import gnark_mi355x as gm
    L = gm.load_library()
    x = ctypes.c_void_p(0x1000)
    for call in (lambda r: L.gm_points_decode(x, 2, 1, 0, 0, None, 0, None, None, r),
                 lambda r: L.gm_points_decode(x, 0, 0, 1, 0x100, x, 0, x, x, r),
                 lambda r: L.gm_points_decode_host(x, 1, 0, 0, 0, None, 0, None, None, r)):
        rep = gm._PointsDecodeReport()
        ctypes.memset(ctypes.byref(rep), 0xEE, ctypes.sizeof(rep))
        assert call(ctypes.byref(rep)) == OK
        assert rep.as_dict() == dict(n=0, infinities=0, not_reduced=0, off_curve=0, off_subgroup=0, bad_encoding=0,
                                     no_root=0, first_bad=0, first_class=0)
    bad = ctypes.c_uint64(77)
    assert L.gm_points_encode(x, 1, 1, 1, None, 0, None, ctypes.byref(bad)) == OK and bad.value == 0
