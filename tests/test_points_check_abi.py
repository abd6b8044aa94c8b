"""The point-check entries without a GPU: the generated constants, the closing
identities of the subgroup tests, the entries through header, library, binding
and Makefile, and every refusal that needs no device."""
import ctypes
import os
import subprocess
import sys

import pytest

import points_check_cases as pc
from points_check_cases import sub

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "gnark_mi355x.h")
NAMES = ("gm_points_check", "gm_points_check_host", "gm_set_points_check_chunk", "gm_g16_pk_check",
         "gm_g16_pk_check_dump")
OK, ERR_INVALID, ERR_UNSUPPORTED = 0, -1, -4


def test_generated_header_is_what_the_tool_prints():
    text = open(sub.HEADER).read()
    assert text == sub.header()
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "subgroup_constants.py"), "--print"],
                         capture_output=True, text=True, check=True).stdout
    assert out == text
    assert open(sub.HEADER).read() == text          # --print writes nothing


@pytest.mark.parametrize("cname", pc.CURVE_NAMES)
def test_closing_identities(cname):
    """derive() asserts them; they are restated here on its results."""
    import math
    d = pc.derived(cname)
    c = d["c"]
    p, r, u, t, h1, h2 = c.p, c.r, d["u"], d["t"], d["h1"], d["h2"]
    assert p + 1 - t == h1 * r
    k = d["g2_scalar"]
    assert k == t - 1 and (k - p) % r == 0 and k * k - t * k + p == h1 * r
    if d["bn"]:
        assert h1 == 1 and k == 6 * u * u
    else:
        lam = d["lam"]
        assert lam == u * u - 1 and lam * lam + lam + 1 == r
        assert (d["beta"] ** 2 + d["beta"] + 1) % p == 0
        assert h1 == (u - 1) ** 2 // 3 and math.gcd(h1, h2) == 1
    assert (cname == "bls12381") == (u < 0)
    # #E'(Fp2) = h2 r, on twist points that are not in the subgroup
    import pyref
    G2 = pyref.Group(c, True)
    for Q in sub.random_curve_points(c, True, 2, 0xAB1):
        assert G2.mul(Q, r) is not None and G2.mul(Q, h2 * r) is None
    # the counted work per point
    assert sub.op_counts(d, False) == ((0, 0) if d["bn"] else (126, 2 * (bin(abs(u)).count("1") - 1) + 1))
    assert sub.op_counts(d, True)[0] == (126 if d["bn"] else 63)


@pytest.mark.parametrize("cname,g2", pc.GROUPS)
def test_endomorphism_equations_equal_the_definition(cname, g2):
    """The equation each device test evaluates, in Python integers with the tool's
    constants, against [r]P = infinity on every on-curve case: subgroup points,
    random curve points, cofactor points and every small-order point."""
    c = pc.params(cname)
    seen = set()
    for name, raw, _ in pc.cases(cname, g2):
        cls, inf = pc.classify(cname, g2, raw)
        if inf or cls in (pc.NOT_REDUCED, pc.OFF_CURVE):
            continue
        assert pc.endomorphism_test(cname, g2, pc.decode(c, g2, raw)) == (cls == pc.OK), name
        seen.add(cls)
    assert seen == ({pc.OK} if (cname, g2) == ("bn254", False) else {pc.OK, pc.OFF_SUBGROUP})


def test_oracle_group_law_handles_the_exceptional_cases():
    """pyref's add and double on P + (-P), infinity + P and a point with y = 0 (the
    order-2 point of BLS12-377 G1): the oracle of the GPU tests relies on them."""
    import pyref
    for cname, g2 in pc.GROUPS:
        assert pc.group_law_handles_exceptions(pc.params(cname), g2)
    c = pc.params("bls12377")
    T = (c.p - 1, 0)                                  # (-1)^3 + 1 = 0
    G = pyref.Group(c, False)
    assert G.on_curve(T) and pc.group_law_handles_exceptions(c, False, T)
    # the suite's order-2 case is one of the three points with y = 0 (x^3 = -1)
    two = [raw for name, raw, _ in pc.cases("bls12377", False) if name == "order 2"]
    assert len(two) == 1 and two[0][1] == 0 and two[0][0] != 0


def test_square_roots():
    import random
    rng = random.Random(5)
    for cname in pc.CURVE_NAMES:
        c = pc.params(cname)
        import pyref
        F = pyref.F2(c)
        for _ in range(5):
            a = rng.randrange(c.p)
            assert sub.sqrt_fp(a * a % c.p, c.p) in (a, c.p - a)
            z = (rng.randrange(c.p), rng.randrange(c.p))
            s = sub.sqrt_fp2(F.mul(z, z), c)
            assert s in (z, F.neg(z))
            s = sub.sqrt_fp2((a * a % c.p, 0), c)
            assert F.mul(s, s) == (a * a % c.p, 0)


def test_header_library_binding_and_makefile_have_the_entries():
    import gnark_mi355x as gm
    src = open(HEADER).read()
    lo, hi = src.index("---- point validation"), src.index("---- staged prover inputs")
    for name in NAMES:
        assert lo < src.index("int %s(" % name) < hi
    assert "GM_POINT_OK = 0, GM_POINT_NOT_REDUCED = 1, GM_POINT_OFF_CURVE = 2, GM_POINT_OFF_SUBGROUP = 3" in src
    assert "} gm_points_report;" in src and "} gm_g16_pk_report;" in src
    L = gm.load_library()
    for name in NAMES:
        assert name in gm.SYMBOLS and hasattr(L, name), name
    for method in ("points_check", "points_check_host", "set_points_check_chunk", "g16_pk_check", "g16_pk_check_dump"):
        assert callable(getattr(gm.Context, method))
    assert (gm.POINT_OK, gm.POINT_NOT_REDUCED, gm.POINT_OFF_CURVE, gm.POINT_OFF_SUBGROUP) == (0, 1, 2, 3)
    assert ctypes.sizeof(gm._PointsReport) == 56 and ctypes.sizeof(gm._G16PkReport) == 568
    assert len(gm.G16_PK_MEMBERS) == 10
    mk = open(os.path.join(ROOT, "gnark-icicle_amd", "Makefile")).read()
    srcs = mk[mk.index("SRCS :="):mk.index("OBJS :=")]
    for unit in ("points_check", "points_check_bn254", "points_check_bls12377", "points_check_bls12381"):
        assert "csrc/%s.hip" % unit in srcs
        assert os.path.exists(os.path.join(ROOT, "gnark-icicle_amd", "csrc", unit + ".hip"))


def _pk_host(gm, **kw):
    h = gm._PkHost()
    h.domain_size, h.nbA, h.nbB, h.nbK = 8, 3, 2, 4
    for k in ("g1_alpha", "g1_beta", "g1_delta", "g1_A", "g1_B", "g1_Z", "g1_K", "g2_beta", "g2_delta", "g2_B"):
        setattr(h, k, 0x1000)
    for k, v in kw.items():
        setattr(h, k, v)
    return h


def test_refusals_before_any_device_call(tmp_path):
    """No context exists in this process and `x` is never dereferenced: a call that
    got past its refusal would fail with another code or not return at all."""
    import gnark_mi355x as gm
    L = gm.load_library()
    x = ctypes.c_void_p(0x1000)
    rep, krep, end = gm._PointsReport(), gm._G16PkReport(), ctypes.c_uint64()
    r, kr = ctypes.byref(rep), ctypes.byref(krep)
    h = ctypes.byref(_pk_host(gm))
    fd = os.open(str(tmp_path / "empty"), os.O_RDWR | os.O_CREAT)
    closed = os.open(str(tmp_path / "closed"), os.O_RDWR | os.O_CREAT)
    os.close(closed)
    null = "null"
    cases = [
        ("gm_points_check", null, lambda: L.gm_points_check(None, 0, 0, x, 4, None, r)),
        ("gm_points_check", null, lambda: L.gm_points_check(x, 0, 0, None, 4, None, r)),
        ("gm_points_check", null, lambda: L.gm_points_check(x, 0, 0, x, 4, None, None)),
        ("gm_points_check", "g2", lambda: L.gm_points_check(x, 0, 2, x, 4, None, r)),
        ("gm_points_check", "g2", lambda: L.gm_points_check(x, 1, -1, x, 4, None, r)),
        ("gm_points_check", "aligned", lambda: L.gm_points_check(x, 2, 1, ctypes.c_void_p(0x1008), 4, None, r)),
        ("gm_points_check_host", null, lambda: L.gm_points_check_host(None, 0, 0, x, 4, r)),
        ("gm_points_check_host", null, lambda: L.gm_points_check_host(x, 0, 0, None, 4, r)),
        ("gm_points_check_host", null, lambda: L.gm_points_check_host(x, 0, 0, x, 4, None)),
        ("gm_points_check_host", "g2", lambda: L.gm_points_check_host(x, 2, 2, x, 4, r)),
        ("gm_points_check_host", "address space", lambda: L.gm_points_check_host(x, 1, 1, x, 1 << 62, r)),
        ("gm_set_points_check_chunk", null, lambda: L.gm_set_points_check_chunk(None, 0)),
        ("gm_set_points_check_chunk", "64 MiB", lambda: L.gm_set_points_check_chunk(x, (64 << 20) + 1)),
        ("gm_g16_pk_check", null, lambda: L.gm_g16_pk_check(None, 0, h, kr)),
        ("gm_g16_pk_check", null, lambda: L.gm_g16_pk_check(x, 0, None, kr)),
        ("gm_g16_pk_check", null, lambda: L.gm_g16_pk_check(x, 0, h, None)),
        ("gm_g16_pk_check", "domain_size", lambda: L.gm_g16_pk_check(x, 0, ctypes.byref(_pk_host(gm, domain_size=1)), kr)),
        ("gm_g16_pk_check", "NULL", lambda: L.gm_g16_pk_check(x, 2, ctypes.byref(_pk_host(gm, g2_B=None)), kr)),
        ("gm_g16_pk_check", "NULL", lambda: L.gm_g16_pk_check(x, 1, ctypes.byref(_pk_host(gm, g1_alpha=None)), kr)),
        ("gm_g16_pk_check_dump", null, lambda: L.gm_g16_pk_check_dump(None, 0, h, fd, 0, kr, None)),
        ("gm_g16_pk_check_dump", null, lambda: L.gm_g16_pk_check_dump(x, 0, None, fd, 0, kr, None)),
        ("gm_g16_pk_check_dump", null, lambda: L.gm_g16_pk_check_dump(x, 0, h, fd, 0, None, None)),
        ("gm_g16_pk_check_dump", "file descriptor", lambda: L.gm_g16_pk_check_dump(x, 0, h, -1, 0, kr, None)),
        ("pk dump", "pread", lambda: L.gm_g16_pk_check_dump(x, 1, h, closed, 0, kr, ctypes.byref(end))),
        ("pk dump", "end of file", lambda: L.gm_g16_pk_check_dump(x, 0, h, fd, 0, kr, ctypes.byref(end))),
    ]
    try:
        for k, (entry, word, call) in enumerate(cases):
            assert call() == ERR_INVALID, (k, entry)
            msg = L.gm_last_error().decode()
            assert entry in msg and word.lower() in msg.lower(), (k, entry, msg)
        # a dump whose first slice length disagrees with meta is refused by its length
        os.write(fd, (7).to_bytes(8, "little") + bytes(64 * 7))
        assert L.gm_g16_pk_check_dump(x, 0, h, fd, 0, kr, None) == ERR_INVALID
        assert "slice 0 holds 7 points, expected 3" in L.gm_last_error().decode()
    finally:
        os.close(fd)


def test_empty_arrays_give_a_zero_report():
    import gnark_mi355x as gm
    L = gm.load_library()
    x = ctypes.c_void_p(0x1000)
    for call in (lambda r: L.gm_points_check(x, 2, 1, None, 0, None, r),
                 lambda r: L.gm_points_check(x, 0, 0, x, 0, x, r),
                 lambda r: L.gm_points_check_host(x, 1, 0, None, 0, r)):
        rep = gm._PointsReport()
        ctypes.memset(ctypes.byref(rep), 0xEE, ctypes.sizeof(rep))
        assert call(ctypes.byref(rep)) == OK
        assert rep.as_dict() == dict(n=0, infinities=0, not_reduced=0, off_curve=0, off_subgroup=0, first_bad=0,
                                     first_class=0)


def test_curve_ids():
    import gnark_mi355x as gm
    L = gm.load_library()
    x = ctypes.c_void_p(0x1000)
    rep, krep = gm._PointsReport(), gm._G16PkReport()
    r, kr = ctypes.byref(rep), ctypes.byref(krep)
    h = ctypes.byref(_pk_host(gm))
    for curve in (3, -1, 7):
        for call in (lambda: L.gm_points_check(x, curve, 0, x, 4, None, r),
                     lambda: L.gm_points_check_host(x, curve, 0, x, 4, r),
                     lambda: L.gm_g16_pk_check(x, curve, h, kr),
                     lambda: L.gm_g16_pk_check_dump(x, curve, h, 0, 0, kr, None)):
            assert call() == ERR_INVALID
            assert "unknown curve id" in L.gm_last_error().decode()
    assert L.gm_g16_pk_check_dump(x, 2, h, 0, 0, kr, None) == ERR_UNSUPPORTED
    msg = L.gm_last_error().decode()
    assert "gm_g16_pk_check_dump" in msg and "BLS12-381" in msg, msg
