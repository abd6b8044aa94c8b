"""The PLONK linearized-polynomial entry at the C boundary, without a GPU: the
header declares the entry and both structs, the built library exports it, the
Python binding lists it and mirrors the structs and the launch geometry, and a
NULL context, NULL input struct or NULL output struct is refused before any device
is touched."""
import ctypes
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "gnark_mi355x.h")
GEOMETRY = os.path.join(ROOT, "gnark-icicle_amd", "csrc", "plonk_lin.hpp")
LIB = os.path.join(ROOT, "gnark-icicle_amd", "libgnark_mi355x.so")
ENTRY = "gm_plonk_linearize"
GM_ERR_INVALID = -1
# the structs' members in declaration order
QUOTIENT_FIELDS = ["n", "ql", "qr", "qm", "qo", "qk", "s1", "s2", "s3", "l", "r", "o", "z", "nb_bsb", "qcp", "pi2",
                   "bl", "br", "bo", "bz", "alpha", "beta", "gamma"]
IN_FIELDS = QUOTIENT_FIELDS[:20] + ["h", "h_rand", "alpha", "beta", "gamma", "zeta"]
OUT_FIELDS = ["lin", "l_blinded", "r_blinded", "o_blinded", "z_blinded", "evals"]
PERM_FIELDS = ["n", "l", "r", "o", "s1", "s2", "s3", "beta", "gamma"]


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB):
        subprocess.check_call(["make", "-s", "-j8", "-C", os.path.join(ROOT, "gnark-icicle_amd")])
    return ctypes.CDLL(LIB)


def _members(src, name):
    m = re.search(r"typedef struct \{((?:(?!typedef).)*?)\} %s;" % name, src, re.S)
    assert m, name
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    names = []
    for decl in body.split(";"):
        names += re.findall(r"\*?\s*([a-z0-9_]+)\s*(?:,|$)", decl.strip())
    return names


def test_header_declares_the_entry_and_both_structs():
    src = open(HEADER).read()
    assert re.search(r"^int gm_plonk_linearize\(gm_ctx\* ctx, int curve, const gm_plonk_linearize_in\* in,\s*"
                     r"const gm_plonk_linearize_out\* out\);", src, re.M)
    assert _members(src, "gm_plonk_linearize_in") == IN_FIELDS
    assert _members(src, "gm_plonk_linearize_out") == OUT_FIELDS
    m = re.search(r"GM_ERR_INVALID\s*=\s*(-?\d+)", src)
    assert m and int(m.group(1)) == GM_ERR_INVALID
    # declared after the permutation entry
    assert src.index("int gm_plonk_perm_z(") < src.index("int gm_plonk_linearize(") < src.index("int gm_ntt(")


def test_the_quotient_and_perm_structs_are_as_they_were():
    src = open(HEADER).read()
    assert _members(src, "gm_plonk_quotient_in") == QUOTIENT_FIELDS
    assert _members(src, "gm_plonk_perm_in") == PERM_FIELDS
    assert ("  const void *bz;                  /* host, 3 Fr (degree 2) */\n"
            "  const void *alpha, *beta, *gamma;/* host, 1 Fr each */\n"
            "} gm_plonk_quotient_in;\n"
            "int gm_plonk_quotient(gm_ctx* ctx, int curve, const gm_plonk_quotient_in* in, void* h_dev);\n") in src
    assert ("  const void *beta, *gamma;    /* host, 1 Fr each */\n"
            "} gm_plonk_perm_in;\n"
            "int gm_plonk_perm_z(gm_ctx* ctx, int curve, const gm_plonk_perm_in* in,\n") in src


def test_library_exports_the_entry(lib):
    assert hasattr(lib, ENTRY)


def test_binding_lists_the_entry_and_mirrors_the_structs():
    import gnark_mi355x as gm
    assert ENTRY in gm.SYMBOLS
    assert callable(gm.Context.plonk_linearize)
    assert [f[0] for f in gm._PlonkLinearizeIn._fields_] == IN_FIELDS
    assert [f[0] for f in gm._PlonkLinearizeOut._fields_] == OUT_FIELDS
    # every member is one machine word: no padding to get wrong
    word = ctypes.sizeof(ctypes.c_void_p)
    assert ctypes.sizeof(gm._PlonkLinearizeIn) == len(IN_FIELDS) * word
    assert ctypes.sizeof(gm._PlonkLinearizeOut) == len(OUT_FIELDS) * word
    # the first twenty members are the quotient's, at the same offsets
    for name in IN_FIELDS[:20]:
        assert getattr(gm._PlonkLinearizeIn, name).offset == getattr(gm._PlonkQuotientIn, name).offset, name
    assert gm.PLONK_LIN_BLINDED == tuple(OUT_FIELDS[1:5])


def test_binding_mirrors_the_launch_geometry():
    """The GPU tests size their inputs by the block of the combination pass: the
    binding's constant is the kernel's, and the grid is not capped (no lane loops,
    so there is no second-iteration size to test)."""
    import gnark_mi355x as gm
    src = open(GEOMETRY).read()
    m = re.search(r"constexpr int LIN_TPB_LOG = (\d+);", src)
    assert m and re.search(r"constexpr int LIN_BLOCK = 1 << LIN_TPB_LOG;", src)
    assert gm.PLONK_LIN_BLOCK == 1 << int(m.group(1))
    assert "not capped" in src


def test_null_context_and_null_structs_are_refused_without_a_device():
    """Run in a child with every GPU hidden: the three checks come before any HIP
    call, so the entry returns GM_ERR_INVALID there too."""
    import sys
    code = r"""
import ctypes, sys
L = ctypes.CDLL(sys.argv[1])
vp, i = ctypes.c_void_p, ctypes.c_int
L.gm_plonk_linearize.argtypes = [vp, i, vp, vp]
arg = (ctypes.c_size_t * 26)()
out = (ctypes.c_size_t * 6)()
fake_ctx = (ctypes.c_uint8 * 64)()
A, O, X = ctypes.addressof(arg), ctypes.addressof(out), ctypes.addressof(fake_ctx)
for curve in (0, 1):
    print(L.gm_plonk_linearize(None, curve, A, O))
    print(L.gm_plonk_linearize(None, curve, None, O))
    print(L.gm_plonk_linearize(None, curve, A, None))
    # a NULL struct is refused before the context is looked at
    print(L.gm_plonk_linearize(X, curve, None, O))
    print(L.gm_plonk_linearize(X, curve, A, None))
"""
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")
    out = subprocess.run([sys.executable, "-c", code, LIB], env=env, capture_output=True, text=True, check=True)
    assert out.stdout.split() == [str(GM_ERR_INVALID)] * 10
