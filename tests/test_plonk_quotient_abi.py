"""The PLONK quotient entry at the C boundary, without a GPU: the header declares
the entry and its input struct, the built library exports it, the Python binding
lists it and mirrors the struct, and a NULL context or a NULL struct is refused
before any device is touched."""
import ctypes
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "gnark_mi355x.h")
LIB = os.path.join(ROOT, "gnark-icicle_amd", "libgnark_mi355x.so")
ENTRY = "gm_plonk_quotient"
GM_ERR_INVALID = -1
# the struct's members in declaration order
FIELDS = ["n", "ql", "qr", "qm", "qo", "qk", "s1", "s2", "s3", "l", "r", "o", "z", "nb_bsb", "qcp", "pi2",
          "bl", "br", "bo", "bz", "alpha", "beta", "gamma"]


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB):
        subprocess.check_call(["make", "-s", "-j8", "-C", os.path.join(ROOT, "gnark-icicle_amd")])
    return ctypes.CDLL(LIB)


def test_header_declares_the_entry_and_the_struct():
    src = open(HEADER).read()
    assert re.search(r"^int gm_plonk_quotient\(gm_ctx\* ctx, int curve, const gm_plonk_quotient_in\* in, "
                     r"void\* h_dev\);", src, re.M)
    m = re.search(r"typedef struct \{(.*?)\} gm_plonk_quotient_in;", src, re.S)
    assert m
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    names = []
    for decl in body.split(";"):
        names += re.findall(r"\*?\s*([a-z0-9_]+)\s*(?:,|$)", decl.strip())
    assert names == FIELDS
    m = re.search(r"GM_ERR_INVALID\s*=\s*(-?\d+)", src)
    assert m and int(m.group(1)) == GM_ERR_INVALID


def test_library_exports_the_entry(lib):
    assert hasattr(lib, ENTRY)


def test_binding_lists_the_entry_and_mirrors_the_struct():
    import gnark_mi355x as gm
    assert ENTRY in gm.SYMBOLS
    assert callable(gm.Context.plonk_quotient)
    assert [f[0] for f in gm._PlonkQuotientIn._fields_] == FIELDS
    # every member is one machine word: no padding to get wrong
    assert ctypes.sizeof(gm._PlonkQuotientIn) == len(FIELDS) * ctypes.sizeof(ctypes.c_void_p)


def test_null_context_and_null_struct_are_refused_without_a_device():
    """Run in a child with every GPU hidden: both checks come before any HIP
    call, so the entry returns GM_ERR_INVALID there too."""
    import sys
    code = r"""
import ctypes, sys
L = ctypes.CDLL(sys.argv[1])
vp, i = ctypes.c_void_p, ctypes.c_int
L.gm_plonk_quotient.argtypes = [vp, i, vp, vp]
arg = (ctypes.c_size_t * 23)()
out = (ctypes.c_uint8 * 64)()
fake_ctx = (ctypes.c_uint8 * 64)()
for curve in (0, 1):
    print(L.gm_plonk_quotient(None, curve, ctypes.addressof(arg), ctypes.addressof(out)))
    print(L.gm_plonk_quotient(None, curve, None, ctypes.addressof(out)))
    # a NULL struct is refused before the context is looked at
    print(L.gm_plonk_quotient(ctypes.addressof(fake_ctx), curve, None, ctypes.addressof(out)))
"""
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")
    out = subprocess.run([sys.executable, "-c", code, LIB], env=env, capture_output=True, text=True, check=True)
    assert out.stdout.split() == [str(GM_ERR_INVALID)] * 6
