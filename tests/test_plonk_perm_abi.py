"""The PLONK permutation-polynomial entry at the C boundary, without a GPU: the
header declares the entry and its input struct, the built library exports it, the
Python binding lists it and mirrors the struct and the scan geometry, and a NULL
context or a NULL struct is refused before any device is touched."""
import ctypes
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "gnark_mi355x.h")
GEOMETRY = os.path.join(ROOT, "gnark-icicle_amd", "csrc", "plonk_perm.hpp")
LIB = os.path.join(ROOT, "gnark-icicle_amd", "libgnark_mi355x.so")
ENTRY = "gm_plonk_perm_z"
GM_ERR_INVALID = -1
# the struct's members in declaration order
FIELDS = ["n", "l", "r", "o", "s1", "s2", "s3", "beta", "gamma"]


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB):
        subprocess.check_call(["make", "-s", "-j8", "-C", os.path.join(ROOT, "gnark-icicle_amd")])
    return ctypes.CDLL(LIB)


def test_header_declares_the_entry_and_the_struct():
    src = open(HEADER).read()
    assert re.search(r"^int gm_plonk_perm_z\(gm_ctx\* ctx, int curve, const gm_plonk_perm_in\* in,\s*"
                     r"void\* z_lagrange_dev, void\* z_canonical_dev[^)]*\);", src, re.M)
    m = re.search(r"typedef struct \{((?:(?!typedef).)*?)\} gm_plonk_perm_in;", src, re.S)
    assert m
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    names = []
    for decl in body.split(";"):
        names += re.findall(r"\*?\s*([a-z0-9_]+)\s*(?:,|$)", decl.strip())
    assert names == FIELDS
    m = re.search(r"GM_ERR_INVALID\s*=\s*(-?\d+)", src)
    assert m and int(m.group(1)) == GM_ERR_INVALID
    # the existing quotient struct is as it was
    assert re.search(r"const void \*l, \*r, \*o, \*z;\s*/\* device, n Fr each, NOT blinded \*/", src)


def test_library_exports_the_entry(lib):
    assert hasattr(lib, ENTRY)


def test_binding_lists_the_entry_and_mirrors_the_struct():
    import gnark_mi355x as gm
    assert ENTRY in gm.SYMBOLS
    assert callable(gm.Context.plonk_perm_z)
    assert [f[0] for f in gm._PlonkPermIn._fields_] == FIELDS
    # every member is one machine word: no padding to get wrong
    assert ctypes.sizeof(gm._PlonkPermIn) == 9 * ctypes.sizeof(ctypes.c_void_p)


def test_binding_mirrors_the_scan_geometry():
    """The GPU tests place zero denominators by run and size their inputs by chunk
    and carry tile: the binding's constants are the kernels'."""
    import gnark_mi355x as gm
    src = open(GEOMETRY).read()
    log = {k: int(v) for k, v in re.findall(r"constexpr int PERM_([A-Z]+)_LOG = (\d+);", src)}
    assert set(log) == {"TPB", "E", "CT"}
    assert gm.PLONK_PERM_E == 1 << log["E"]
    assert gm.PLONK_PERM_CHUNK == 1 << (log["E"] + log["TPB"])
    assert gm.PLONK_PERM_CARRY_TILE == 1 << log["CT"]
    # one inversion serves at least 512 rows, and 2^17 rows span two carry tiles
    assert gm.PLONK_PERM_CHUNK >= 512
    assert 2 * gm.PLONK_PERM_CARRY_TILE * gm.PLONK_PERM_CHUNK <= 1 << 17


def test_null_context_and_null_struct_are_refused_without_a_device():
    """Run in a child with every GPU hidden: both checks come before any HIP
    call, so the entry returns GM_ERR_INVALID there too."""
    import sys
    code = r"""
import ctypes, sys
L = ctypes.CDLL(sys.argv[1])
vp, i = ctypes.c_void_p, ctypes.c_int
L.gm_plonk_perm_z.argtypes = [vp, i, vp, vp, vp]
arg = (ctypes.c_size_t * 9)()
out = (ctypes.c_uint8 * 64)()
fake_ctx = (ctypes.c_uint8 * 64)()
for curve in (0, 1):
    print(L.gm_plonk_perm_z(None, curve, ctypes.addressof(arg), ctypes.addressof(out), None))
    print(L.gm_plonk_perm_z(None, curve, None, ctypes.addressof(out), None))
    # a NULL struct is refused before the context is looked at
    print(L.gm_plonk_perm_z(ctypes.addressof(fake_ctx), curve, None, ctypes.addressof(out), None))
"""
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")
    out = subprocess.run([sys.executable, "-c", code, LIB], env=env, capture_output=True, text=True, check=True)
    assert out.stdout.split() == [str(GM_ERR_INVALID)] * 6
