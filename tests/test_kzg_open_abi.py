"""The KZG opening entries at the C boundary, without a GPU: the header declares
them, the built library exports them, the Python binding lists them, and each
refuses a NULL context before it touches a device."""
import ctypes
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "gnark_mi355x.h")
LIB = os.path.join(ROOT, "gnark-icicle_amd", "libgnark_mi355x.so")
ENTRIES = ("gm_kzg_eval", "gm_poly_div_linear", "gm_poly_fold", "gm_kzg_open", "gm_kzg_batch_open")
GM_ERR_INVALID = -1


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB):
        subprocess.check_call(["make", "-s", "-j8", "-C", os.path.join(ROOT, "gnark-icicle_amd")])
    return ctypes.CDLL(LIB)


def test_header_declares_the_opening_entries():
    src = open(HEADER).read()
    declared = set(re.findall(r"^int (gm_[a-z0-9_]+)\(", src, re.M))
    assert set(ENTRIES) <= declared
    m = re.search(r"GM_ERR_INVALID\s*=\s*(-?\d+)", src)
    assert m and int(m.group(1)) == GM_ERR_INVALID


def test_library_exports_the_opening_entries(lib):
    assert not [n for n in ENTRIES if not hasattr(lib, n)]


def test_binding_lists_the_opening_entries():
    import gnark_mi355x as gm
    assert set(ENTRIES) <= set(gm.SYMBOLS)
    for name in ("kzg_eval", "poly_div_linear", "poly_fold", "kzg_open", "kzg_batch_open"):
        assert callable(getattr(gm.Context, name))


def test_null_context_is_refused_without_a_device():
    """Run in a child with every GPU hidden: the NULL-context check comes before
    any HIP call, so the entries return GM_ERR_INVALID there too."""
    import sys
    code = r"""
import ctypes, sys
L = ctypes.CDLL(sys.argv[1])
vp, sz, i = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int
pvp, psz = ctypes.POINTER(vp), ctypes.POINTER(sz)
L.gm_kzg_eval.argtypes = [vp, i, pvp, psz, sz, vp, vp]
L.gm_poly_div_linear.argtypes = [vp, i, vp, sz, vp, vp, vp]
L.gm_poly_fold.argtypes = [vp, i, pvp, psz, sz, vp, vp]
L.gm_kzg_open.argtypes = [vp, i, vp, sz, vp, sz, vp, vp, vp]
L.gm_kzg_batch_open.argtypes = [vp, i, vp, sz, pvp, psz, sz, vp, vp, vp, vp]
z = (ctypes.c_uint8 * 32)()
out = (ctypes.c_uint8 * 96)()
ptrs = (vp * 1)(None)
lens = (sz * 1)(0)
for curve in (0, 1):
    print(L.gm_kzg_eval(None, curve, ptrs, lens, 1, z, out))
    print(L.gm_poly_div_linear(None, curve, None, 1, z, None, out))
    print(L.gm_poly_fold(None, curve, ptrs, lens, 1, z, None))
    print(L.gm_kzg_open(None, curve, None, 4, None, 1, z, out, out))
    print(L.gm_kzg_batch_open(None, curve, None, 4, ptrs, lens, 1, z, z, out, out))
"""
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")
    out = subprocess.run([sys.executable, "-c", code, LIB], env=env, capture_output=True, text=True, check=True)
    assert out.stdout.split() == [str(GM_ERR_INVALID)] * 10
