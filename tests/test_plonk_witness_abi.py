"""The resident wire tables, the gather stage, round 1 from the witness and the
sparse BSB22 input at the C boundary, without a GPU: the header declares the
entries and the struct, the built library exports them, the Python binding lists
them and mirrors the struct, and a NULL context, tables, session, input struct or
out is refused, with a message, before any device is touched."""
import ctypes
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "gnark_mi355x.h")
LIB = os.path.join(ROOT, "gnark-icicle_amd", "libgnark_mi355x.so")
MAKEFILE = os.path.join(ROOT, "gnark-icicle_amd", "Makefile")
ENTRIES = ["gm_plonk_wires_upload", "gm_plonk_wires_bytes", "gm_plonk_wires_free", "gm_plonk_gather_lro",
           "gm_plonk_session_round1_witness", "gm_plonk_session_bsb22_sparse"]
GM_ERR_INVALID = -1
# the struct's members in declaration order
WITNESS_FIELDS = ["witness", "commitment_vals", "bl", "br", "bo", "bz", "h_rand"]


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


def test_header_declares_the_entries_and_the_struct():
    src = open(HEADER).read()
    for name in ENTRIES:
        assert re.search(r"^int %s\(" % name, src, re.M), name
    assert re.search(r"^typedef struct gm_plonk_wires gm_plonk_wires;$", src, re.M)
    assert _members(src, "gm_plonk_round1_witness_in") == WITNESS_FIELDS
    # inside the PLONK session block: after the session's own entries, before the NTT
    assert src.index("int gm_plonk_session_free(") < src.index("int gm_plonk_wires_upload(") < \
        src.index("int gm_plonk_gather_lro(") < src.index("int gm_plonk_session_round1_witness(") < \
        src.index("int gm_plonk_session_bsb22_sparse(") < src.index("int gm_ntt(")


def test_library_exports_the_entries(lib):
    assert not [n for n in ENTRIES if not hasattr(lib, n)]


def test_makefile_builds_the_unit():
    srcs = re.search(r"^SRCS := (.*?)\n\S", open(MAKEFILE).read(), re.S | re.M).group(1)
    assert "csrc/plonk_wires.hip" in srcs.split()


def test_binding_lists_the_entries_and_mirrors_the_struct():
    import gnark_mi355x as gm
    assert set(ENTRIES) <= set(gm.SYMBOLS)
    assert [f[0] for f in gm._PlonkRound1WitnessIn._fields_] == WITNESS_FIELDS
    # every member is one machine word: no padding to get wrong
    assert ctypes.sizeof(gm._PlonkRound1WitnessIn) == len(WITNESS_FIELDS) * ctypes.sizeof(ctypes.c_void_p)
    for name in ("gather", "resident_bytes", "free"):
        assert callable(getattr(gm.PlonkWires, name)), name
    assert callable(gm.PlonkSession.round1_witness) and callable(gm.PlonkSession.bsb22_sparse)


def _child(code):
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")
    return subprocess.run([sys.executable, "-c", code, LIB], env=env, capture_output=True, text=True, check=True)


def test_null_handles_are_refused_without_a_device():
    """Run in a child with every GPU hidden: the checks come before any HIP call,
    so every entry returns GM_ERR_INVALID there too, each with its own message."""
    code = r"""
import ctypes, sys
L = ctypes.CDLL(sys.argv[1])
vp, sz = ctypes.c_void_p, ctypes.c_size_t
L.gm_last_error.restype = ctypes.c_char_p
L.gm_plonk_wires_upload.argtypes = [vp, sz, sz, vp, vp, vp, vp]
L.gm_plonk_wires_bytes.argtypes = [vp, vp]
L.gm_plonk_wires_free.argtypes = [vp, vp]
L.gm_plonk_gather_lro.argtypes = [vp, vp, vp, vp, vp, vp]
L.gm_plonk_session_round1_witness.argtypes = [vp, vp, vp, vp]
L.gm_plonk_session_bsb22_sparse.argtypes = [vp, sz, vp, vp, sz, vp]
arg = (ctypes.c_uint32 * 64)()
out = (ctypes.c_size_t * 64)()
fake = (ctypes.c_uint8 * 4096)()
A, O, X = ctypes.addressof(arg), ctypes.addressof(out), ctypes.addressof(fake)
def show(rc):
    print(rc, L.gm_last_error().decode().replace(" ", "_"))
show(L.gm_plonk_wires_upload(None, 8, 8, A, A, A, O))
show(L.gm_plonk_wires_upload(X, 8, 8, None, A, A, O))
show(L.gm_plonk_wires_upload(X, 8, 8, A, None, A, O))
show(L.gm_plonk_wires_upload(X, 8, 8, A, A, None, O))
show(L.gm_plonk_wires_upload(X, 8, 8, A, A, A, None))
show(L.gm_plonk_wires_bytes(None, O))
show(L.gm_plonk_wires_bytes(X, None))
show(L.gm_plonk_wires_free(None, X))
show(L.gm_plonk_wires_free(X, None))
show(L.gm_plonk_gather_lro(None, X, A, O, O, O))
show(L.gm_plonk_gather_lro(X, None, A, O, O, O))
show(L.gm_plonk_gather_lro(X, X, None, O, O, O))
show(L.gm_plonk_gather_lro(X, X, A, None, O, O))
show(L.gm_plonk_gather_lro(X, X, A, O, None, O))
show(L.gm_plonk_gather_lro(X, X, A, O, O, None))
show(L.gm_plonk_session_round1_witness(None, X, A, O))
show(L.gm_plonk_session_round1_witness(X, None, A, O))
show(L.gm_plonk_session_round1_witness(X, X, None, O))
show(L.gm_plonk_session_bsb22_sparse(None, 0, A, A, 1, O))
"""
    lines = [ln.split() for ln in _child(code).stdout.splitlines()]
    assert len(lines) == 19
    assert [ln[0] for ln in lines] == [str(GM_ERR_INVALID)] * 19
    want = ["plonk_wires_upload"] * 5 + ["plonk_wires_bytes"] * 2 + ["plonk_wires_free"] * 2 + \
        ["plonk_gather_lro"] * 6 + ["plonk_session_round_1_from_the_witness"] * 3 + ["plonk_session_bsb22_sparse"]
    for ln, w in zip(lines, want):
        assert ln[1].startswith(w), (ln, w)


def test_upload_checks_its_arguments_on_the_host():
    """n, nb_wires and every id are judged before any device call, on a fake
    context with every GPU hidden; the message names the table and the row."""
    code = r"""
import ctypes, sys
L = ctypes.CDLL(sys.argv[1])
vp, sz = ctypes.c_void_p, ctypes.c_size_t
L.gm_last_error.restype = ctypes.c_char_p
L.gm_plonk_wires_upload.argtypes = [vp, sz, sz, vp, vp, vp, vp]
ok = (ctypes.c_uint32 * 16)(*range(16))
bad = (ctypes.c_uint32 * 16)(*range(16))
bad[11] = 16
top = (ctypes.c_uint32 * 16)(*([0xffffffff] * 16))
out = (ctypes.c_size_t * 4)()
fake = (ctypes.c_uint8 * 4096)()
K, B, T, O, X = (ctypes.addressof(v) for v in (ok, bad, top, out, fake))
def show(rc):
    print(rc, L.gm_last_error().decode().replace(" ", "_"))
show(L.gm_plonk_wires_upload(X, 12, 16, K, K, K, O))
show(L.gm_plonk_wires_upload(X, 4, 16, K, K, K, O))
show(L.gm_plonk_wires_upload(X, 0, 16, K, K, K, O))
show(L.gm_plonk_wires_upload(X, 16, 0, K, K, K, O))
show(L.gm_plonk_wires_upload(X, 16, 1 << 32, K, K, K, O))
show(L.gm_plonk_wires_upload(X, 16, 15, K, K, K, O))
show(L.gm_plonk_wires_upload(X, 16, 16, K, B, K, O))
show(L.gm_plonk_wires_upload(X, 16, 16, K, K, B, O))
show(L.gm_plonk_wires_upload(X, 16, (1 << 32) - 1, T, K, K, O))
print(out[0])
"""
    lines = _child(code).stdout.splitlines()
    assert [ln.split()[0] for ln in lines[:9]] == [str(GM_ERR_INVALID)] * 9
    msgs = [ln.split()[1] for ln in lines[:9]]
    assert all(m.startswith("plonk_wires:") for m in msgs)
    assert all("power_of_two" in m for m in msgs[:3])
    assert "nb_wires" in msgs[3] and "nb_wires" in msgs[4]
    assert "xa[15]_=_15" in msgs[5]
    assert "xb[11]_=_16" in msgs[6]
    assert "xc[11]_=_16" in msgs[7]
    assert "xa[0]_=_4294967295" in msgs[8]
    assert lines[9] == "0"  # out was never written


def test_a_null_input_struct_or_null_tables_are_refused_before_the_session_is_read():
    """The session pointer is not dereferenced when `in` or the tables are NULL: a
    fake session does not crash the child."""
    code = r"""
import ctypes, sys
L = ctypes.CDLL(sys.argv[1])
L.gm_plonk_session_round1_witness.argtypes = [ctypes.c_void_p] * 4
fake = (ctypes.c_uint8 * 4096)(*([0xff] * 4096))
out = (ctypes.c_size_t * 64)()
X, O = ctypes.addressof(fake), ctypes.addressof(out)
print(L.gm_plonk_session_round1_witness(X, X, None, O))
print(L.gm_plonk_session_round1_witness(X, None, X, O))
"""
    assert _child(code).stdout.split() == [str(GM_ERR_INVALID)] * 2
