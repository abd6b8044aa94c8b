"""The resident PLONK key and the prover session at the C boundary, without a GPU:
the header declares the entries and both structs, the built library exports them,
the Python binding lists them and mirrors the structs, and a NULL context, key,
session, input struct or out is refused, with a message, before any device is
touched."""
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
ENTRIES = ["gm_plonk_pk_upload", "gm_plonk_pk_bytes", "gm_plonk_pk_free", "gm_plonk_session_begin",
           "gm_plonk_session_bsb22", "gm_plonk_session_round1", "gm_plonk_session_round2",
           "gm_plonk_session_round3", "gm_plonk_session_round4", "gm_plonk_session_round5",
           "gm_plonk_session_free"]
GM_ERR_INVALID = -1
# the structs' members in declaration order
PK_FIELDS = ["n", "nb_public", "ql", "qr", "qm", "qo", "qk", "s1", "s2", "s3", "nb_bsb", "qcp", "commitment_row",
             "srs_canonical", "srs_canonical_len", "srs_lagrange"]
ROUND1_FIELDS = ["l", "r", "o", "public_inputs", "commitment_vals", "bl", "br", "bo", "bz", "h_rand"]


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


def test_header_declares_the_entries_and_both_structs():
    src = open(HEADER).read()
    for name in ENTRIES:
        assert re.search(r"^int %s\(" % name, src, re.M), name
    assert _members(src, "gm_plonk_pk_host") == PK_FIELDS
    assert _members(src, "gm_plonk_round1_in") == ROUND1_FIELDS
    assert re.search(r"^#define GM_PLONK_PK_NO_COSET_CACHE 1u$", src, re.M)
    # declared after the stages they drive
    assert src.index("int gm_plonk_linearize(") < src.index("int gm_plonk_pk_upload(") < \
        src.index("int gm_plonk_session_begin(") < src.index("int gm_ntt(")


def test_library_exports_the_entries(lib):
    assert not [n for n in ENTRIES if not hasattr(lib, n)]


def test_makefile_builds_the_two_units():
    srcs = re.search(r"^SRCS := (.*?)\n\S", open(MAKEFILE).read(), re.S | re.M).group(1)
    assert "csrc/plonk_pk.hip" in srcs and "csrc/plonk_session.hip" in srcs


def test_binding_lists_the_entries_and_mirrors_the_structs():
    import gnark_mi355x as gm
    assert set(ENTRIES) <= set(gm.SYMBOLS)
    assert [f[0] for f in gm._PlonkPkHost._fields_] == PK_FIELDS
    assert [f[0] for f in gm._PlonkRound1In._fields_] == ROUND1_FIELDS
    # every member is one machine word: no padding to get wrong
    word = ctypes.sizeof(ctypes.c_void_p)
    assert ctypes.sizeof(gm._PlonkPkHost) == len(PK_FIELDS) * word
    assert ctypes.sizeof(gm._PlonkRound1In) == len(ROUND1_FIELDS) * word
    assert gm.PLONK_PK_NO_COSET_CACHE == 1
    for name in ("bsb22", "round1", "round2", "round3", "round4", "round5", "free"):
        assert callable(getattr(gm.PlonkSession, name)), name
    assert callable(gm.PlonkProvingKey.session) and callable(gm.PlonkProvingKey.resident_bytes)


def test_null_handles_are_refused_without_a_device():
    """Run in a child with every GPU hidden: the checks come before any HIP call,
    so every entry returns GM_ERR_INVALID there too, each with its own message."""
    code = r"""
import ctypes, sys
L = ctypes.CDLL(sys.argv[1])
vp, i, sz, u = ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t, ctypes.c_uint
L.gm_last_error.restype = ctypes.c_char_p
L.gm_plonk_pk_upload.argtypes = [vp, i, vp, u, vp]
L.gm_plonk_pk_bytes.argtypes = [vp, vp, vp]
L.gm_plonk_pk_free.argtypes = [vp, vp]
L.gm_plonk_session_begin.argtypes = [vp, vp, vp]
L.gm_plonk_session_bsb22.argtypes = [vp, sz, vp, vp]
L.gm_plonk_session_round1.argtypes = [vp, vp, vp]
L.gm_plonk_session_round2.argtypes = [vp, vp, vp, vp]
L.gm_plonk_session_round3.argtypes = [vp, vp, vp]
L.gm_plonk_session_round4.argtypes = [vp, vp, vp, vp, vp, vp]
L.gm_plonk_session_round5.argtypes = [vp, vp, vp]
L.gm_plonk_session_free.argtypes = [vp]
arg = (ctypes.c_size_t * 16)()
out = (ctypes.c_size_t * 64)()
fake = (ctypes.c_uint8 * 4096)()
A, O, X = ctypes.addressof(arg), ctypes.addressof(out), ctypes.addressof(fake)
def show(rc):
    print(rc, L.gm_last_error().decode().replace(" ", "_"))
for curve in (0, 1):
    show(L.gm_plonk_pk_upload(None, curve, A, 0, O))
    show(L.gm_plonk_pk_upload(X, curve, None, 0, O))
    show(L.gm_plonk_pk_upload(X, curve, A, 0, None))
show(L.gm_plonk_pk_bytes(None, O, O))
show(L.gm_plonk_pk_free(None, X))
show(L.gm_plonk_pk_free(X, None))
show(L.gm_plonk_session_begin(None, X, O))
show(L.gm_plonk_session_begin(X, None, O))
show(L.gm_plonk_session_begin(X, X, None))
show(L.gm_plonk_session_bsb22(None, 0, A, O))
show(L.gm_plonk_session_round1(None, A, O))
show(L.gm_plonk_session_round2(None, A, A, O))
show(L.gm_plonk_session_round3(None, A, O))
show(L.gm_plonk_session_round4(None, A, O, O, O, O))
show(L.gm_plonk_session_round5(None, A, O))
show(L.gm_plonk_session_free(None))
"""
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")
    out = subprocess.run([sys.executable, "-c", code, LIB], env=env, capture_output=True, text=True, check=True)
    lines = [ln.split() for ln in out.stdout.splitlines()]
    assert len(lines) == 19
    assert [ln[0] for ln in lines] == [str(GM_ERR_INVALID)] * 19
    want = ["plonk_pk_upload"] * 6 + ["plonk_pk_bytes"] + ["plonk_pk_free"] * 2 + ["plonk_session_begin"] * 3 + \
        ["plonk_session_bsb22"] + ["plonk_session_round_%d" % k for k in range(1, 6)] + ["plonk_session_free"]
    for ln, w in zip(lines, want):
        assert ln[1].startswith(w), (ln, w)


def test_a_null_input_struct_of_round_1_is_refused_before_the_session_is_read():
    """The session pointer is not dereferenced when `in` is NULL: a fake session
    does not crash the child."""
    code = r"""
import ctypes, sys
L = ctypes.CDLL(sys.argv[1])
L.gm_plonk_session_round1.argtypes = [ctypes.c_void_p] * 3
fake = (ctypes.c_uint8 * 4096)()
out = (ctypes.c_size_t * 64)()
print(L.gm_plonk_session_round1(ctypes.addressof(fake), None, ctypes.addressof(out)))
"""
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")
    out = subprocess.run([sys.executable, "-c", code, LIB], env=env, capture_output=True, text=True, check=True)
    assert out.stdout.split() == [str(GM_ERR_INVALID)]
