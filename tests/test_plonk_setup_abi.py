"""The PLONK setup entries at the C boundary, without a GPU: the header declares the
three functions and the struct, the built library exports them, the Python
binding lists them and mirrors the struct's layout, and a NULL context, struct or
out -- and everything else the host can judge -- is refused with GM_ERR_INVALID
and a message before any device is touched."""
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
ENTRIES = ["gm_kzg_srs_lagrange", "gm_plonk_sigma", "gm_plonk_pk_setup"]
GM_ERR_INVALID = -1
# the struct's members in declaration order
SETUP_FIELDS = ["n", "nb_public", "ql", "qr", "qm", "qo", "qk", "permutation", "nb_bsb", "qcp", "commitment_row",
                "srs_canonical", "srs_canonical_len"]


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
    assert _members(src, "gm_plonk_setup_host") == SETUP_FIELDS
    assert re.search(r"const int64_t\* permutation;", src)
    # gm_plonk_pk_upload and its struct stay as they are, ahead of the new block
    assert src.index("} gm_plonk_pk_host;") < src.index("int gm_plonk_pk_upload(") < \
        src.index("int gm_kzg_srs_lagrange(") < src.index("int gm_plonk_sigma(") < \
        src.index("} gm_plonk_setup_host;") < src.index("int gm_plonk_pk_setup(") < src.index("int gm_ntt(")


def test_library_exports_the_entries(lib):
    assert not [n for n in ENTRIES if not hasattr(lib, n)]


def test_makefile_builds_the_unit():
    srcs = re.search(r"^SRCS := (.*?)\n\S", open(MAKEFILE).read(), re.S | re.M).group(1)
    assert "csrc/plonk_setup.hip" in srcs.split()


def test_binding_lists_the_entries_and_mirrors_the_struct():
    import gnark_mi355x as gm
    assert set(ENTRIES) <= set(gm.SYMBOLS)
    S = gm._PlonkSetupHost
    assert [f[0] for f in S._fields_] == SETUP_FIELDS
    # every member is one machine word, size_t or pointer: no padding to get wrong
    word = ctypes.sizeof(ctypes.c_void_p)
    assert ctypes.sizeof(ctypes.c_size_t) == word
    assert ctypes.sizeof(S) == len(SETUP_FIELDS) * word
    for k, name in enumerate(SETUP_FIELDS):
        assert getattr(S, name).offset == k * word and getattr(S, name).size == word, name
    kinds = dict(S._fields_)
    for name in ("n", "nb_public", "nb_bsb", "srs_canonical_len"):
        assert kinds[name] is ctypes.c_size_t, name
    assert kinds["permutation"] is ctypes.POINTER(ctypes.c_int64)
    assert kinds["commitment_row"] is ctypes.POINTER(ctypes.c_size_t)
    # gm_plonk_pk_host is gm_plonk_setup_host with s1, s2, s3 for the permutation and the Lagrange SRS behind
    host = [f[0] for f in gm._PlonkPkHost._fields_]
    assert [f for f in host if f not in ("s1", "s2", "s3", "srs_lagrange")] == \
        [f for f in SETUP_FIELDS if f != "permutation"]
    assert callable(gm.Context.kzg_srs_lagrange) and callable(gm.Context.plonk_sigma)
    assert callable(gm.PlonkProvingKey.setup)


def _child(code):
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")
    return subprocess.run([sys.executable, "-c", code, LIB], env=env, capture_output=True, text=True, check=True)


PRELUDE = r"""
import ctypes, sys
L = ctypes.CDLL(sys.argv[1])
vp, sz = ctypes.c_void_p, ctypes.c_size_t
L.gm_last_error.restype = ctypes.c_char_p
L.gm_kzg_srs_lagrange.argtypes = [vp, ctypes.c_int, vp, sz, vp]
L.gm_plonk_sigma.argtypes = [vp, ctypes.c_int, sz, vp, vp, vp, vp]
L.gm_plonk_pk_setup.argtypes = [vp, ctypes.c_int, vp, ctypes.c_uint, vp, vp, vp]
class Setup(ctypes.Structure):
    _fields_ = [("n", sz), ("nb_public", sz)] + [(k, vp) for k in ("ql", "qr", "qm", "qo", "qk", "permutation")] + \
        [("nb_bsb", sz), ("qcp", vp), ("commitment_row", vp), ("srs_canonical", vp), ("srs_canonical_len", sz)]
fake = (ctypes.c_uint8 * 8192)()
out = (ctypes.c_size_t * 64)()
X, O = ctypes.addressof(fake), ctypes.addressof(out)
def show(rc):
    print(rc, L.gm_last_error().decode().replace(" ", "_"))
"""


def test_null_handles_are_refused_without_a_device():
    """Run in a child with every GPU hidden: the checks come before any HIP call."""
    code = PRELUDE + r"""
s = Setup()
S = ctypes.addressof(s)
show(L.gm_kzg_srs_lagrange(None, 0, X, 8, X))
show(L.gm_kzg_srs_lagrange(X, 0, None, 8, X))
show(L.gm_kzg_srs_lagrange(X, 0, X, 8, None))
show(L.gm_plonk_sigma(None, 0, 8, X, X, X, X))
show(L.gm_plonk_sigma(X, 0, 8, None, X, X, X))
show(L.gm_plonk_sigma(X, 0, 8, X, None, X, X))
show(L.gm_plonk_sigma(X, 0, 8, X, X, None, X))
show(L.gm_plonk_sigma(X, 0, 8, X, X, X, None))
show(L.gm_plonk_pk_setup(None, 0, S, 0, O, X, None))
show(L.gm_plonk_pk_setup(X, 0, None, 0, O, X, None))
show(L.gm_plonk_pk_setup(X, 0, S, 0, None, X, None))
show(L.gm_plonk_pk_setup(X, 7, S, 0, O, X, None))
"""
    lines = [ln.split() for ln in _child(code).stdout.splitlines()]
    assert len(lines) == 12
    assert [ln[0] for ln in lines] == [str(GM_ERR_INVALID)] * 12
    want = ["kzg_srs_lagrange"] * 3 + ["plonk_sigma"] * 5 + ["plonk_pk_setup"] * 3 + ["unknown_curve"]
    for ln, w in zip(lines, want):
        assert ln[1].startswith(w), (ln, w)


def test_the_host_checks_come_before_any_device_call():
    """The overlap rule, the permutation's range (first offender named) and the
    key's refusals are judged on a fake context with every GPU hidden."""
    code = PRELUDE + r"""
# the Lagrange SRS: in place or disjoint (BN254 points are 64 bytes)
show(L.gm_kzg_srs_lagrange(X, 0, X, 8, X + 64))
show(L.gm_kzg_srs_lagrange(X, 0, X + 64 * 7, 8, X))
# sigma: n, then the entries
perm = (ctypes.c_int64 * 24)(*range(24))
P = ctypes.addressof(perm)
show(L.gm_plonk_sigma(X, 0, 12, P, X, X, X))
show(L.gm_plonk_sigma(X, 0, 0, P, X, X, X))
perm[13], perm[20] = -1, 99
show(L.gm_plonk_sigma(X, 0, 8, P, X, X, X))
perm[13] = 24
show(L.gm_plonk_sigma(X, 1, 8, P, X, X, X))
# the key
def key(**over):
    s = Setup()
    s.n, s.nb_public, s.nb_bsb, s.srs_canonical_len = 8, 2, 0, 11
    for k in ("ql", "qr", "qm", "qo", "qk", "srs_canonical"):
        setattr(s, k, X)
    s.permutation = P
    digests = over.pop("digests", X)
    flags = over.pop("flags", 0)
    for k, v in over.items():
        setattr(s, k, v)
    show(L.gm_plonk_pk_setup(X, 0, ctypes.addressof(s), flags, O, digests, None))
key(n=12)
key(n=4)
key(flags=2)
key(qm=None)
key(srs_canonical=None)
key(srs_canonical_len=10)
key(nb_public=9)
key(nb_bsb=1)
key(permutation=None)
key(digests=None)
key()
"""
    lines = [ln.split() for ln in _child(code).stdout.splitlines()]
    assert len(lines) == 17
    assert [ln[0] for ln in lines] == [str(GM_ERR_INVALID)] * 17
    want = ["kzg_srs_lagrange:_the_output_overlaps"] * 2 + ["plonk_sigma:_n_must_be"] * 2 + \
        ["plonk_setup:_permutation[13]_=_-1_", "plonk_setup:_permutation[13]_=_24_"] + \
        ["plonk_pk:_n_must_be"] * 2 + ["plonk_pk:_unknown_flag"] + ["plonk_pk:_the_polynomials"] * 2 + \
        ["plonk_pk:_the_canonical_SRS_needs", "plonk_pk:_more_public_inputs", "plonk_pk:_nb_bsb_>_0_needs"] + \
        ["plonk_setup:_the_permutation_and_vk_digests"] * 2 + ["plonk_setup:_permutation[13]_=_24_"]
    for ln, w in zip(lines, want):
        assert ln[1].startswith(w), (ln, w)
