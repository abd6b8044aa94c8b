"""The Groth16 setup entries at the C boundary, without a GPU: the header declares
the entries and the two structs, the built library exports them, the Python
binding lists them and mirrors the struct layouts word for word, the Makefile
builds the unit, and a NULL handle, an unknown curve, a window or cut out of range,
unknown flags or an empty constraint system is refused with GM_ERR_INVALID and a
message that names the entry before any device is touched."""
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
ENTRIES = ["gm_set_fixed_base_window", "gm_batch_mul_fixed", "gm_set_g16_setup_column_cut", "gm_g16_setup_sizes",
           "gm_g16_setup", "gm_g16_pk_setup"]
GM_ERR_INVALID = -1
# the structs' members in declaration order
IN_FIELDS = ["toxic", "nb_public", "gamma_wires", "nb_gamma"]
OUT_FIELDS = ["g1_alpha", "g1_beta", "g1_delta", "g1_A", "g1_B", "g1_Z", "g1_K", "g1_K_gamma", "g2_beta", "g2_delta",
              "g2_gamma", "g2_B", "infA", "infB", "k_wires"]


def _members(src, name):
    m = re.search(r"typedef struct \{((?:(?!typedef).)*?)\} %s;" % name, src, re.S)
    assert m, name
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    names = []
    for decl in body.split(";"):
        names += re.findall(r"\*?\s*([A-Za-z0-9_]+)\s*(?:,|$)", decl.strip())
    return names


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB):
        subprocess.check_call(["make", "-s", "-j8", "-C", os.path.join(ROOT, "gnark-icicle_amd")])
    return ctypes.CDLL(LIB)


def test_header_declares_the_entries():
    src = open(HEADER).read()
    for name in ENTRIES:
        assert re.search(r"^int %s\(" % name, src, re.M), name
    # the signature is gm_batch_mul_base's
    sig = lambda name: re.sub(r"\s+", " ", re.search(r"^int %s\((.*?)\);" % name, src, re.M | re.S).group(1))
    assert sig("gm_batch_mul_fixed").replace("out_dev", "points_out_dev") == sig("gm_batch_mul_base")
    assert sig("gm_set_fixed_base_window") == "gm_ctx* ctx, int c"
    assert _members(src, "gm_g16_setup_in") == IN_FIELDS
    assert _members(src, "gm_g16_setup_out") == OUT_FIELDS
    assert src.index("} gm_g16_setup_out;") < src.index("int gm_g16_setup_sizes(") < src.index("int gm_g16_setup(") < \
        src.index("int gm_g16_pk_setup(")
    # gm_batch_mul_base stays where it was, behind the new block
    assert src.index("int gm_jac_to_affine(") < src.index("int gm_set_fixed_base_window(") < \
        src.index("int gm_batch_mul_fixed(") < src.index("int gm_batch_mul_base(")


def test_library_exports_the_entries(lib):
    assert not [n for n in ENTRIES if not hasattr(lib, n)]


def test_makefile_builds_the_unit():
    srcs = re.search(r"^SRCS := (.*?)\n\S", open(MAKEFILE).read(), re.S | re.M).group(1)
    assert "csrc/g16_setup.hip" in srcs.split()
    assert os.path.exists(os.path.join(ROOT, "gnark-icicle_amd", "csrc", "g16_setup.hpp"))


def test_binding_lists_and_wraps_the_entries(lib):
    import gnark_mi355x as gm
    assert set(ENTRIES) <= set(gm.SYMBOLS)
    assert callable(gm.Context.batch_mul_fixed) and callable(gm.Context.set_fixed_base_window)
    L = gm.load_library()
    assert L.gm_batch_mul_fixed.argtypes == L.gm_batch_mul_base.argtypes
    assert L.gm_set_fixed_base_window.argtypes == L.gm_set_msm_window.argtypes
    assert callable(gm.Context.set_g16_setup_column_cut) and callable(gm.R1CS.g16_setup)
    assert callable(gm.ProvingKey.setup)
    # every member is one machine word, size_t or pointer: no padding to get wrong
    word = ctypes.sizeof(ctypes.c_void_p)
    assert ctypes.sizeof(ctypes.c_size_t) == word
    for S, fields in ((gm._G16SetupIn, IN_FIELDS), (gm._G16SetupOut, OUT_FIELDS)):
        assert [f[0] for f in S._fields_] == fields
        assert ctypes.sizeof(S) == len(fields) * word
        for k, name in enumerate(fields):
            assert getattr(S, name).offset == k * word and getattr(S, name).size == word, name
    kinds = dict(gm._G16SetupIn._fields_)
    assert kinds["nb_public"] is ctypes.c_size_t and kinds["nb_gamma"] is ctypes.c_size_t
    assert kinds["gamma_wires"] is ctypes.POINTER(ctypes.c_uint32)
    assert tuple(OUT_FIELDS) == gm.G16_SETUP_OUT_FIELDS


def _child(code):
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")
    return subprocess.run([sys.executable, "-c", code, LIB], env=env, capture_output=True, text=True, check=True)


PRELUDE = r"""
import ctypes, sys
L = ctypes.CDLL(sys.argv[1])
vp, sz = ctypes.c_void_p, ctypes.c_size_t
L.gm_last_error.restype = ctypes.c_char_p
L.gm_set_fixed_base_window.argtypes = [vp, ctypes.c_int]
L.gm_batch_mul_fixed.argtypes = [vp, ctypes.c_int, ctypes.c_int, vp, vp, sz, vp]
L.gm_set_g16_setup_column_cut.argtypes = [vp, ctypes.c_int]
L.gm_g16_setup_sizes.argtypes = [vp, vp, vp, vp, vp, vp]
L.gm_g16_setup.argtypes = [vp, vp, vp, vp]
L.gm_g16_pk_setup.argtypes = [vp, vp, vp, ctypes.c_uint, vp, vp]
class In(ctypes.Structure):
    _fields_ = [("toxic", vp), ("nb_public", sz), ("gamma_wires", vp), ("nb_gamma", sz)]
fake = (ctypes.c_uint8 * 8192)()
X = ctypes.addressof(fake)
def show(rc):
    print(rc, L.gm_last_error().decode().replace(" ", "_"))
"""


def test_null_handles_and_bad_arguments_are_refused_without_a_device():
    """Run in a child with every GPU hidden: the checks come before any HIP call."""
    code = PRELUDE + r"""
show(L.gm_set_fixed_base_window(None, 8))
show(L.gm_batch_mul_fixed(None, 0, 0, X, X, 4, X))
show(L.gm_batch_mul_fixed(X, 0, 0, None, X, 4, X))
show(L.gm_batch_mul_fixed(X, 0, 1, X, None, 4, X))
show(L.gm_batch_mul_fixed(X, 1, 0, X, X, 4, None))
show(L.gm_batch_mul_fixed(X, 7, 0, X, X, 4, X))
show(L.gm_batch_mul_fixed(X, -1, 1, X, X, 4, X))
show(L.gm_batch_mul_fixed(X, 0, 0, X, X, 1 << 32, X))
i = In()
I, O = ctypes.addressof(i), X + 4096
show(L.gm_set_g16_setup_column_cut(None, 8))
show(L.gm_g16_setup_sizes(None, X, I, O, O, O))
show(L.gm_g16_setup_sizes(X, None, I, O, O, O))
show(L.gm_g16_setup_sizes(X, X, None, O, O, O))
show(L.gm_g16_setup_sizes(X, X, I, None, O, O))
show(L.gm_g16_setup_sizes(X, X, I, O, None, O))
show(L.gm_g16_setup_sizes(X, X, I, O, O, None))
show(L.gm_g16_setup(None, X, I, O))
show(L.gm_g16_setup(X, None, I, O))
show(L.gm_g16_setup(X, X, None, O))
show(L.gm_g16_setup(X, X, I, None))
show(L.gm_g16_pk_setup(None, X, I, 0, O, None))
show(L.gm_g16_pk_setup(X, None, I, 0, O, None))
show(L.gm_g16_pk_setup(X, X, None, 0, O, None))
show(L.gm_g16_pk_setup(X, X, I, 0, None, None))
"""
    lines = [ln.split() for ln in _child(code).stdout.splitlines()]
    assert len(lines) == 23
    assert [ln[0] for ln in lines] == [str(GM_ERR_INVALID)] * 23
    want = ["gm_set_fixed_base_window:"] + ["gm_batch_mul_fixed:"] * 4 + ["unknown_curve"] * 2 + \
        ["gm_batch_mul_fixed:_n_must_be_below", "gm_set_g16_setup_column_cut:"] + ["gm_g16_setup_sizes:"] * 6 + \
        ["gm_g16_setup:"] * 4 + ["gm_g16_pk_setup:"] * 4
    for ln, w in zip(lines, want):
        assert ln[1].startswith(w), (ln, w)


def test_window_out_of_range_is_refused():
    """Judged before the context is touched: a stand-in pointer is enough."""
    code = PRELUDE + r"""
for c in (1, 17, -3, 100):
    show(L.gm_set_fixed_base_window(X, c))
"""
    lines = [ln.split() for ln in _child(code).stdout.splitlines()]
    assert len(lines) == 4
    assert [ln[0] for ln in lines] == [str(GM_ERR_INVALID)] * 4
    for ln in lines:
        assert ln[1].startswith("gm_set_fixed_base_window:_c_must_be_0_(the_model)_or_in_[2,_16]"), ln


def test_setup_host_checks_come_before_any_device_call():
    """On a stand-in context and a zeroed stand-in constraint system: the cut's range,
    unknown key flags, NULL toxic scalars and a system without wires."""
    code = PRELUDE + r"""
i = In()
I, O = ctypes.addressof(i), X + 4096
show(L.gm_set_g16_setup_column_cut(X, -1))
show(L.gm_set_g16_setup_column_cut(X, (1 << 30) + 1))
show(L.gm_g16_pk_setup(X, X, I, 4, O, None))
show(L.gm_g16_setup(X, X, I, O))
i.toxic = X + 2048
show(L.gm_g16_setup(X, X, I, O))
show(L.gm_g16_setup_sizes(X, X, I, O, O, O))
show(L.gm_g16_pk_setup(X, X, I, 1, O, None))
"""
    lines = [ln.split() for ln in _child(code).stdout.splitlines()]
    assert len(lines) == 7
    assert [ln[0] for ln in lines] == [str(GM_ERR_INVALID)] * 7
    want = ["gm_set_g16_setup_column_cut:_t_must_be"] * 2 + ["gm_g16_pk_setup:_unknown_flags",
            "gm_g16_setup:_the_toxic_scalars_are_NULL", "gm_g16_setup:_the_R1CS_has_no_wire",
            "gm_g16_setup_sizes:_the_R1CS_has_no_wire", "gm_g16_pk_setup:_the_R1CS_has_no_wire"]
    for ln, w in zip(lines, want):
        assert ln[1].startswith(w), (ln, w)
