"""gm_plonk_scs_* / gm_plonk_pk_setup_scs without a GPU: the entries through
header, library, binding and Makefile, the refusals that need no device, and the
model of plonk_scs_model.py against the conventions the existing tests use
(test_plonk_witness_gpu.tables, test_plonk_setup_gpu.build_permutation)."""
import ctypes
import os
import re

import numpy as np
import pytest

import plonk_scs_model as model
import pyref
from test_plonk_setup_gpu import build_permutation
from test_plonk_wires_perm_abi import perm_model
from test_plonk_witness_gpu import tables as witness_tables

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "gnark_mi355x.h")
NAMES = ("gm_plonk_scs_upload", "gm_plonk_scs_bytes", "gm_plonk_scs_free", "gm_plonk_scs_wires",
         "gm_plonk_scs_selector", "gm_plonk_pk_setup_scs", "gm_plonk_scs_check")
ERR_INVALID, ERR_UNSUPPORTED = -1, -4


def test_header_declares_the_entries_in_their_own_block():
    src = open(HEADER).read()
    lo, hi = src.index("---- PLONK circuit on the device"), src.index("---- NTT (iciclegnark")
    assert src.index("int gm_plonk_pk_setup_wires(") < lo < hi
    at = [src.index("int %s(" % name) for name in NAMES]
    assert lo < min(at) and max(at) < hi
    assert re.search(r"enum \{ GM_SCS_QL, GM_SCS_QR, GM_SCS_QM, GM_SCS_QO, GM_SCS_QK, GM_SCS_QCP0", src)
    assert "} gm_plonk_scs_host;" in src


def test_library_and_binding_have_the_entries():
    import gnark_mi355x as gm
    L = gm.load_library()
    for name in NAMES:
        assert name in gm.SYMBOLS
        assert hasattr(L, name), name
    for method in ("wires", "selector", "check", "free", "resident_bytes"):
        assert callable(getattr(gm.PlonkCircuit, method))
    assert callable(gm.PlonkProvingKey.setup_from_circuit)
    assert (gm.SCS_QL, gm.SCS_QR, gm.SCS_QM, gm.SCS_QO, gm.SCS_QK, gm.SCS_QCP0) == (0, 1, 2, 3, 4, 5)
    # the struct as the header lays it out: eleven words
    assert ctypes.sizeof(gm._PlonkScsHost) == 11 * ctypes.sizeof(ctypes.c_size_t)


def test_makefile_builds_the_unit():
    mk = open(os.path.join(ROOT, "gnark-icicle_amd", "Makefile")).read()
    srcs = mk[mk.index("SRCS :="):mk.index("OBJS :=")]
    assert "csrc/plonk_scs.hip" in srcs
    for f in ("plonk_scs.hip", "plonk_scs.hpp"):
        assert os.path.exists(os.path.join(ROOT, "gnark-icicle_amd", "csrc", f))


def test_null_arguments_are_refused_before_any_device_call():
    """No context exists in this process: a call that reached the device would fail
    with another code and another message."""
    import gnark_mi355x as gm
    L = gm.load_library()
    x = ctypes.c_void_p(0x1000)  # never dereferenced: a NULL beside it is found first
    h = gm._PlonkScsHost()
    out = ctypes.c_void_p()
    sz = ctypes.c_size_t()
    o, hh, s = ctypes.byref(out), ctypes.byref(h), ctypes.byref(sz)
    cases = {
        "plonk scs upload": [lambda: L.gm_plonk_scs_upload(None, 0, hh, o),
                             lambda: L.gm_plonk_scs_upload(x, 0, None, o),
                             lambda: L.gm_plonk_scs_upload(x, 1, hh, None)],
        "plonk scs bytes": [lambda: L.gm_plonk_scs_bytes(None, s), lambda: L.gm_plonk_scs_bytes(x, None)],
        "plonk scs free": [lambda: L.gm_plonk_scs_free(None, x), lambda: L.gm_plonk_scs_free(x, None)],
        "plonk scs wires": [lambda: L.gm_plonk_scs_wires(None, o), lambda: L.gm_plonk_scs_wires(x, None)],
        "plonk scs selector": [lambda: L.gm_plonk_scs_selector(None, x, 0, x),
                               lambda: L.gm_plonk_scs_selector(x, None, 0, x),
                               lambda: L.gm_plonk_scs_selector(x, x, 0, None)],
        "plonk pk setup scs": [lambda: L.gm_plonk_pk_setup_scs(None, x, x, 11, 0, o, x, None),
                               lambda: L.gm_plonk_pk_setup_scs(x, None, x, 11, 0, o, x, None),
                               lambda: L.gm_plonk_pk_setup_scs(x, x, x, 11, 0, None, x, None)],
        "plonk scs check": [lambda: L.gm_plonk_scs_check(None, x, x, s, s),
                            lambda: L.gm_plonk_scs_check(x, None, x, s, s),
                            lambda: L.gm_plonk_scs_check(x, x, None, s, s),
                            lambda: L.gm_plonk_scs_check(x, x, x, None, s),
                            lambda: L.gm_plonk_scs_check(x, x, x, s, None)],
    }
    for what, calls in cases.items():
        for k, call in enumerate(calls):
            assert call() == ERR_INVALID, (what, k)
            msg = L.gm_last_error().decode()
            assert what in msg and "null" in msg.lower(), (what, k, msg)


def test_curve_ids():
    import gnark_mi355x as gm
    L = gm.load_library()
    x = ctypes.c_void_p(0x1000)
    h = gm._PlonkScsHost()
    out = ctypes.c_void_p()
    assert L.gm_plonk_scs_upload(x, 2, ctypes.byref(h), ctypes.byref(out)) == ERR_UNSUPPORTED
    msg = L.gm_last_error().decode()
    assert "gm_plonk_scs_upload" in msg and "BLS12-381" in msg, msg
    for curve in (3, -1):
        assert L.gm_plonk_scs_upload(x, curve, ctypes.byref(h), ctypes.byref(out)) == ERR_INVALID
        assert "unknown curve id" in L.gm_last_error().decode()


def as_records(t, nb_public, nb_constraints):
    """Records whose wire ids are the constraint rows of complete tables."""
    rec = np.zeros((nb_constraints, 9), np.uint32)
    rec[:, :3] = t[:, nb_public:nb_public + nb_constraints].T
    return rec


@pytest.mark.parametrize("n", [8, 64, 1024])
def test_model_tables_follow_the_existing_convention(n):
    """test_plonk_witness_gpu.tables: two public rows, two padding rows."""
    for nb_wires in (2, 5, n, 3 * n):
        t = witness_tables(n, nb_wires, 0xC100 + n + nb_wires)
        got = model.tables(as_records(t, 2, n - 4), n, 2)
        assert np.array_equal(got, t)
        # and its permutation input gives gnark's permutation on the same rows
        assert perm_model(got).tolist() == build_permutation(t, nb_wires)


def test_model_selectors_and_gate_on_a_hand_made_circuit():
    c = pyref.CURVES["bn254"]
    r = c.r
    coeffs = [0, 1, 2, r - 1, r - 2, 7]
    # x2 = x0 * x1 ; x3 = 7 x2 + 2 ; a COMMITTED row that does not hold
    rec = np.array([[0, 1, 2, 0, 0, 3, 1, 0, model.NOT],
                    [2, 0, 3, 5, 0, 3, 0, 2, model.NOT],
                    [1, 1, 1, 1, 1, 1, 1, 1, model.COMMITTED]], np.uint32)
    wit = [3, 4, 12, 86]
    assert model.unsatisfied(c, rec, coeffs, wit) == []
    assert model.unsatisfied(c, rec, coeffs, [3, 4, 13, 86]) == [0, 1]
    assert model.unsatisfied(c, rec, coeffs, [3, 4, 12, 87]) == [1]
    cols, qcp = model.selectors(c, rec, coeffs, 8, 2, [[2, 2]])
    assert cols["ql"] == [r - 1, r - 1, 0, 7, 1, 0, 0, 0]
    assert cols["qm"] == [0, 0, 1, 0, 1, 0, 0, 0] and cols["qo"] == [0, 0, r - 1, r - 1, 1, 0, 0, 0]
    assert cols["qk"] == [0, 0, 0, 2, 1, 0, 0, 0] and cols["qr"] == [0, 0, 0, 0, 1, 0, 0, 0]
    assert qcp == [[0, 0, 0, 0, 1, 0, 0, 0]]
    raw = model.selector_bytes(c, rec, coeffs, 8, 2, [[2, 2]])
    for col, want in zip(raw, [cols[k] for k in model.SELECTOR_NAMES] + qcp):
        assert col.tobytes() == model.enc(c, want)
    assert model.tables(rec, 8, 2).tolist() == [[0, 1, 0, 2, 1, 0, 0, 0], [0, 0, 1, 0, 1, 0, 0, 0],
                                                [0, 0, 2, 3, 1, 0, 0, 0]]


@pytest.mark.parametrize("cname", ["bn254", "bls12377"])
def test_generators(cname):
    c = pyref.CURVES[cname]
    for n, pub, nc, ncoeffs in ((8, 2, 6, 5), (64, 0, 64, 6), (1024, 3, 1000, 1000)):
        k = model.random_circuit(c, n, pub, nc, n // 2 + 3, ncoeffs, 0xC200 + n, nb_bsb=2)
        rec = k.records
        assert rec[:, :3].min() == 0 and rec[:, :3].max() == k.nb_wires - 1
        assert rec[:, 3:8].min() == 0 and rec[:, 3:8].max() == ncoeffs - 1
        assert {model.COMMITTED, model.COMMITMENT_ROW} <= set(rec[:, 8].tolist()) <= {0, 1, 2}
        cols, qcp = model.selectors(c, rec, k.coeffs, n, pub, k.committed)
        raw = model.selector_bytes(c, rec, k.coeffs, n, pub, k.committed)
        for col, want in zip(raw, [cols[name] for name in model.SELECTOR_NAMES] + qcp):
            assert col.tobytes() == model.enc(c, want)
        sat = model.chain_circuit(c, n, pub, nc, 0xC300 + n, commitments=True)
        assert sat.nb_wires == max(pub, 2) + nc and len(sat.witness) == sat.nb_wires
        assert model.unsatisfied(c, sat.records, sat.coeffs, sat.witness) == []
        # the rows the solver skips do not hold
        plain = sat.records.copy()
        plain[:, 8] = model.NOT
        assert model.unsatisfied(c, plain, sat.coeffs, sat.witness) == [1, 2, 5]
