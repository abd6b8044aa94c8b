"""gm_plonk_wires_permutation / gm_plonk_sigma_wires / gm_plonk_pk_setup_wires
without a GPU: the three entries through header, library, binding and Makefile,
the refusals that need no device, and the vectorised model of gnark's
buildPermutation (setup.go:271-325) that the GPU tests compare against, checked
here against the loop in test_plonk_setup_gpu.build_permutation."""
import ctypes
import os
import re

import numpy as np
import pytest

from test_plonk_setup_gpu import build_permutation

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "gnark_mi355x.h")
NAMES = ("gm_plonk_wires_permutation", "gm_plonk_sigma_wires", "gm_plonk_pk_setup_wires")


def perm_model(lro):
    """buildPermutation on lro (position -> wire id), vectorised: sort the positions
    by wire id, stably; inside a run each position points to its predecessor, the
    first one to the last."""
    lro = np.asarray(lro).reshape(-1)
    order = np.argsort(lro, kind="stable")
    k = lro[order]
    head = np.r_[True, k[1:] != k[:-1]]
    tail = np.r_[head[1:], True]
    prev = np.r_[0, order[:-1]]
    rid = np.cumsum(head) - 1
    prev[head] = order[tail][rid[head]]
    perm = np.empty_like(order)
    perm[order] = prev
    return perm.astype(np.int64)


def one_wire(n):
    """Every position holds wire 0: perm[p] = p - 1, perm[0] = 3n - 1."""
    return np.zeros((3, n), np.uint32), 1, np.r_[3 * n - 1, np.arange(3 * n - 1)].astype(np.int64)


def distinct_descending(n):
    """3n distinct wires in descending order: every wire occurs once, the identity."""
    t = np.arange(3 * n - 1, -1, -1, dtype=np.uint32).reshape(3, n)
    return t, 3 * n, np.arange(3 * n, dtype=np.int64)


def alternating(n):
    """Wire p % 2 at position p: p - 2, and the first two point to the last two."""
    t = (np.arange(3 * n, dtype=np.uint32) % 2).reshape(3, n)
    want = np.arange(3 * n, dtype=np.int64) - 2
    want[0], want[1] = 3 * n - 2, 3 * n - 1
    return t, 2, want


CLOSED_FORMS = (one_wire, distinct_descending, alternating)


def random_tables(n, nb_wires, seed):
    """Random ids below nb_wires; 0, nb_wires - 1 and nb_wires - 2 occur (the top
    digit of the sort is used), some of them more than once."""
    rng = np.random.default_rng(seed)
    t = rng.integers(0, nb_wires, size=(3, n), dtype=np.uint32)
    top, sub = nb_wires - 1, max(nb_wires - 2, 0)
    t[0, 1], t[1, 2], t[2, 3] = top, sub, 0
    t[2, n - 1], t[0, 5], t[1, 0] = top, sub, 0
    return t


def test_header_declares_the_entries_inside_the_setup_block():
    src = open(HEADER).read()
    lo, hi = src.index("---- PLONK setup on the device"), src.index("---- NTT (iciclegnark")
    assert lo < hi
    at = [src.index("int %s(" % name) for name in NAMES]
    assert lo < src.index("int gm_plonk_pk_setup(") < at[0] < at[1] < at[2] < hi
    assert re.search(r"int gm_plonk_wires_permutation\(gm_ctx\* ctx, const gm_plonk_wires\* w, int64_t\* perm_dev", src)


def test_library_and_binding_have_the_entries():
    import gnark_mi355x as gm
    L = gm.load_library()
    for name in NAMES:
        assert name in gm.SYMBOLS
        assert hasattr(L, name), name
    assert callable(gm.PlonkWires.permutation) and callable(gm.Context.plonk_sigma_wires)
    assert callable(gm.PlonkProvingKey.setup_from_wires)


def test_makefile_builds_the_unit():
    mk = open(os.path.join(ROOT, "gnark-icicle_amd", "Makefile")).read()
    srcs = mk[mk.index("SRCS :="):mk.index("OBJS :=")]
    assert "csrc/plonk_wires_perm.hip" in srcs
    assert os.path.exists(os.path.join(ROOT, "gnark-icicle_amd", "csrc", "plonk_wires_perm.hip"))


def test_null_arguments_are_refused_before_any_device_call():
    """No context exists in this process: a call that reached the device would fail
    with another code and another message."""
    import gnark_mi355x as gm
    L = gm.load_library()
    L.gm_last_error.restype = ctypes.c_char_p
    x = ctypes.c_void_p(0x1000)  # never dereferenced: a NULL beside it is found first
    h = gm._PlonkSetupHost()
    out = ctypes.c_void_p()
    cases = {
        "plonk wires permutation": [lambda: L.gm_plonk_wires_permutation(None, x, x),
                                    lambda: L.gm_plonk_wires_permutation(x, None, x),
                                    lambda: L.gm_plonk_wires_permutation(x, x, None)],
        "plonk sigma wires": [lambda: L.gm_plonk_sigma_wires(None, 0, x, x, x, x),
                              lambda: L.gm_plonk_sigma_wires(x, 0, None, x, x, x),
                              lambda: L.gm_plonk_sigma_wires(x, 0, x, None, x, x),
                              lambda: L.gm_plonk_sigma_wires(x, 0, x, x, None, x),
                              lambda: L.gm_plonk_sigma_wires(x, 0, x, x, x, None)],
        "plonk pk setup wires": [lambda: L.gm_plonk_pk_setup_wires(None, 0, ctypes.byref(h), x, 0, ctypes.byref(out), x, None),
                                 lambda: L.gm_plonk_pk_setup_wires(x, 0, None, x, 0, ctypes.byref(out), x, None),
                                 lambda: L.gm_plonk_pk_setup_wires(x, 0, ctypes.byref(h), None, 0, ctypes.byref(out), x, None),
                                 lambda: L.gm_plonk_pk_setup_wires(x, 0, ctypes.byref(h), x, 0, None, x, None)],
    }
    for what, calls in cases.items():
        for k, call in enumerate(calls):
            assert call() == -1, (what, k)
            msg = L.gm_last_error().decode()
            assert what in msg and "null" in msg.lower(), (what, k, msg)


@pytest.mark.parametrize("n", [8, 64, 1024])
def test_vectorised_model_equals_the_loop(n):
    for nb_wires in (1, 2, 5, n // 2 + 3, 3 * n):
        t = random_tables(n, nb_wires, 0xA100 + n + nb_wires)
        got = perm_model(t)
        assert got.tolist() == build_permutation(t, nb_wires), nb_wires
        assert sorted(got.tolist()) == list(range(3 * n))
    # 2^32 - 1 wires: the loop's per-wire table would not fit, so it runs on the
    # ids' ranks (the permutation depends on the ids' equalities only)
    t = random_tables(n, 2**32 - 1, 0xA1FF + n)
    assert int(t.max()) == 2**32 - 2
    _, ranks = np.unique(t.reshape(-1), return_inverse=True)
    assert perm_model(t).tolist() == build_permutation(ranks.reshape(3, n), int(ranks.max()) + 1)


@pytest.mark.parametrize("n", [8, 64, 1024])
@pytest.mark.parametrize("form", CLOSED_FORMS)
def test_closed_forms(form, n):
    t, nb_wires, want = form(n)
    assert int(t.max()) < nb_wires
    assert perm_model(t).tolist() == want.tolist()
    assert build_permutation(t, nb_wires) == want.tolist()
