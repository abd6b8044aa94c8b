"""gm_plonk_wires_permutation / gm_plonk_sigma_wires / gm_plonk_pk_setup_wires:
gnark's trace.S derived on the device from resident wire tables, and S1-S3 and
the resident key from it.

Every comparison is for exact equality: an unstable sort would give a valid
permutation with the same cycles and another verifying key.  The expected
permutation is buildPermutation in numpy (test_plonk_wires_perm_abi.perm_model,
checked there against the loop of test_plonk_setup_gpu.build_permutation)."""
import ctypes
import functools

import numpy as np
import pytest

import pyref
import test_plonk_witness_gpu as pw
from test_plonk_session_gpu import Inst, assert_same, enc, make_key, run_proof, srs
from test_plonk_setup_gpu import build_permutation, setup_key, sigma, sigma_model
from test_plonk_wires_perm_abi import CLOSED_FORMS, perm_model, random_tables

pytestmark = pytest.mark.gpu

CURVES = ("bn254", "bls12377")
# 8-bit digits: nb_wires - 1 has 0, 1, 1, 1, 2, 2, 2, 3, 3, 4, 4 bytes
NB_WIRES = (1, 2, 255, 256, 257, 65535, 65536, 65537, 1 << 24, (1 << 24) + 1, (1 << 32) - 1)


def device_perm(ctx, t, nb_wires):
    import gnark_mi355x as gm
    n = t.shape[1]
    w = gm.PlonkWires(ctx, n, nb_wires, *t)
    buf = None
    try:
        buf = w.permutation()
        assert buf.nbytes == 24 * n
        return np.frombuffer(buf.to_host(), np.int64)
    finally:
        w.free()
        if buf is not None:
            buf.free()


def assert_perm(got, want):
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (bad.size, bad[:8].tolist(), got[bad[:8]].tolist(), want[bad[:8]].tolist())


@functools.lru_cache(maxsize=None)
def big_case():
    """2^19 rows, 1.5 M entries: every grid-stride loop takes a second turn."""
    n = 1 << 19
    t = random_tables(n, n // 2, 0xB219)
    return t, n // 2, perm_model(t)


# ---------------------------------------------------------------------------
# 1. the size and pass grid
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("n", [8, 64, 1024, 1 << 15])
def test_grid(gm_ctx, n):
    for nb_wires in NB_WIRES:
        t = random_tables(n, nb_wires, 0xB100 + n + nb_wires % 977)
        ids = set(t.reshape(-1).tolist())
        assert {0, nb_wires - 1, max(nb_wires - 2, 0)} <= ids
        got = device_perm(gm_ctx, t, nb_wires)
        assert_perm(got, perm_model(t))


def test_second_turn_of_the_grid_stride_loops(gm_ctx):
    t, nb_wires, want = big_case()
    assert_perm(device_perm(gm_ctx, t, nb_wires), want)


# ---------------------------------------------------------------------------
# 2. closed forms, stability, gnark's shape
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("n", [8, 1024, 1 << 15])
@pytest.mark.parametrize("form", CLOSED_FORMS)
def test_closed_forms(gm_ctx, form, n):
    t, nb_wires, want = form(n)
    assert_perm(device_perm(gm_ctx, t, nb_wires), want)


@pytest.mark.parametrize("nb_wires", [3, 7])
def test_long_runs_stay_in_position_order(gm_ctx, nb_wires):
    """Every run is spread over all waves of a tile and over many tiles."""
    n = 1 << 15
    t = np.random.default_rng(0xB300 + nb_wires).integers(0, nb_wires, size=(3, n), dtype=np.uint32)
    want = perm_model(t)
    got = device_perm(gm_ctx, t, nb_wires)
    assert_perm(got, want)
    # what stability means, said directly: a position points below itself unless
    # it is its wire's first
    lro = t.reshape(-1)
    first = np.array([np.flatnonzero(lro == v)[0] for v in range(nb_wires)])
    rest = np.setdiff1d(np.arange(3 * n), first)
    assert (got[rest] < rest).all() and (got[first] >= first).all()


def test_gnark_shape(gm_ctx):
    n, nb_wires = 64, 64 // 2 + 3
    t = pw.tables(n, nb_wires, 0xB400).copy()
    once, never = nb_wires - 2, nb_wires - 3
    t[(t == once) | (t == never)] = 1
    t[1, 20] = once
    lro = t.reshape(-1)
    assert (lro == once).sum() == 1 and (lro == never).sum() == 0
    assert (t[1:, :2] == 0).all() and (t[:, n - 2:] == 0).all()  # placeholder and padding rows
    got = device_perm(gm_ctx, t, nb_wires)
    assert sorted(got.tolist()) == list(range(3 * n)) and got.tolist() != list(range(3 * n))
    assert got[n + 20] == n + 20
    assert got.tolist() == build_permutation(t, nb_wires)


# ---------------------------------------------------------------------------
# 3. state: stale workspace, the tables, trim, the output's bounds
# ---------------------------------------------------------------------------
def test_small_call_after_a_large_one(gm_ctx):
    t, nb_wires, want = big_case()
    assert_perm(device_perm(gm_ctx, t, nb_wires), want)
    # the workspace now holds the large call's counters and positions
    for nb in (1, 2, 300):
        s = random_tables(8, nb, 0xB500 + nb)
        assert_perm(device_perm(gm_ctx, s, nb), perm_model(s))


def test_tables_unchanged_reuse_trim_and_guard(gm_ctx):
    import gnark_mi355x as gm
    n, nb_wires = 1024, 700
    t = random_tables(n, nb_wires, 0xB600)
    want = perm_model(t)
    W = np.random.default_rng(0xB601).integers(0, 256, size=(nb_wires, 32), dtype=np.uint8)
    w = gm.PlonkWires(gm_ctx, n, nb_wires, *t)
    wit = gm_ctx.copy_to_device(W)
    lro = [gm_ctx.malloc(32 * n) for _ in range(3)]
    guard = 4096
    pattern = np.full(guard + 24 * n + guard, 0xA5, np.uint8)
    raw = gm_ctx.copy_to_device(pattern)
    out = gm.DeviceBuffer(gm_ctx, raw.ptr + guard, 24 * n)
    try:
        def gathered():
            w.gather(wit, *lro)
            return [b.to_host() for b in lro]

        before = gathered()
        assert before == [W[t[k]].tobytes() for k in range(3)]
        for turn in range(3):
            assert w.permutation(out) is out
            back = np.frombuffer(raw.to_host(), np.uint8)
            assert (back[:guard] == 0xA5).all() and (back[guard + 24 * n:] == 0xA5).all(), turn
            assert_perm(np.frombuffer(back[guard:guard + 24 * n].tobytes(), np.int64), want)
            raw.write(pattern)
            if turn == 0:
                gm_ctx.trim()
            if turn == 1:  # the fused call in between, on the same tables
                for b in gm_ctx.plonk_sigma_wires("bn254", w):
                    b.free()
        assert gathered() == before
        assert w.resident_bytes() == 12 * n
    finally:
        w.free()
        for b in [wit, raw] + lro:
            b.free()


# ---------------------------------------------------------------------------
# 4. S1, S2, S3 from the tables
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("n", [8, 64, 1024])
@pytest.mark.parametrize("cname", CURVES)
def test_sigma_wires(gm_ctx, cname, n):
    import gnark_mi355x as gm
    c = pyref.CURVES[cname]
    nb_wires = n // 2 + 3
    t = pw.tables(n, nb_wires, 0xB700 + n)
    built = build_permutation(t, nb_wires)
    w = gm.PlonkWires(gm_ctx, n, nb_wires, *t)
    bufs = ()
    try:
        bufs = gm_ctx.plonk_sigma_wires(cname, w)
        got = b"".join(b.to_host() for b in bufs)
    finally:
        w.free()
        for b in bufs:
            b.free()
    assert len(got) == 3 * 32 * n
    assert got == sigma(gm_ctx, cname, n, np.array(built, np.int64))
    assert got == enc(c, sigma_model(c, n, built))


# ---------------------------------------------------------------------------
# 5. the key from the tables
# ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def wires_case(cname, n, nb):
    """A random instance whose s1, s2, s3 are the integer model of the permutation
    of random wire tables."""
    c = pyref.CURVES[cname]
    inst = Inst(c, n, nb, 0xB800 + 16 * n + nb)
    inst.nb_wires = n // 2 + 3
    inst.tables = pw.tables(n, inst.nb_wires, 0xB900 + n + nb)
    inst.perm = build_permutation(inst.tables, inst.nb_wires)
    s = sigma_model(c, n, inst.perm)
    inst.fixed.update(s1=s[:n], s2=s[n:2 * n], s3=s[2 * n:])
    return inst


def check_key_from_wires(gm_ctx, oracle, cname, n, nb, cache):
    inst = wires_case(cname, n, nb)
    _, _, lag, _ = srs(oracle, cname, n)
    w = pw.make_wires(gm_ctx, inst)
    keys = []
    try:
        key, digests, lag_out = setup_key(gm_ctx, oracle, cname, inst, cache=cache, permutation=None, wires=w)
        keys.append(key)
        w.free()  # the key does not refer to the tables
        host, host_digests, host_lag = setup_key(gm_ctx, oracle, cname, inst, cache=cache)
        keys.append(host)
        up = make_key(gm_ctx, oracle, cname, inst, cache=cache)
        keys.append(up)
        assert len(digests) == 8 + nb and digests == host_digests
        assert lag_out == host_lag == lag
        assert key.resident_bytes() == host.resident_bytes() == up.resident_bytes()
        assert (key.resident_bytes()[1] == 0) == (not cache)
        want = run_proof(up, inst, True)
        assert_same(run_proof(key, inst, True), want)
        assert_same(run_proof(host, inst, True), want)
    finally:
        w.free()
        for k in keys:
            k.free()


@pytest.mark.parametrize("nb", [0, 2])
@pytest.mark.parametrize("n", [8, 64])
@pytest.mark.parametrize("cname", CURVES)
def test_key_from_wires(gm_ctx, oracle, cname, n, nb):
    check_key_from_wires(gm_ctx, oracle, cname, n, nb, True)


@pytest.mark.parametrize("cname", CURVES)
def test_key_from_wires_without_the_coset_cache(gm_ctx, oracle, cname):
    check_key_from_wires(gm_ctx, oracle, cname, 64, 2, False)


def test_setup_from_wires_is_the_same_call(gm_ctx, oracle):
    import gnark_mi355x as gm
    cname, n, nb = "bn254", 8, 0
    inst = wires_case(cname, n, nb)
    c = inst.c
    _, can, _, _ = srs(oracle, cname, n)
    w = pw.make_wires(gm_ctx, inst)
    key = None
    try:
        key, digests, lag = gm.PlonkProvingKey.setup_from_wires(
            gm_ctx, cname, n, 2, {k: enc(c, inst.fixed[k]) for k in gm.PLONK_SETUP_POLYS}, w, [], [], can)
        host, host_digests, _ = setup_key(gm_ctx, oracle, cname, inst)
        host.free()
        assert digests == host_digests and lag is None
    finally:
        w.free()
        if key is not None:
            key.free()


# ---------------------------------------------------------------------------
# 6. refusals: each is followed by a correct call
# ---------------------------------------------------------------------------
def refused(f, *a, **kw):
    import gnark_mi355x as gm
    with pytest.raises(gm.GmError) as e:
        f(*a, **kw)
    assert "error -1: plonk" in str(e.value), str(e.value)
    return str(e.value)


def test_permutation_refusals(gm_ctx):
    """Not constructible from here: an output that overlaps the tables (their
    address is not exposed) and n > 2^30 (a 12 GiB upload)."""
    import gnark_mi355x as gm
    n, nb_wires = 64, 40
    t = random_tables(n, nb_wires, 0xBA00)
    want = perm_model(t)
    L = gm.load_library()
    w = gm.PlonkWires(gm_ctx, n, nb_wires, *t)
    raw = gm_ctx.malloc(24 * n + 8)
    other = gm.Context(0)
    foreign = gm.PlonkWires(other, n, nb_wires, *t)
    try:
        def ok():
            out = gm.DeviceBuffer(gm_ctx, raw.ptr, 24 * n)
            w.permutation(out)
            assert_perm(np.frombuffer(out.to_host(), np.int64), want)

        ok()
        msg = refused(w.permutation, gm.DeviceBuffer(gm_ctx, raw.ptr + 4, 24 * n))
        assert "plonk wires permutation: perm_dev must be 8-byte aligned" in msg
        ok()
        assert L.gm_plonk_wires_permutation(gm_ctx.handle, foreign.handle, ctypes.c_void_p(raw.ptr)) == -1
        assert "plonk wires permutation: the tables were uploaded on another context" in L.gm_last_error().decode()
        ok()
        for args in ((None, w.handle, ctypes.c_void_p(raw.ptr)), (gm_ctx.handle, None, ctypes.c_void_p(raw.ptr)),
                     (gm_ctx.handle, w.handle, None)):
            assert L.gm_plonk_wires_permutation(*args) == -1
            assert "plonk wires permutation: a required pointer is NULL" in L.gm_last_error().decode()
        ok()
    finally:
        foreign.free()
        other.close()
        w.free()
        raw.free()


@pytest.mark.parametrize("cname", CURVES)
def test_sigma_wires_refusals(gm_ctx, cname):
    """Not constructible from here: n above the curve's limit (2^28 rows and more)."""
    import gnark_mi355x as gm
    c = pyref.CURVES[cname]
    n, nb_wires = 8, 5
    t = pw.tables(n, nb_wires, 0xBB00)
    L = gm.load_library()
    w = gm.PlonkWires(gm_ctx, n, nb_wires, *t)
    other = gm.Context(0)
    foreign = gm.PlonkWires(other, n, nb_wires, *t)
    s = [gm_ctx.malloc(32 * n) for _ in range(3)]
    ptrs = [ctypes.c_void_p(b.ptr) for b in s]
    try:
        def ok():
            assert L.gm_plonk_sigma_wires(gm_ctx.handle, gm.curve_id(cname), w.handle, *ptrs) == 0
            assert b"".join(b.to_host() for b in s) == enc(c, sigma_model(c, n, build_permutation(t, nb_wires)))

        ok()
        assert L.gm_plonk_sigma_wires(gm_ctx.handle, 7, w.handle, *ptrs) == -1
        assert "unknown curve id" in L.gm_last_error().decode()
        ok()
        assert L.gm_plonk_sigma_wires(gm_ctx.handle, gm.curve_id(cname), foreign.handle, *ptrs) == -1
        assert "plonk sigma wires: the tables were uploaded on another context" in L.gm_last_error().decode()
        ok()
        for k in range(3):
            p = list(ptrs)
            p[k] = None
            assert L.gm_plonk_sigma_wires(gm_ctx.handle, gm.curve_id(cname), w.handle, *p) == -1
            assert "plonk sigma wires: a required pointer is NULL" in L.gm_last_error().decode()
        ok()
    finally:
        foreign.free()
        other.close()
        w.free()
        for b in s:
            b.free()


@pytest.mark.parametrize("cname", CURVES)
def test_key_from_wires_refusals(gm_ctx, oracle, cname):
    import gnark_mi355x as gm
    n, nb = 64, 2
    inst = wires_case(cname, n, nb)
    c = inst.c
    fixed = {k: enc(c, inst.fixed[k]) for k in gm.PLONK_SETUP_POLYS}
    w = pw.make_wires(gm_ctx, inst)
    small = gm.PlonkWires(gm_ctx, 32, inst.nb_wires, *[x[:32] for x in inst.tables])
    other = gm.Context(0)
    foreign = gm.PlonkWires(other, n, inst.nb_wires, *inst.tables)
    try:
        for name, over, text in (
            ("a host permutation beside the tables", dict(permutation=inst.perm), "in->permutation must be null"),
            ("tables of another n", dict(wires=small), "the wire tables have n = 32, the key has n = 64"),
            ("tables of another context", dict(wires=foreign), "uploaded on another context"),
            ("null vk_digests", dict(digests=False), "vk_digests must be non-null"),
            ("n = 48", dict(n=48), "plonk"),
            ("short canonical SRS", dict(srs_canonical_len=n + 2), "plonk"),
            ("commitment row = n", dict(commitment_row=[3, n]), "plonk"),
            ("null ql", dict(polys=dict(fixed, ql=None)), "plonk"),
            ("null canonical SRS", dict(srs_canonical=None, srs_canonical_len=n + 3), "plonk"),
            ("null qcp table", dict(qcp=None), "plonk"),
        ):
            a = dict(permutation=None, wires=w)
            a.update(over)
            msg = refused(setup_key, gm_ctx, oracle, cname, inst, **a)
            assert text in msg, (name, msg)
            key, digests, _ = setup_key(gm_ctx, oracle, cname, inst, permutation=None, wires=w, lagrange=False)
            try:
                assert len(digests) == 8 + nb
            finally:
                key.free()
        # gm_plonk_pk_setup itself still wants its permutation
        assert "the permutation and vk_digests must be non-null" in refused(setup_key, gm_ctx, oracle, cname, inst,
                                                                            permutation=None)
        L = gm.load_library()
        h = gm._PlonkSetupHost()
        out = ctypes.c_void_p()
        assert L.gm_plonk_pk_setup_wires(gm_ctx.handle, gm.curve_id(cname), h, None, 0, ctypes.byref(out), None,
                                         None) == -1
        assert "plonk pk setup wires: a required pointer is NULL" in L.gm_last_error().decode()
        assert L.gm_plonk_pk_setup_wires(gm_ctx.handle, 7, h, w.handle, 0, ctypes.byref(out), None, None) == -1
        assert "unknown curve id" in L.gm_last_error().decode()
    finally:
        foreign.free()
        other.close()
        small.free()
        w.free()
