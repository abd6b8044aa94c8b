"""gm_plonk_scs_* / gm_plonk_pk_setup_scs: a PLONK constraint system resident on
the device, and what is made from it there: the wire tables, NewTrace's
selectors, the proving key and a check of a witness.

The selectors and the tables are words moved untouched, so they are compared byte
for byte against plonk_scs_model.py (Python integers and a numpy gather of the
encoded CoeffTable).  The key is compared against gm_plonk_pk_setup_wires given the
model's selectors and an uploaded copy of the model's tables: digests, Lagrange
SRS, resident bytes and whole proofs (test_plonk_session_gpu's proof loop).  The
check is compared against the gate equation in Python integers.
"""
import ctypes
import functools
import random
import types

import numpy as np
import pytest

import plonk_scs_model as model
import pyref
import test_plonk_session_gpu as ps
import test_plonk_witness_gpu as pw
from test_plonk_session_gpu import assert_same, challenge, dec, enc, run_proof, srs
from test_plonk_wires_perm_abi import perm_model

pytestmark = pytest.mark.gpu

CURVES = ps.CURVES
TILE = 256  # records per block of the split kernel (csrc/plonk_scs.hip)


def upload(ctx, cname, k, **over):
    import gnark_mi355x as gm
    a = dict(n=k.n, nb_public=k.nb_public, nb_wires=k.nb_wires, records=k.records, coeffs=enc(k.c, k.coeffs),
             committed=k.committed, commitment_index=k.commitment_index)
    a.update(over)
    return gm.PlonkCircuit(ctx, cname, **a)


def refused(f, *a, **kw):
    import gnark_mi355x as gm
    with pytest.raises(gm.GmError) as e:
        f(*a, **kw)
    assert "error -1: plonk" in str(e.value), str(e.value)
    return str(e.value)


def columns(k):
    return model.selector_bytes(k.c, k.records, k.coeffs, k.n, k.nb_public, k.committed)


# ---------------------------------------------------------------------------
# 1. selectors, byte for byte
# ---------------------------------------------------------------------------
GUARD = 64


def check_selectors(ctx, cname, k, buf=None):
    """Every column of k into buf (or a buffer of its own with guard bytes behind
    the column)."""
    import gnark_mi355x as gm
    n = k.n
    circ = upload(ctx, cname, k)
    own = buf is None
    if own:
        buf = ctx.malloc(32 * n + GUARD)
    try:
        want = columns(k)
        assert len(want) == 5 + len(k.commitment_index)
        resident = circ.resident_bytes()
        for which, col in enumerate(want):
            buf.write(np.full(32 * n + GUARD, 0xA5, np.uint8))
            circ.selector(which, gm.DeviceBuffer(ctx, buf.ptr, 32 * n))
            got = np.frombuffer(buf.to_host(32 * n + GUARD), np.uint8)
            assert np.array_equal(got[:32 * n].reshape(n, 32), col), which
            assert (got[32 * n:] == 0xA5).all(), which
        assert circ.resident_bytes() == resident
    finally:
        circ.free()
        if own:
            buf.free()


@pytest.mark.parametrize("nb_public,nb_constraints", [(0, 0), (0, 8), (2, 6), (2, 1)])
@pytest.mark.parametrize("cname", CURVES)
def test_selectors_n8(gm_ctx, cname, nb_public, nb_constraints):
    c = pyref.CURVES[cname]
    nb = 2 if nb_constraints >= 4 else 0
    k = model.random_circuit(c, 8, nb_public, nb_constraints, 5, 5, 0xD000 + nb_constraints, nb_bsb=nb)
    check_selectors(gm_ctx, cname, k)


@pytest.mark.parametrize("n,ncoeffs", [(64, 5), (64, 6), (1024, 1000), (1 << 15, 70000), (1 << 15, 6)])
@pytest.mark.parametrize("cname", CURVES)
def test_selectors(gm_ctx, cname, n, ncoeffs):
    c = pyref.CURVES[cname]
    k = model.random_circuit(c, n, 3, n - 7, n // 2 + 3, ncoeffs, 0xD100 + n + ncoeffs, nb_bsb=2)
    check_selectors(gm_ctx, cname, k)


@pytest.mark.parametrize("cname", CURVES)
def test_selectors_second_turn_of_the_grid_stride_loop(gm_ctx, cname):
    """2^19 rows are 2^20 lanes: twice the 2048 blocks of 256."""
    c = pyref.CURVES[cname]
    n = 1 << 19
    k = model.random_circuit(c, n, 2, n - 2, n, 1000, 0xD200, nb_bsb=1)
    check_selectors(gm_ctx, cname, k)


def test_small_selector_after_a_large_one(gm_ctx):
    import gnark_mi355x as gm
    c = pyref.CURVES["bn254"]
    big, n = 1 << 15, 8
    large = model.random_circuit(c, big, 2, big - 2, big, 6, 0xD300)
    small = model.random_circuit(c, n, 2, 6, 5, 5, 0xD301, nb_bsb=2)
    buf = gm_ctx.malloc(32 * big)
    a, b = upload(gm_ctx, "bn254", large), upload(gm_ctx, "bn254", small)
    try:
        a.selector(gm.SCS_QM, buf)
        before = buf.to_host()
        assert before == columns(large)[gm.SCS_QM].tobytes()
        for which in (gm.SCS_QL, gm.SCS_QCP0 + 1):
            b.selector(which, gm.DeviceBuffer(gm_ctx, buf.ptr, 32 * n))
            now = buf.to_host()
            assert now[:32 * n] == columns(small)[which].tobytes() and now[32 * n:] == before[32 * n:]
    finally:
        a.free()
        b.free()
        buf.free()


# ---------------------------------------------------------------------------
# 2. the split: the borrowed tables, read back through the gather
# ---------------------------------------------------------------------------
def read_tables(ctx, circ):
    """The three columns through gm_plonk_gather_lro of a witness whose element i
    encodes i."""
    n, nb_wires = circ.n, circ.nb_wires
    W = np.zeros((nb_wires, 8), np.uint32)
    W[:, 0] = np.arange(nb_wires, dtype=np.uint32)
    W[:, 7] = ~W[:, 0]
    wit = ctx.copy_to_device(W)
    out = [ctx.malloc(32 * n) for _ in range(3)]
    try:
        circ.wires().gather(wit, *out)
        cols = [np.frombuffer(b.to_host(), np.uint32).reshape(n, 8) for b in out]
        for col in cols:
            assert np.array_equal(col[:, 7], ~col[:, 0]) and not col[:, 1:7].any()
        return np.stack([col[:, 0] for col in cols])
    finally:
        wit.free()
        for b in out:
            b.free()


SPLIT_CASES = [(8, 0, 0), (8, 2, 1), (8, 0, 8), (1024, 2, 1), (1024, 3, TILE - 1), (1024, 0, TILE), (1024, 5, TILE + 1),
               (1024, 2, 1000), (1 << 15, 2, (1 << 15) - 5)]


@pytest.mark.parametrize("n,nb_public,nb_constraints", SPLIT_CASES)
def test_tables_and_permutation(gm_ctx, n, nb_public, nb_constraints):
    c = pyref.CURVES["bls12377"]
    nb_wires = max(n // 2 + 3, nb_public)
    k = model.random_circuit(c, n, nb_public, nb_constraints, nb_wires, 7, 0xD400 + n + nb_constraints)
    want = model.tables(k.records, n, nb_public)
    circ = upload(gm_ctx, "bls12377", k)
    try:
        assert np.array_equal(read_tables(gm_ctx, circ), want)
        w = circ.wires()
        assert w.resident_bytes() == 12 * n
        perm = w.permutation()
        try:
            assert np.array_equal(np.frombuffer(perm.to_host(), np.int64), perm_model(want))
        finally:
            perm.free()
    finally:
        circ.free()


@pytest.mark.parametrize("cname", CURVES)
def test_borrowed_tables_in_the_setup_calls(gm_ctx, oracle, cname):
    """gm_plonk_sigma_wires and gm_plonk_pk_setup_wires on the tables inside the
    circuit give what they give on an uploaded copy."""
    import gnark_mi355x as gm
    n, nb = 64, 2
    k, _ = key_case(cname, n, nb)
    c = k.c
    _, can, _, _ = srs(oracle, cname, n)
    cols, qcp = model.selectors(c, k.records, k.coeffs, n, k.nb_public, k.committed)
    circ = upload(gm_ctx, cname, k)
    copy = gm.PlonkWires(gm_ctx, n, k.nb_wires, *model.tables(k.records, n, k.nb_public))
    keys, bufs = [], []
    try:
        for w in (circ.wires(), copy):
            bufs.append(gm_ctx.plonk_sigma_wires(cname, w))
        for a, b in zip(*bufs):
            assert a.to_host() == b.to_host()
        key, digests, _ = gm.PlonkProvingKey.setup_from_wires(
            gm_ctx, cname, n, k.nb_public, {name: enc(c, cols[name]) for name in gm.PLONK_SETUP_POLYS},
            circ.wires(), [enc(c, q) for q in qcp], [k.nb_public + i for i in k.commitment_index], can)
        keys.append(key)
        ref, ref_digests, _ = reference_key(gm_ctx, oracle, cname, k)
        keys.append(ref)
        assert digests == ref_digests
    finally:
        for s in bufs:
            for b in s:
                b.free()
        copy.free()
        circ.free()
        for key in keys:
            key.free()


@pytest.mark.parametrize("nb_constraints", [(1 << 20) - 5, 1])
def test_split_second_turn_of_its_loops(gm_ctx, nb_constraints):
    """2^20 rows: more than 2048 tiles of records, or more than 2048 * 256 rows
    outside the constraints."""
    c = pyref.CURVES["bn254"]
    n = 1 << 20
    k = model.random_circuit(c, n, 2, nb_constraints, n + 11, 6, 0xD500 + nb_constraints)
    circ = upload(gm_ctx, "bn254", k)
    try:
        assert np.array_equal(read_tables(gm_ctx, circ), model.tables(k.records, n, 2))
        want = columns(k)[2]
        col = circ.selector(2)
        try:
            assert col.to_host() == want.tobytes()
        finally:
            col.free()
    finally:
        circ.free()


# ---------------------------------------------------------------------------
# 3. the key from the circuit = the key from the tables and the model's selectors
# ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def key_case(cname, n, nb):
    c = pyref.CURVES[cname]
    k = model.random_circuit(c, n, ps.NB_PUBLIC, n - 2, n // 2 + 3, 9, 0xD600 + 16 * n + nb, nb_bsb=nb)
    inst = ps.Inst(c, n, nb, 0xD700 + 16 * n + nb)  # the witness side of a proof; its fixed part is not used
    assert inst.rows == [ps.NB_PUBLIC + i for i in k.commitment_index]
    return k, inst


def reference_key(ctx, oracle, cname, k, cache=True):
    """gm_plonk_pk_setup_wires on the model's selectors and an uploaded copy of the
    model's tables."""
    import gnark_mi355x as gm
    c = k.c
    _, can, _, _ = srs(oracle, cname, k.n)
    cols, qcp = model.selectors(c, k.records, k.coeffs, k.n, k.nb_public, k.committed)
    w = gm.PlonkWires(ctx, k.n, k.nb_wires, *model.tables(k.records, k.n, k.nb_public))
    try:
        return gm.PlonkProvingKey.setup_from_wires(
            ctx, cname, k.n, k.nb_public, {name: enc(c, cols[name]) for name in gm.PLONK_SETUP_POLYS}, w,
            [enc(c, q) for q in qcp], [k.nb_public + i for i in k.commitment_index], can, cache=cache, lagrange=True)
    finally:
        w.free()


def check_key(ctx, oracle, cname, n, nb, cache):
    import gnark_mi355x as gm
    k, inst = key_case(cname, n, nb)
    _, can, lag, _ = srs(oracle, cname, n)
    circ = upload(ctx, cname, k)
    keys = []
    try:
        resident = circ.resident_bytes()
        key, digests, lag_out = gm.PlonkProvingKey.setup_from_circuit(circ, can, cache=cache, lagrange=True)
        keys.append(key)
        assert circ.resident_bytes() == resident
        circ.free()  # the key does not refer to the circuit
        ref, ref_digests, ref_lag = reference_key(ctx, oracle, cname, k, cache)
        keys.append(ref)
        assert len(digests) == 8 + nb and digests == ref_digests
        assert lag_out == ref_lag == lag
        assert key.resident_bytes() == ref.resident_bytes()
        assert (key.resident_bytes()[1] == 0) == (not cache)
        assert_same(run_proof(key, inst, True), run_proof(ref, inst, True))
    finally:
        circ.free()
        for key in keys:
            key.free()


@pytest.mark.parametrize("nb", [0, 2])
@pytest.mark.parametrize("n", [8, 64, 1024])
@pytest.mark.parametrize("cname", CURVES)
def test_key_from_circuit(gm_ctx, oracle, cname, n, nb):
    check_key(gm_ctx, oracle, cname, n, nb, True)


@pytest.mark.parametrize("cname", CURVES)
def test_key_from_circuit_without_the_coset_cache(gm_ctx, oracle, cname):
    check_key(gm_ctx, oracle, cname, 64, 2, False)


@functools.lru_cache(maxsize=None)
def chain(cname, n, commitments=True):
    return model.chain_circuit(pyref.CURVES[cname], n, ps.NB_PUBLIC, n - 4, 0xD800 + n, commitments=commitments)


@pytest.mark.parametrize("cname", CURVES)
def test_satisfiable_circuit_proves_from_the_witness_and_verifies(gm_ctx, oracle, cname):
    """Setup from the circuit and the canonical SRS alone, Prove from the witness
    alone through the borrowed tables: the verifier's identity at zeta holds
    (verify.go:213-225, as test_plonk_session_gpu states it)."""
    import gnark_mi355x as gm
    n = 64
    k = chain(cname, n, commitments=False)
    c, r = k.c, k.c.r
    rng = random.Random(0xD900)
    rnd = lambda m: [rng.randrange(r) for _ in range(m)]
    t = model.tables(k.records, n, k.nb_public)
    inst = types.SimpleNamespace(c=c, n=n, nb=0, sparse=[], pi2=[], cvals=[], witness=enc(c, k.witness),
                                 public=k.witness[:k.nb_public], h_rand=rnd(2), salt=b"chain",
                                 b={"bl": rnd(2), "br": rnd(2), "bo": rnd(2), "bz": rnd(3)},
                                 w={name: [k.witness[i] for i in t[j]] for j, name in enumerate("lro")})
    _, can, _, _ = srs(oracle, cname, n)
    circ = upload(gm_ctx, cname, k)
    key = None
    try:
        assert circ.check(inst.witness) == (0, None)
        key, _, _ = gm.PlonkProvingKey.setup_from_circuit(circ, can)
        got = pw.run_proof_witness(key, circ.wires(), inst, True)
        # the existing path on the same key, from host-gathered l, r, o
        assert_same(got, run_proof(key, inst, True))
    finally:
        circ.free()
        if key is not None:
            key.free()
    be = challenge(c, "beta", inst.salt, *got["bsb"], *got["lro"])
    ga = challenge(c, "gamma", inst.salt, *got["bsb"], *got["lro"])
    al, ze = challenge(c, "alpha", got["z"]), challenge(c, "zeta", *got["h"])
    lin_ze, le, re_, oe, s1e, s2e = dec(c, b"".join(got["claimed"]))
    (zue,) = dec(c, got["z_shifted"])
    l1 = (pow(ze, n, r) - 1) * pow(n * (ze - 1) % r, -1, r) % r
    assert lin_ze == -(al * (le + be * s1e + ga) % r * (re_ + be * s2e + ga) % r * (oe + ga) % r * zue
                       - al * al * l1) % r


# ---------------------------------------------------------------------------
# 4. the witness check
# ---------------------------------------------------------------------------
def with_qc(k, rows):
    """k with another constant in the given constraints: exactly those fail."""
    rec = k.records.copy()
    for i in rows:
        rec[i, model.QC] = 4 + (rec[i, model.QC] - 3) % (len(k.coeffs) - 4)
    out = types.SimpleNamespace(**vars(k))
    out.records = rec
    return out


def check_against_model(ctx, cname, k, witness):
    bad = model.unsatisfied(k.c, k.records, k.coeffs, witness)
    circ = upload(ctx, cname, k)
    try:
        resident = circ.resident_bytes()
        assert circ.check(enc(k.c, witness)) == (len(bad), bad[0] if bad else None)
        assert circ.resident_bytes() == resident
    finally:
        circ.free()
    return bad


@pytest.mark.parametrize("cname", CURVES)
def test_check(gm_ctx, cname):
    n = 64
    k = chain(cname, n)
    nc, r = k.nb_constraints, k.c.r
    # satisfied; the COMMITTED and COMMITMENT rows, which do not hold, are not reported
    assert check_against_model(gm_ctx, cname, k, k.witness) == []
    plain = types.SimpleNamespace(**vars(k))
    plain.records = k.records.copy()
    plain.records[:, model.COMMITMENT] = model.NOT
    assert check_against_model(gm_ctx, cname, plain, k.witness) == [1, 2, 5]
    # one corrupted wire: the rows that read it
    wit = list(k.witness)
    wit[ps.NB_PUBLIC + 20] = (wit[ps.NB_PUBLIC + 20] + 1) % r
    assert check_against_model(gm_ctx, cname, k, wit) == [20, 21, 22]
    # the first row only, the last row only, every row the solver looks at
    assert check_against_model(gm_ctx, cname, with_qc(k, [0]), k.witness) == [0]
    assert check_against_model(gm_ctx, cname, with_qc(k, [nc - 1]), k.witness) == [nc - 1]
    every = check_against_model(gm_ctx, cname, k, [0] * k.nb_wires)
    assert every == [i for i in range(nc) if i not in (1, 2, 5)]


@pytest.mark.parametrize("cname", CURVES)
def test_check_minimum_across_blocks(gm_ctx, cname):
    n = 1 << 15
    k = chain(cname, n)
    nc = k.nb_constraints
    rows = [nc - 1, 20000, 700, 701, 12345, 31000]
    assert check_against_model(gm_ctx, cname, with_qc(k, rows), k.witness) == sorted(rows)
    assert len(check_against_model(gm_ctx, cname, k, [0] * k.nb_wires)) == nc - 3


# ---------------------------------------------------------------------------
# 5. refusals: each is followed by a correct call on the same context
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("cname", CURVES)
def test_refusals(gm_ctx, oracle, cname):
    import gnark_mi355x as gm
    n, nb = 64, 2
    k, inst = key_case(cname, n, nb)
    c = k.c
    nc = k.nb_constraints
    _, can, _, _ = srs(oracle, cname, n)
    pb = gm.point_bytes(cname, False)
    L = gm.load_library()

    def bad_record(i, field, value):
        rec = k.records.copy()
        rec[i, field] = value
        return dict(records=rec)

    # 1. the upload
    assert "record 9: XB = %d" % k.nb_wires in refused(upload, gm_ctx, cname, k, **bad_record(9, model.XB, k.nb_wires))
    assert "record 0: XA" in refused(upload, gm_ctx, cname, k, **bad_record(0, model.XA, 2**32 - 1))
    assert "record 61: QM = 9" in refused(upload, gm_ctx, cname, k, **bad_record(61, model.QM, len(k.coeffs)))
    assert "record 3: QC" in refused(upload, gm_ctx, cname, k, **bad_record(3, model.QC, 1000))
    assert "record 7: Commitment = 3" in refused(upload, gm_ctx, cname, k, **bad_record(7, model.COMMITMENT, 3))
    for over in (dict(n=48), dict(n=4), dict(n=32), dict(nb_public=3), dict(nb_wires=0), dict(nb_wires=1),
                 dict(nb_wires=2**32), dict(ncoeffs=1), dict(records=None, nb_constraints=nc), dict(coeffs=None),
                 dict(committed=[[nc], [0]]), dict(commitment_index=[1, nc]),
                 dict(committed=[[0]] * 1025, commitment_index=[0] * 1025)):
        refused(upload, gm_ctx, cname, k, **over)

    circ = upload(gm_ctx, cname, k)
    other_ctx = gm.Context(0)
    foreign = upload(other_ctx, cname, k)
    buf = gm_ctx.malloc(32 * n + 16)
    keys = []
    try:
        want = columns(k)
        # 2. the selectors
        refused(circ.selector, gm.SCS_QCP0 + nb, buf)
        with pytest.raises(gm.GmError):  # a circuit of another context
            gm._check(L.gm_plonk_scs_selector(gm_ctx.handle, foreign.handle, 0, buf.ptr))
        refused(circ.selector, 0, gm.DeviceBuffer(gm_ctx, buf.ptr + 8, 32 * n))
        assert circ.selector(gm.SCS_QCP0 + nb - 1, buf).to_host(32 * n) == want[-1].tobytes()
        # 3. the key
        refused(gm.PlonkProvingKey.setup_from_circuit, circ, can, digests=False)
        refused(gm.PlonkProvingKey.setup_from_circuit, circ, can, srs_canonical_len=n + 2)
        refused(gm.PlonkProvingKey.setup_from_circuit, circ, None)
        with pytest.raises(gm.GmError):  # a circuit of another context
            gm._check(L.gm_plonk_pk_setup_scs(gm_ctx.handle, foreign.handle, gm._p(gm._buf(can)), len(can) // pb, 0,
                                              ctypes.byref(ctypes.c_void_p()),
                                              gm._p(np.zeros(pb * (8 + nb), np.uint8)), None))
        # 4. the check
        refused(circ.check, None)
        with pytest.raises(gm.GmError):
            sz = ctypes.c_size_t()
            gm._check(L.gm_plonk_scs_check(gm_ctx.handle, foreign.handle, gm._p(gm._buf(enc(c, [0] * k.nb_wires))),
                                           ctypes.byref(sz), ctypes.byref(sz)))
        # the borrowed tables are not freed on their own, and the circuit goes on working
        w = circ.wires()
        assert "belong to a circuit" in refused(w.free)
        gm_ctx.trim()
        assert np.array_equal(read_tables(gm_ctx, circ), model.tables(k.records, n, k.nb_public))
        assert circ.selector(gm.SCS_QL, buf).to_host(32 * n) == want[0].tobytes()
        gm_ctx.trim()
        # after every refusal: a right circuit and a right key on the same context
        again = upload(gm_ctx, cname, k)
        try:
            key, digests, _ = gm.PlonkProvingKey.setup_from_circuit(again, can)
            keys.append(key)
        finally:
            again.free()
        ref, ref_digests, _ = reference_key(gm_ctx, oracle, cname, k)
        keys.append(ref)
        assert digests == ref_digests
        assert_same(run_proof(key, inst, False), run_proof(ref, inst, False))
    finally:
        buf.free()
        circ.free()
        foreign.free()
        other_ctx.close()
        for key in keys:
            key.free()
