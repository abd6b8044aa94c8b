"""gm_plonk_wires_* / gm_plonk_gather_lro / gm_plonk_session_round1_witness /
gm_plonk_session_bsb22_sparse: a PLONK session that starts from the solver's
values, with the circuit's wire tables resident on the device.

The gather moves 32-byte words untouched, so it is checked element-wise against
a numpy fancy-index of the same bytes.  For whole proofs the reference is the
existing path (round1 from host-gathered l, r, o, dense bsb22), which
test_plonk_session_gpu.py pins to an integer model: every output of all five
rounds must be the same bytes.  Instances, keys, challenges and the proof loop
are that module's.
"""
import random

import numpy as np
import pytest

import pyref
import test_plonk_session_gpu as ps
from test_plonk_session_gpu import NB_PUBLIC, assert_same, challenge, enc, make_key, run_proof

pytestmark = pytest.mark.gpu

CURVES = ps.CURVES


# ---------------------------------------------------------------------------
# helpers
# ---------------------------------------------------------------------------
def refused(f, *a, **kw):
    import gnark_mi355x as gm
    with pytest.raises(gm.GmError) as e:
        f(*a, **kw)
    assert "error -1: plonk" in str(e.value), str(e.value)
    return str(e.value)


def tables(n, nb_wires, seed):
    """Random wire tables in evaluateLROSmallDomain's convention: placeholder rows
    (i, 0, 0) for the public inputs, padding rows (0, 0, 0) at the end; ids 0 and
    nb_wires - 1 both occur."""
    rng = np.random.default_rng(seed)
    t = rng.integers(0, nb_wires, size=(3, n), dtype=np.uint32)
    pub = min(NB_PUBLIC, nb_wires)
    t[0, :pub] = np.arange(pub)
    t[1:, :pub] = 0
    t[:, n - 2:] = 0
    t[0, pub], t[1, pub + 1], t[2, pub + 2] = nb_wires - 1, 0, nb_wires - 1
    return t


def witness_case(cname, n, nb, nb_wires, seed):
    """An instance whose l, r, o are the gather of a random witness through random
    tables, whose public inputs are the witness' first elements and whose
    committed-values vectors are zero but on a few (unsorted) rows."""
    c = pyref.CURVES[cname]
    inst = ps.Inst(c, n, nb, seed)
    rng = random.Random(seed ^ 0x9100)
    t = tables(n, nb_wires, seed)
    wit = [rng.randrange(c.r) for _ in range(nb_wires)]
    inst.tables, inst.nb_wires, inst.witness = t, nb_wires, enc(c, wit)
    inst.public = wit[:NB_PUBLIC]
    inst.w = {k: [wit[i] for i in t[j]] for j, k in enumerate(("l", "r", "o"))}
    # host L, R, O by numpy, on the bytes the device sees
    W = np.frombuffer(inst.witness, np.uint8).reshape(nb_wires, 32)
    for j, k in enumerate(("l", "r", "o")):
        assert W[t[j]].tobytes() == enc(c, inst.w[k])
    inst.sparse = []
    for j in range(nb):
        rows = rng.sample(range(n), 5)
        vals = [rng.randrange(1, c.r) for _ in rows]
        set_sparse(inst, j, rows, vals)
    return inst


def set_sparse(inst, j, rows, vals):
    vec = [0] * inst.n
    for row, v in zip(rows, vals):
        vec[row] = v
    inst.pi2[j] = vec
    while len(inst.sparse) <= j:
        inst.sparse.append(None)
    inst.sparse[j] = (list(rows), list(vals))


def make_wires(ctx, inst):
    import gnark_mi355x as gm
    return gm.PlonkWires(ctx, inst.n, inst.nb_wires, *inst.tables)


def finish(s, inst, out):
    """Rounds 2 to 5 as ps.run_proof runs them."""
    c = inst.c
    e1 = lambda v: enc(c, [v])
    beta = challenge(c, "beta", inst.salt, *out["bsb"], *out["lro"])
    gamma = challenge(c, "gamma", inst.salt, *out["bsb"], *out["lro"])
    out["z"] = s.round2(e1(beta), e1(gamma))
    out["h"] = s.round3(e1(challenge(c, "alpha", out["z"])))
    out["lin"], out["claimed"], out["z_shifted"], out["z_open"] = s.round4(e1(challenge(c, "zeta", *out["h"])))
    out["batch"] = s.round5(e1(challenge(c, "kzg", out["lin"], *out["claimed"], out["z_shifted"], out["z_open"])))
    return out


def witness_args(inst, h_rand):
    c = inst.c
    return dict(blinds={k: enc(c, v) for k, v in inst.b.items()},
                commitment_vals=enc(c, inst.cvals) if inst.nb else None,
                h_rand=enc(c, inst.h_rand) if h_rand else None)


def run_proof_witness(key, wires, inst, h_rand):
    """A whole proof through bsb22_sparse and round1_witness."""
    c = inst.c
    s = key.session()
    try:
        out = {"bsb": [s.bsb22_sparse(j, rows, enc(c, vals)) for j, (rows, vals) in enumerate(inst.sparse)]}
        out["lro"] = s.round1_witness(wires, inst.witness, **witness_args(inst, h_rand))
        return finish(s, inst, out)
    finally:
        s.free()


# ---------------------------------------------------------------------------
# 1. the gather, element-wise
# ---------------------------------------------------------------------------
def gather_check(ctx, n, nb_wires, t, seed, bufs=None):
    import gnark_mi355x as gm
    W = np.random.default_rng(seed).integers(0, 256, size=(nb_wires, 32), dtype=np.uint8)
    wires = gm.PlonkWires(ctx, n, nb_wires, *t)
    wit = ctx.copy_to_device(W)
    out = bufs or [ctx.malloc(32 * n) for _ in range(3)]
    try:
        assert wires.resident_bytes() == 12 * n
        wires.gather(wit, *out)
        for k in range(3):
            got = np.frombuffer(out[k].to_host(32 * n), np.uint8).reshape(n, 32)
            assert np.array_equal(got, W[t[k]]), "lro"[k]
    finally:
        wires.free()
        wit.free()
        if not bufs:
            for b in out:
                b.free()


# 2^19: the first size at which a lane takes more than one turn of the grid-stride loop
@pytest.mark.parametrize("n,wires_of", [(8, (1, 4, 8, 24)), (1024, (1, 512, 1024, 3072)),
                                        (1 << 15, (1, 1 << 14, 1 << 15, 3 << 15)), (1 << 19, (1 << 18,))])
def test_gather_random_tables(gm_ctx, n, wires_of):
    for nb_wires in wires_of:
        t = tables(n, nb_wires, 0x9000 + n + nb_wires)
        if nb_wires > 1:
            assert t.min() == 0 and t.max() == nb_wires - 1
        gather_check(gm_ctx, n, nb_wires, t, n ^ nb_wires)


@pytest.mark.parametrize("n", [8, 1024, 1 << 15])
def test_gather_special_tables(gm_ctx, n):
    rng = np.random.default_rng(0x9001 + n)
    # every row at the same wire (the last one)
    gather_check(gm_ctx, n, n // 2, np.full((3, n), n // 2 - 1, np.uint32), 1)
    # a permutation per table
    gather_check(gm_ctx, n, n, np.stack([rng.permutation(n) for _ in range(3)]).astype(np.uint32), 2)
    # xa = xb = xc
    one = rng.integers(0, 3 * n, size=n, dtype=np.uint32)
    gather_check(gm_ctx, n, 3 * n, np.stack([one, one, one]), 3)


def test_gather_after_a_larger_call_writes_its_rows_only(gm_ctx):
    """The same output buffers after a larger gather: the small call's rows are
    right and nothing behind them is written."""
    big, n = 1 << 15, 8
    bufs = [gm_ctx.malloc(32 * big) for _ in range(3)]
    try:
        gather_check(gm_ctx, big, big, tables(big, big, 0x9002), 4, bufs)
        before = [b.to_host() for b in bufs]
        gather_check(gm_ctx, n, 3 * n, tables(n, 3 * n, 0x9003), 5, bufs)
        for b, old in zip(bufs, before):
            now = b.to_host()
            assert now[32 * n:] == old[32 * n:] and now[:32 * n] != old[:32 * n]
    finally:
        for b in bufs:
            b.free()


# ---------------------------------------------------------------------------
# 2. whole proofs: witness path = existing path, byte for byte
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("h_rand", [False, True])
@pytest.mark.parametrize("nb", [0, 2])
@pytest.mark.parametrize("n", [8, 64, 1024])
@pytest.mark.parametrize("cname", CURVES)
def test_whole_proof_from_the_witness_equals_the_existing_path(gm_ctx, oracle, cname, n, nb, h_rand):
    # fewer wires than rows with h_rand, more without
    nb_wires = n // 2 if h_rand else n + n // 2 + 3
    inst = witness_case(cname, n, nb, nb_wires, 0x9200 + 16 * n + nb)
    key = make_key(gm_ctx, oracle, cname, inst)
    wires = make_wires(gm_ctx, inst)
    try:
        want = run_proof(key, inst, h_rand)
        assert_same(run_proof_witness(key, wires, inst, h_rand), want)
    finally:
        wires.free()
        key.free()


# ---------------------------------------------------------------------------
# 3. the sparse bsb22 input at its edges
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["empty and single", "ends and unsorted"])
@pytest.mark.parametrize("cname", CURVES)
def test_sparse_bsb22_edges(gm_ctx, oracle, cname, which):
    n, nb = 64, 2
    inst = witness_case(cname, n, nb, n, 0x9300)
    r = inst.c.r
    if which == "empty and single":
        set_sparse(inst, 0, [], [])
        set_sparse(inst, 1, [17], [r - 1])
    else:
        set_sparse(inst, 0, [n - 1, 0], [5, r - 2])
        set_sparse(inst, 1, [40, 3, 63, 0, 22, 21], [1, 2, 3, 4, 5, 6])
    key = make_key(gm_ctx, oracle, cname, inst)
    wires = make_wires(gm_ctx, inst)
    try:
        want = run_proof(key, inst, True)
        got = run_proof_witness(key, wires, inst, True)
        assert_same(got, want)
        if which == "empty and single":
            # the commit of the zero vector is the point at infinity
            assert not any(got["bsb"][0])
    finally:
        wires.free()
        key.free()


# ---------------------------------------------------------------------------
# 4. one table object, many sessions; the key is never written
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("cname", CURVES)
def test_wires_reused_across_sessions_and_trim(gm_ctx, oracle, cname):
    n, nb = 64, 2
    inst = witness_case(cname, n, nb, n + 7, 0x9400)
    key = make_key(gm_ctx, oracle, cname, inst)
    resident = key.resident_bytes()
    wires = make_wires(gm_ctx, inst)
    try:
        assert key.resident_bytes() == resident and wires.resident_bytes() == 12 * n
        want = run_proof(key, inst, True)
        for _ in range(3):
            assert_same(run_proof_witness(key, wires, inst, True), want)
        gm_ctx.trim()
        assert_same(run_proof_witness(key, wires, inst, True), want)
        # both kinds of session interleaved on the key, also one that ends early
        assert run_proof(key, inst, True, upto=1)["lro"] == want["lro"]
        assert_same(run_proof_witness(key, wires, inst, True), want)
        assert_same(run_proof(key, inst, True), want)
        plain = run_proof(key, inst, False)
        assert_same(run_proof_witness(key, wires, inst, False), plain)
        assert key.resident_bytes() == resident
    finally:
        wires.free()
        key.free()


# ---------------------------------------------------------------------------
# 5. refusals: each leaves the session able to finish a correct proof
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("cname", CURVES)
def test_refusals(gm_ctx, oracle, cname):
    import gnark_mi355x as gm
    n, nb = 64, 2
    inst = witness_case(cname, n, nb, n, 0x9500)
    c = inst.c
    t = inst.tables
    one = enc(c, [1])

    # uploads
    bad = t.copy()
    bad[1, 9] = n
    assert "xb[9] = %d" % n in refused(gm.PlonkWires, gm_ctx, n, n, *bad)
    refused(gm.PlonkWires, gm_ctx, n, 0, *t)
    refused(gm.PlonkWires, gm_ctx, n, n, t[0], None, t[2])
    refused(gm.PlonkWires, gm_ctx, 4, n, *t[:, :4])

    key = make_key(gm_ctx, oracle, cname, inst)
    want = run_proof(key, inst, False)
    wires = make_wires(gm_ctx, inst)
    half = gm.PlonkWires(gm_ctx, n // 2, n, *t[:, :n // 2])  # another n than the key
    few = gm.PlonkWires(gm_ctx, n, 1, *np.zeros((3, n), np.uint32))  # fewer wires than public inputs
    other_ctx = gm.Context(0)
    foreign = gm.PlonkWires(other_ctx, n, n, *t)
    s = key.session()
    try:
        args = witness_args(inst, False)
        sparse = [(rows, enc(c, vals)) for rows, vals in inst.sparse]
        # before the bsb22 calls
        refused(s.round1_witness, wires, inst.witness, **args)
        refused(s.bsb22_sparse, nb, *sparse[0])
        refused(s.bsb22_sparse, 0, [3, 9, 3], enc(c, [1, 2, 3]))  # a duplicate row
        refused(s.bsb22_sparse, 0, [3, n], enc(c, [1, 2]))  # a row outside the domain
        refused(s.bsb22_sparse, 0, list(range(n)) + [0], enc(c, [1] * (n + 1)))  # count > n
        refused(s.bsb22_sparse, 0, [3], None)
        got = {"bsb": [s.bsb22_sparse(0, *sparse[0])]}
        refused(s.round1_witness, wires, inst.witness, **args)  # one of two
        got["bsb"].append(s.bsb22_sparse(1, *sparse[1]))
        # round 1 from the witness
        refused(s.round2, one, one)
        refused(s.round1_witness, half, inst.witness, **args)
        refused(s.round1_witness, few, inst.witness, **args)
        refused(s.round1_witness, foreign, inst.witness, **args)
        refused(s.round1_witness, None, inst.witness, **args)
        refused(s.round1_witness, wires, None, **args)
        refused(s.round1_witness, wires, inst.witness, **dict(args, commitment_vals=None))
        refused(s.round1_witness, wires, inst.witness, **dict(args, blinds=dict(args["blinds"], bz=None)))
        got["lro"] = s.round1_witness(wires, inst.witness, **args)
        # after round 1
        refused(s.bsb22_sparse, 0, *sparse[0])
        refused(s.round1_witness, wires, inst.witness, **args)
        refused(s.round3, one)
        # the session that met every refusal made the existing path's proof
        assert_same(finish(s, inst, got), want)
        refused(s.round1_witness, wires, inst.witness, **args)
    finally:
        s.free()
        for w in (wires, half, few, foreign):
            w.free()
        other_ctx.close()
        key.free()


def test_gather_refusals(gm_ctx):
    import gnark_mi355x as gm
    n = 64
    t = tables(n, n, 0x9600)
    W = np.random.default_rng(6).integers(0, 256, size=(n, 32), dtype=np.uint8)
    wires = gm.PlonkWires(gm_ctx, n, n, *t)
    wit = gm_ctx.copy_to_device(W)
    out = [gm_ctx.malloc(32 * n) for _ in range(3)]
    view = lambda b, off: gm.DeviceBuffer(gm_ctx, b.ptr + off, b.nbytes - off)
    other_ctx = gm.Context(0)
    try:
        refused(wires.gather, wit, out[0], out[1], wit)  # an output is the witness
        refused(wires.gather, wit, view(wit, 32 * (n - 1)), out[1], out[2])  # an output begins in its last element
        refused(wires.gather, view(out[2], 32 * (n - 1)), out[0], out[1], view(out[2], 0))
        refused(wires.gather, wit, out[0], out[0], out[2])  # two outputs overlap
        refused(wires.gather, wit, view(out[0], 8), out[1], out[2])  # not 16-byte aligned
        foreign = gm.PlonkWires(other_ctx, n, n, *t)
        try:
            with pytest.raises(gm.GmError):
                gm._check(gm.load_library().gm_plonk_gather_lro(gm_ctx.handle, foreign.handle, wit.ptr,
                                                                 *[b.ptr for b in out]))
        finally:
            foreign.free()
        # the witness was not written, and the call still works
        assert wit.to_host() == W.tobytes()
        wires.gather(wit, *out)
        for k in range(3):
            assert out[k].to_host() == W[t[k]].tobytes()
    finally:
        other_ctx.close()
        wires.free()
        wit.free()
        for b in out:
            b.free()
