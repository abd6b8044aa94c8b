"""gm_kzg_srs_lagrange / gm_plonk_sigma / gm_plonk_pk_setup: the Lagrange SRS, S1-S3
and the resident key derived on the device from what gnark's Setup holds.

Expected values are integers: with a known tau the canonical SRS is [tau^j] G and
the Lagrange SRS [L_i(tau)] G, L_i(tau) = (tau^n - 1) w^i / (n (tau - w^i)), both
made by the oracle from integer scalars (test_plonk_session_gpu.srs); s_k[i] is
g^(S / n) w^(S mod n) in Python integers; a digest is [sum_i v_i L_i(tau)] G.  A key
made by gm_plonk_pk_setup must prove like the uploaded one: the same bytes in
every round.
"""
import functools
import random

import numpy as np
import pytest

import pyref
import test_plonk_witness_gpu as pw
from test_plonk_session_gpu import NB_PUBLIC, Inst, assert_same, enc, make_key, point, run_proof, srs

pytestmark = pytest.mark.gpu

CURVES = ("bn254", "bls12377")


def pbytes(cname):
    import gnark_mi355x as gm
    return gm.point_bytes(cname, False)


def points(b, pb):
    return [b[i:i + pb] for i in range(0, len(b), pb)]


def lagrange(ctx, cname, src, n, in_place=False):
    """gm_kzg_srs_lagrange on host bytes; (result bytes, input bytes afterwards)."""
    pb = pbytes(cname)
    a = ctx.copy_to_device(src[:n * pb])
    out = None
    try:
        out = ctx.kzg_srs_lagrange(cname, a, n, a if in_place else None)
        return out.to_host(), a.to_host()
    finally:
        a.free()
        if out is not None and not in_place:
            out.free()


# ---------------------------------------------------------------------------
# 1. known tau
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("n", [2, 4, 8, 64, 1024, 4096])
@pytest.mark.parametrize("cname", CURVES)
def test_known_tau(gm_ctx, oracle, cname, n):
    _, can, lag, _ = srs(oracle, cname, n)
    got, _ = lagrange(gm_ctx, cname, can, n)
    pb = pbytes(cname)
    bad = [i for i, (a, b) in enumerate(zip(points(got, pb), points(lag, pb))) if a != b]
    assert not bad, (len(bad), bad[:8])
    assert len(got) == n * pb


# ---------------------------------------------------------------------------
# 2. degenerate inputs: doublings, cancellations and infinities in the butterflies
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("n", [8, 64])
@pytest.mark.parametrize("cname", CURVES)
def test_degenerate_inputs(gm_ctx, oracle, cname, n):
    import gnark_mi355x as gm
    c = pyref.CURVES[cname]
    r, pb = c.r, pbytes(cname)
    g, inf = gm.generator(cname), bytes(pb)
    w = pyref.domain_generator(c, n)

    def unit(k):
        return b"".join(g if i == k else inf for i in range(n))

    # tau = 1: every input is G; the first stage is all doublings and all infinities
    got, _ = lagrange(gm_ctx, cname, g * n, n)
    assert got == unit(0)
    # tau = w^k: L_i(tau) is 1 at i = k and 0 elsewhere
    for k in (1, n // 2, n - 1):
        src = oracle.batch_mul_base(cname, False, g, enc(c, [pow(w, k * j, r) for j in range(n)]))
        got, _ = lagrange(gm_ctx, cname, src, n)
        assert got == unit(k), k
    # tau = 0: G followed by infinities; every output is [1/n] G
    got, _ = lagrange(gm_ctx, cname, g + inf * (n - 1), n)
    assert got == point(oracle, cname, pow(n, -1, r)) * n


# ---------------------------------------------------------------------------
# 3. in place against out of place
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("cname", CURVES)
def test_in_place_and_overlap(gm_ctx, oracle, cname):
    import gnark_mi355x as gm
    n = 64
    _, can, lag, _ = srs(oracle, cname, n)
    pb = pbytes(cname)
    src = can[:n * pb]
    out, after = lagrange(gm_ctx, cname, src, n)
    assert after == src  # out of place leaves the input unchanged
    inp, _ = lagrange(gm_ctx, cname, src, n, in_place=True)
    assert inp == out == lag
    # a partial overlap, from either side
    buf = gm_ctx.copy_to_device(src + bytes(pb))
    try:
        lo = gm.DeviceBuffer(gm_ctx, buf.ptr, n * pb)
        hi = gm.DeviceBuffer(gm_ctx, buf.ptr + pb, n * pb)
        for a, b in ((lo, hi), (hi, lo)):
            with pytest.raises(gm.GmError) as e:
                gm_ctx.kzg_srs_lagrange(cname, a, n, b)
            assert "error -1: kzg srs lagrange" in str(e.value) and "overlaps" in str(e.value)
        assert buf.to_host(n * pb) == src
        # n out of range
        for m in (0, 1, 48):
            with pytest.raises(gm.GmError) as e:
                gm_ctx.kzg_srs_lagrange(cname, lo, m, lo)
            assert "error -1" in str(e.value)
        assert buf.to_host(n * pb) == src
    finally:
        buf.free()


# ---------------------------------------------------------------------------
# 4. S1, S2, S3
# ---------------------------------------------------------------------------
def sigma_model(c, n, perm):
    """s[t] = g^(S / n) w^(S mod n), S = perm[t]."""
    r, g, w = c.r, c.coset_gen, pyref.domain_generator(c, n)
    ids, wi = [], 1
    for _ in range(n):
        ids.append(wi)
        wi = wi * w % r
    ids = ids + [g * x % r for x in ids] + [g * g * x % r for x in ids]
    return [ids[s] for s in perm]


def random_permutation(n, seed):
    """A permutation of [0, 3n) that maps row 0 to 3n - 1 and contains 0, n - 1 and n
    away from their own places."""
    rng = random.Random(seed)
    perm = list(range(3 * n))
    rng.shuffle(perm)
    for want, at in ((0, 5), (n - 1, 1), (n, 2 * n + 3), (3 * n - 1, 0)):
        i = perm.index(want)
        perm[i], perm[at] = perm[at], perm[i]
    assert sorted(perm) == list(range(3 * n))
    return perm


def build_permutation(t, nb_wires):
    """gnark's buildPermutation (setup.go:271-325) on complete wire tables: each
    position points to the previous position of the same wire, the first one to the
    last."""
    lro = [int(x) for row in t for x in row]
    perm, cycle = [-1] * len(lro), [-1] * nb_wires
    for i, v in enumerate(lro):
        if cycle[v] != -1:
            perm[i] = cycle[v]
        cycle[v] = i
    for i, v in enumerate(lro):
        if perm[i] == -1:
            perm[i] = cycle[v]
    return perm


def sigma(ctx, cname, n, perm):
    bufs = ctx.plonk_sigma(cname, n, perm)
    try:
        return b"".join(b.to_host() for b in bufs)
    finally:
        for b in bufs:
            b.free()


@pytest.mark.parametrize("n", [8, 64, 1024])
@pytest.mark.parametrize("cname", CURVES)
def test_sigma(gm_ctx, cname, n):
    import gnark_mi355x as gm
    c = pyref.CURVES[cname]
    perm = random_permutation(n, 0x9300 + n)
    assert sigma(gm_ctx, cname, n, perm) == enc(c, sigma_model(c, n, perm))
    nb_wires = n // 2 + 3
    built = build_permutation(pw.tables(n, nb_wires, 0x9310 + n), nb_wires)
    assert sorted(built) == list(range(3 * n)) and built != list(range(3 * n))
    assert sigma(gm_ctx, cname, n, np.array(built, np.int64)) == enc(c, sigma_model(c, n, built))
    for bad, row in ((-1, 2 * n + 1), (3 * n, n - 1)):
        p = list(perm)
        p[row] = bad
        p[row + 1] = -7  # a later offender: the first one is named
        with pytest.raises(gm.GmError) as e:
            gm_ctx.plonk_sigma(cname, n, p)
        assert "error -1: plonk setup: permutation[%d] = %d " % (row, bad) in str(e.value), str(e.value)


# ---------------------------------------------------------------------------
# 5. a key from gm_plonk_pk_setup against the uploaded key
# ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def setup_case(cname, n, nb):
    """A random instance whose s1, s2, s3 are the integer model of a random permutation."""
    c = pyref.CURVES[cname]
    inst = Inst(c, n, nb, 0x9400 + 16 * n + nb)
    inst.perm = random_permutation(n, 0x9500 + n + nb)
    s = sigma_model(c, n, inst.perm)
    inst.fixed.update(s1=s[:n], s2=s[n:2 * n], s3=s[2 * n:])
    return inst


def setup_key(ctx, oracle, cname, inst, cache=True, **over):
    import gnark_mi355x as gm
    c = inst.c
    _, can, _, _ = srs(oracle, cname, inst.n)
    a = dict(n=inst.n, nb_public=NB_PUBLIC, polys={k: enc(c, inst.fixed[k]) for k in gm.PLONK_SETUP_POLYS},
             permutation=inst.perm, qcp=[enc(c, f) for f in inst.qcp], commitment_row=list(inst.rows),
             srs_canonical=can, cache=cache, lagrange=True)
    a.update(over)
    return gm.PlonkProvingKey.setup(ctx, cname, **a)


def check_setup_against_upload(gm_ctx, oracle, cname, n, nb, cache):
    inst = setup_case(cname, n, nb)
    c, r = inst.c, inst.c.r
    _, _, lag, lag_int = srs(oracle, cname, n)
    key, digests, lag_out = setup_key(gm_ctx, oracle, cname, inst, cache=cache)
    up = None
    try:
        assert lag_out == lag
        order = [inst.fixed[k] for k in ("s1", "s2", "s3", "ql", "qr", "qm", "qo", "qk")] + inst.qcp
        assert len(digests) == 8 + nb
        for j, (d, v) in enumerate(zip(digests, order)):
            assert d == point(oracle, cname, sum(a * b for a, b in zip(v, lag_int)) % r), j
        up = make_key(gm_ctx, oracle, cname, inst, cache=cache)
        assert key.resident_bytes() == up.resident_bytes()
        assert (key.resident_bytes()[1] == 0) == (not cache)
        assert_same(run_proof(key, inst, True), run_proof(up, inst, True))
    finally:
        key.free()
        if up is not None:
            up.free()


@pytest.mark.parametrize("nb", [0, 2])
@pytest.mark.parametrize("n", [8, 64, 1024])
@pytest.mark.parametrize("cname", CURVES)
def test_setup_against_upload(gm_ctx, oracle, cname, n, nb):
    check_setup_against_upload(gm_ctx, oracle, cname, n, nb, True)


@pytest.mark.parametrize("cname", CURVES)
def test_setup_against_upload_without_the_coset_cache(gm_ctx, oracle, cname):
    check_setup_against_upload(gm_ctx, oracle, cname, 64, 2, False)


# ---------------------------------------------------------------------------
# 6. refusals: each leaves the context able to make a key
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("cname", CURVES)
def test_refusals(gm_ctx, oracle, cname):
    import gnark_mi355x as gm
    n, nb = 64, 2
    inst = setup_case(cname, n, nb)
    c = inst.c
    fixed = {k: enc(c, inst.fixed[k]) for k in gm.PLONK_SETUP_POLYS}
    low, high = list(inst.perm), list(inst.perm)
    low[7], high[2 * n] = -1, 3 * n
    for name, over in {
        "n = 48": dict(n=48, permutation=inst.perm[:3 * 48]),
        "n = 4": dict(n=4, permutation=list(range(12))),
        "short canonical SRS": dict(srs_canonical_len=n + 2),
        "commitment row = n": dict(commitment_row=[3, n]),
        "null ql": dict(polys=dict(fixed, ql=None)),
        "null qk": dict(polys=dict(fixed, qk=None)),
        "null canonical SRS": dict(srs_canonical=None, srs_canonical_len=n + 3),
        "null qcp table": dict(qcp=None),
        "null qcp entry": dict(qcp=[enc(c, inst.qcp[0]), None]),
        "null permutation": dict(permutation=None),
        "null vk_digests": dict(digests=False),
        "permutation entry -1": dict(permutation=low),
        "permutation entry 3n": dict(permutation=high),
    }.items():
        with pytest.raises(gm.GmError) as e:
            setup_key(gm_ctx, oracle, cname, inst, **over)
        assert "error -1: plonk" in str(e.value), (name, str(e.value))
        if name.startswith("permutation entry"):
            assert "permutation[%d]" % (7 if over["permutation"] is low else 2 * n) in str(e.value)
    L = gm.load_library()
    h = gm._PlonkSetupHost()
    assert L.gm_plonk_pk_setup(gm_ctx.handle, gm.curve_id(cname), h, 2, None, None, None) == -1
    key, digests, _ = setup_key(gm_ctx, oracle, cname, inst, lagrange=False)
    try:
        assert len(digests) == 8 + nb and key.resident_bytes()[1] == 4 * (8 + nb) * n * 32
    finally:
        key.free()
