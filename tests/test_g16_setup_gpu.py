"""gm_g16_setup (R1CS.g16_setup): gnark's Setup from the resident constraint system.
Every array and both infinity masks byte for byte against the C++ oracle on the
circuits the other Groth16 tests use and on one whose ONE wire sits in every row
(all three column classes); against Python integers on small random systems
with every special CoeffTable id, empty rows, unused wires and a wire whose two
A terms cancel exactly; the BSB22 split of K; a proof from the derived key; and
every refusal, after which the same context still derives the right key."""
import random

import numpy as np
import pytest

import gnark_mi355x as gm
import pyref
import r1cs as R

pytestmark = pytest.mark.gpu

TOXIC = (0x1234567, 0x89ABCDEF1, 0x314159265, 0x271828182, 0x161803398)
ORACLE_KEYS = ("g1_alpha", "g1_beta", "g1_delta", "g1_A", "g1_B", "g1_Z", "g1_K", "g2_beta", "g2_delta", "g2_B",
               "infA", "infB")


def upload(ctx, r1):
    return gm.R1CS.from_terms(ctx, r1.curve, r1.nc, r1.nb_wires, r1.rowptr, r1.wires, r1.coeffs, r1.c.r)


def toxic_bytes(cname, vals=TOXIC):
    return R.encode_vec(cname, [t % pyref.CURVES[cname].r for t in vals])


def lagrange_at(c, n, t):
    """[L_j(t)] for j < n in Python integers."""
    r = c.r
    w = pyref.domain_generator(c, n) if n > 1 else 1
    tn1 = (pow(t, n, r) - 1) % r
    ninv = pow(n, -1, r)
    return [pow(w, j, r) * tn1 * ninv * pow((t - pow(w, j, r)) % r, -1, r) % r for j in range(n)]


def abc_ints(r1, t):
    c, r = r1.c, r1.c.r
    lag = lagrange_at(c, r1.domain_size, t % r)
    A, B, C = ([0] * r1.nb_wires for _ in range(3))
    for j, con in enumerate(r1.cons):
        for dst, terms in zip((A, B, C), con):
            for w, co in terms:
                dst[w] = (dst[w] + co * lag[j]) % r
    return A, B, C


def assert_matches_oracle(got, want):
    for k in ORACLE_KEYS:
        assert bytes(got[k]) == bytes(want[k]), k


def check_gamma_side(oracle, cname, r1, got, toxic, gamma_wires=()):
    """g2_gamma and g1_K_gamma against Python integers multiplied by the oracle."""
    c = r1.c
    t, alpha, beta, gamma, delta = (x % c.r for x in toxic)
    assert got["g2_gamma"] == oracle.batch_mul_base(cname, True, gm.generator(cname, True), R.encode_vec(cname, [gamma]))
    A, B, C = abc_ints(r1, t)
    ginv = pow(gamma, -1, c.r)
    wires = list(range(r1.nb_public)) + list(gamma_wires)
    ks = [(beta * A[w] + alpha * B[w] + C[w]) * ginv % c.r for w in wires]
    assert got["g1_K_gamma"] == oracle.batch_mul_base(cname, False, gm.generator(cname), R.encode_vec(cname, ks))


def ones_everywhere(cname, nc=1 << 15):
    """Wire 0 in L of every row (a column as long as the circuit), wire 1 in L of the
    first 100 rows and 50 wires in ~nc/50 rows of L and R each (one block per
    column), the rest short."""
    cons = []
    for j in range(nc):
        L = [(0, 1)] + ([(1, 3)] if j < 100 else []) + [(2 + j % 50, 2)]
        cons.append((L, [(2 + j % 50, 1)], [(52 + j % 7, 1), (59 + j, 5)] if j < 20 else [(52 + j % 7, 1)]))
    return R.R1CS(cname, nb_public=2, nb_wires=80, constraints=cons)


CIRCUITS = {
    "cubic": lambda cn: R.cubic_circuit(cn)[0],
    "chain1": lambda cn: R.squaring_chain(1, cn)[0],
    "chain300": lambda cn: R.squaring_chain(300, cn)[0],
    "chain1023": lambda cn: R.squaring_chain(1023, cn)[0],
    "chain1024": lambda cn: R.squaring_chain(1024, cn)[0],
}


@pytest.mark.parametrize("name", list(CIRCUITS))
@pytest.mark.parametrize("cname", ["bn254", "bls12377"])
def test_against_the_oracle(gm_ctx, oracle, cname, name):
    r1 = CIRCUITS[name](cname)
    tox = toxic_bytes(cname)
    want = oracle.g16_setup(cname, r1, tox)
    h = upload(gm_ctx, r1)
    try:
        assert h.g16_setup_sizes(tox, r1.nb_public) == (r1.nbA, r1.nbB, r1.nb_wires - r1.nb_public)
        got = h.g16_setup(tox, r1.nb_public)
    finally:
        h.free()
    assert_matches_oracle(got, want)
    assert got["k_wires"] == list(range(r1.nb_public, r1.nb_wires))
    if name in ("cubic", "chain300"):
        check_gamma_side(oracle, cname, r1, got, TOXIC)


@pytest.mark.parametrize("cname", ["bn254", "bls12377"])
def test_all_three_column_classes(gm_ctx, oracle, cname):
    """The ONE wire's column is split over several blocks at the forced cut and at
    the default one; wire 1 and the R columns take one block; the rest one lane."""
    r1 = ones_everywhere(cname)
    tox = toxic_bytes(cname)
    want = oracle.g16_setup(cname, r1, tox)
    h = upload(gm_ctx, r1)
    try:
        for cut in (4096, 100, 0):
            gm_ctx.set_g16_setup_column_cut(cut)
            assert_matches_oracle(h.g16_setup(tox, r1.nb_public), want)
    finally:
        gm_ctx.set_g16_setup_column_cut(0)
        h.free()


def random_system(cname, seed, nc, nb_wires, nb_public):
    """Rows with every special CoeffTable id (0, 1, 2, -1, -2) and random
    coefficients, empty rows, wires that appear nowhere (the upper third), and wire
    `cancel` whose two A terms are L_j2(t) and -L_j1(t) in rows j1, j2."""
    c = pyref.CURVES[cname]
    rng = random.Random(f"g16 setup {cname} {seed}")
    special = [0, 1, 2, c.r - 1, c.r - 2]
    used = nb_wires * 2 // 3
    cancel = used - 1

    def row():
        k = rng.choice([0, 0, 1, 2, 3, 5])
        return [(rng.randrange(cancel), rng.choice(special + [rng.randrange(c.r)] * 3)) for _ in range(k)]

    cons = [(row(), row(), row()) for _ in range(nc)]
    n = 1
    while n < nc:
        n <<= 1
    lag = lagrange_at(c, n, TOXIC[0] % c.r)
    j1, j2 = 1, nc - 2
    cons[j1][0].append((cancel, lag[j2]))
    cons[j2][0].append((cancel, (c.r - lag[j1]) % c.r))
    cons[j1][1].append((cancel, 7))
    return R.R1CS(cname, nb_public, nb_wires, cons), cancel


@pytest.mark.parametrize("cname,nc,nb_wires", [("bn254", 64, 30), ("bn254", 37, 12), ("bls12377", 23, 18)])
def test_against_python_integers(gm_ctx, oracle, cname, nc, nb_wires):
    c = pyref.CURVES[cname]
    r1, cancel = random_system(cname, nc, nc, nb_wires, 3)
    want = pyref.g16_setup(c, r1.cons, r1.nb_wires, r1.nb_public, TOXIC)
    h = upload(gm_ctx, r1)
    try:
        got = h.g16_setup(toxic_bytes(cname), r1.nb_public)
    finally:
        h.free()
    assert want["infA"][cancel] and not want["infB"][cancel], "the wire appears, and its A terms cancel"
    assert any(want["infA"][w] and want["infB"][w] for w in range(nb_wires * 2 // 3, nb_wires))
    assert list(got["infA"]) == [int(x) for x in want["infA"]]
    assert list(got["infB"]) == [int(x) for x in want["infB"]]
    encp = lambda P, g2=False: pyref.encode_point(c, P, g2)
    for k in ("g1_alpha", "g1_beta", "g1_delta"):
        assert got[k] == encp(want[k]), k
    for k in ("g2_beta", "g2_delta"):
        assert got[k] == encp(want[k], True), k
    for k in ("g1_A", "g1_B", "g1_Z", "g1_K"):
        assert got[k] == b"".join(encp(P) for P in want[k]), k
    assert got["g2_B"] == b"".join(encp(P, True) for P in want["g2_B"])
    check_gamma_side(oracle, cname, r1, got, TOXIC)


def test_bsb22_split_of_k(gm_ctx, oracle):
    cname = "bn254"
    c = pyref.CURVES[cname]
    r1, info, _solve = R.commitment_chain(40, cname, ncommit=2)
    tox = [t % c.r for t in TOXIC]
    want = oracle.g16_setup_bsb22(cname, r1, info, tox, [0x31337, 0x4242])
    gamma_wires = sorted(set(w for ci in info for w in ci["private_committed"]) |
                         set(ci["commitment_index"] for ci in info))
    h = upload(gm_ctx, r1)
    try:
        got = h.g16_setup(toxic_bytes(cname), r1.nb_public, gamma_wires)
    finally:
        h.free()
    assert got["k_wires"] == list(want["k_wires"])
    assert got["g1_K"] == bytes(want["g1_K"])
    for k in ORACLE_KEYS:
        if k != "g1_K":
            assert bytes(got[k]) == bytes(want[k]), k
    check_gamma_side(oracle, cname, r1, got, TOXIC, gamma_wires)
    # the private committed entries are the Pedersen bases
    g1b = gm.point_bytes(cname, False)
    side = list(range(r1.nb_public)) + gamma_wires
    for i, ci in enumerate(info):
        basis = b"".join(got["g1_K_gamma"][g1b * side.index(w):g1b * (side.index(w) + 1)]
                         for w in ci["private_committed"])
        assert basis == want["ck"][i]["basis"], i


@pytest.mark.parametrize("cname", ["bn254", "bls12377"])
def test_the_derived_key_proves(gm_ctx, oracle, cname):
    r1, W = R.squaring_chain(300, cname, x=3)
    tox = toxic_bytes(cname)
    enc = lambda v: R.encode_vec(cname, v)
    a, b, cc = r1.solve_abc(W)
    rb, sb = enc([0x77777]), enc([0x99999])
    exp = oracle.g16_prove(cname, oracle.g16_setup(cname, r1, tox), r1.nb_public, enc(W), enc(a), enc(b), enc(cc),
                           rb, sb)
    h = upload(gm_ctx, r1)
    try:
        pk = h.g16_setup(tox, r1.nb_public)
        dpk = gm.ProvingKey(gm_ctx, cname, pk, r1.domain_size, r1.nb_wires, r1.nb_public)
        try:
            proof = dpk.prove_r1cs(h, enc(W), rb, sb)
        finally:
            dpk.free()
    finally:
        h.free()
    assert proof == exp
    assert oracle.g16_check(cname, r1, tox, enc(W), rb, sb, *proof) == 7


@pytest.mark.parametrize("cname,precompute", [("bn254", False), ("bn254", True), ("bls12377", False)])
def test_resident_key_from_the_setup(gm_ctx, oracle, cname, precompute):
    """ProvingKey.setup: the derived arrays become the resident key without leaving
    the device.  The same proof bytes twice, equal to the oracle's; the key reports
    the precomputation it was asked for; host_copy returns gm_g16_setup's arrays."""
    r1, W = R.squaring_chain(300, cname, x=3)
    tox = toxic_bytes(cname)
    enc = lambda v: R.encode_vec(cname, v)
    a, b, cc = r1.solve_abc(W)
    rb, sb = enc([0x77777]), enc([0x99999])
    want = oracle.g16_setup(cname, r1, tox)
    exp = oracle.g16_prove(cname, want, r1.nb_public, enc(W), enc(a), enc(b), enc(cc), rb, sb)
    h = upload(gm_ctx, r1)
    try:
        dpk = gm.ProvingKey.setup(gm_ctx, h, tox, r1.nb_public, precompute=precompute)
        try:
            assert dpk.precomputed == precompute
            assert dpk.prove_r1cs(h, enc(W), rb, sb) == exp
            assert dpk.prove(enc(W), enc(a), enc(b), enc(cc), rb, sb) == exp
        finally:
            dpk.free()
        dpk, copy = gm.ProvingKey.setup(gm_ctx, h, tox, r1.nb_public, precompute=precompute, host_copy=True)
        try:
            assert copy == h.g16_setup(tox, r1.nb_public)
            assert_matches_oracle(copy, want)
            assert dpk.prove_r1cs(h, enc(W), rb, sb) == exp
        finally:
            dpk.free()
    finally:
        h.free()


def test_resident_key_with_commitments(gm_ctx, oracle):
    """The BSB22 K filter of a key made by ProvingKey.setup: the oracle's proof."""
    cname = "bn254"
    c = pyref.CURVES[cname]
    r1, info, solve = R.commitment_chain(200, cname, 2)
    tox = [t % c.r for t in TOXIC]
    pk = oracle.g16_setup_bsb22(cname, r1, info, tox, [0x31337, 0x4242])
    exp = oracle.g16_prove_bsb22(cname, pk, r1, info, solve, 0x1357, 0x2468)
    gamma_wires = sorted(set(w for ci in info for w in ci["private_committed"]) |
                         set(ci["commitment_index"] for ci in info))
    h = upload(gm_ctx, r1)
    try:
        dpk = gm.ProvingKey.setup(gm_ctx, h, toxic_bytes(cname), r1.nb_public, gamma_wires)
        try:
            assert dpk.prove_r1cs(h, exp["Wb"], exp["rb"], exp["sb"]) == (exp["ar"], exp["bs"], exp["krs"])
        finally:
            dpk.free()
    finally:
        h.free()


def test_refusals(gm_ctx, oracle):
    cname = "bn254"
    c = pyref.CURVES[cname]
    r1 = R.cubic_circuit(cname)[0]
    tox = toxic_bytes(cname)
    want = oracle.g16_setup(cname, r1, tox)
    w8 = pyref.domain_generator(c, 4)
    h = upload(gm_ctx, r1)

    def with_toxic(i, v):
        t = list(TOXIC)
        t[i] = v
        return toxic_bytes(cname, t)

    cases = [
        ("nb_public exceeds", lambda: h.g16_setup(tox, r1.nb_wires + 1)),
        ("gamma_wires\\[1\\]", lambda: h.g16_setup(tox, 2, [3, 3])),
        ("gamma_wires\\[1\\]", lambda: h.g16_setup(tox, 2, [4, 3])),
        ("gamma_wires\\[0\\]", lambda: h.g16_setup(tox, 2, [1])),
        ("gamma_wires\\[0\\]", lambda: h.g16_setup(tox, 2, [5])),
        ("delta is zero", lambda: h.g16_setup(with_toxic(4, 0), 2)),
        ("gamma is zero", lambda: h.g16_setup(with_toxic(3, 0), 2)),
        ("tau\\^n = 1", lambda: h.g16_setup(with_toxic(0, 1), 2)),
        ("tau\\^n = 1", lambda: h.g16_setup(with_toxic(0, w8), 2)),
        ("tau\\^n = 1", lambda: h.g16_setup_sizes(with_toxic(0, pow(w8, 3, c.r)), 2)),
        ("toxic scalars are NULL", lambda: h.g16_setup(None, 2)),
        ("gm_g16_pk_setup: delta is zero", lambda: gm.ProvingKey.setup(gm_ctx, h, with_toxic(4, 0), 2)),
        ("gm_g16_pk_setup: gamma_wires\\[0\\]", lambda: gm.ProvingKey.setup(gm_ctx, h, tox, 2, [9])),
    ]
    try:
        for pattern, call in cases:
            with pytest.raises(gm.GmError, match=pattern):
                call()
            assert_matches_oracle(h.g16_setup(tox, r1.nb_public), want)
    finally:
        h.free()
    # a constant term, recorded at upload
    table = b"".join(pyref.encode_fr(c, v) for v in (0, 1, 2, c.r - 1, c.r - 2))
    rp = [np.array([0, 1], np.uint32)] * 3
    hc = gm.R1CS(gm_ctx, cname, 1, 3, rp, [[1], [1], [1]], [[0xFFFFFFFF], [1], [2]], table)
    try:
        with pytest.raises(gm.GmError, match="constant term"):
            hc.g16_setup(tox, 1)
    finally:
        hc.free()
    h = upload(gm_ctx, r1)
    try:
        assert_matches_oracle(h.g16_setup(tox, r1.nb_public), want)
    finally:
        h.free()
