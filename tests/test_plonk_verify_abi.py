"""KZG and PLONK verification without a GPU: the symbols, the header against the
Python mirror, and the integer model on its own (plonk_verify_model.py): the model
verifier accepts the model prover's proofs on all three curves and gives every
mutation of the batch test its class, so the fixtures mean something before any
GPU sees them."""
import ctypes
import os
import re

import pytest

import plonk_verify_model as pvm
import pyref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "gnark_mi355x.h")
TEST_HEADER = os.path.join(ROOT, "include", "gnark_mi355x_testhooks.h")
ENTRIES = ("gm_kzg_vk_upload", "gm_kzg_vk_free", "gm_kzg_verify_batch", "gm_kzg_verify_folded", "gm_plonk_vk_upload",
           "gm_plonk_vk_free", "gm_plonk_verify_batch")
HOOKS = ("gm_test_plonk_verify_scalars", "gm_test_plonk_verify_chunked")


def test_symbols_are_exported_from_both_libraries():
    import gnark_mi355x as gm
    L = ctypes.CDLL(gm.LIB_PATH)
    T = ctypes.CDLL(gm.TESTHOOKS_PATH)
    for name in ENTRIES:
        assert hasattr(L, name) and name in gm.SYMBOLS, name
    for name in HOOKS:
        assert hasattr(T, name) and not hasattr(L, name) and name in gm.TEST_SYMBOLS, name


def _enum(src, prefix):
    body = re.search(r"enum\s*\{([^}]*%s[^}]*)\}" % prefix, src).group(1)
    return {k: int(v) for k, v in re.findall(r"(%s[A-Z_]+)\s*=\s*(\d+)" % prefix, body)}


def _struct_fields(src, name):
    body = re.search(r"typedef struct \{([^}]*)\}\s*%s;" % name, src).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        names = [re.sub(r"[\s\*]", "", x) for x in re.sub(r"^(const\s+)?\w+\s*\*?", "", decl, count=1).split(",")]
        fields += [re.sub(r"^const", "", x) for x in names]
    return fields


def test_header_matches_the_python_mirror():
    import gnark_mi355x as gm
    src = open(HEADER).read()
    e = _enum(src, "GM_PLONK_VERIFY_")
    assert e == {"GM_PLONK_VERIFY_OK": gm.PLONK_VERIFY_OK, "GM_PLONK_VERIFY_BAD_POINT": gm.PLONK_VERIFY_BAD_POINT,
                 "GM_PLONK_VERIFY_MISMATCH": gm.PLONK_VERIFY_MISMATCH,
                 "GM_PLONK_VERIFY_BAD_INPUT": gm.PLONK_VERIFY_BAD_INPUT,
                 "GM_PLONK_VERIFY_ALGEBRAIC": gm.PLONK_VERIFY_ALGEBRAIC}
    k = _enum(src, "GM_KZG_VERIFY_")
    assert k == {"GM_KZG_VERIFY_OK": gm.KZG_VERIFY_OK, "GM_KZG_VERIFY_BAD_POINT": gm.KZG_VERIFY_BAD_POINT,
                 "GM_KZG_VERIFY_MISMATCH": gm.KZG_VERIFY_MISMATCH, "GM_KZG_VERIFY_BAD_INPUT": gm.KZG_VERIFY_BAD_INPUT}
    # the first four are the Groth16 entry's values, as the header says
    g = _enum(src, "GM_G16_VERIFY_")
    assert [k[x.replace("G16", "KZG")] for x in g] == list(g.values())
    assert (pvm.OK, pvm.BAD_POINT, pvm.MISMATCH, pvm.BAD_INPUT, pvm.ALGEBRAIC) == tuple(range(5))
    for cname, mirror in (("gm_kzg_vk_host", gm._KzgVkHost), ("gm_kzg_openings_host", gm._KzgOpeningsHost),
                          ("gm_plonk_vk_host", gm._PlonkVkHost), ("gm_plonk_proofs_host", gm._PlonkProofsHost)):
        fields = _struct_fields(src, cname)
        assert [f.rstrip("_") for f, _ in mirror._fields_] == fields, cname
        # every member is a pointer or a size_t: one machine word each
        assert ctypes.sizeof(mirror) == 8 * len(fields), cname
    # the key flag that makes the session's proofs the ones these entries accept
    assert re.search(r"^#define GM_PLONK_PK_LIN_KEY_QK 4u$", src, re.M) and gm.PLONK_PK_LIN_KEY_QK == 4
    assert gm.PLONK_PK_LIN_KEY_QK & gm.PLONK_PK_NO_COSET_CACHE == 0
    hooks = open(TEST_HEADER).read()
    for name in HOOKS:
        assert re.search(r"\b%s\s*\(" % name, hooks)


@pytest.mark.parametrize("nb", [0, 2])
@pytest.mark.parametrize("cname", pvm.CURVES)
def test_model_verifier_accepts_the_model_prover_and_classes_every_mutation(cname, nb):
    c = pyref.CURVES[cname]
    inst, vk, proof = pvm.case(cname, 8, nb)
    assert pvm.verify(c, vk, proof) == pvm.OK
    seen = {}
    for name, bad in pvm.mutations(c, vk, proof):
        st = pvm.verify(c, vk, bad)
        # u is the verifier's own random multiplier: any non-zero u accepts a valid proof
        assert (st == pvm.OK) == (name == "u + 1"), name
        seen[name] = st
    assert seen["bad point"] == pvm.BAD_POINT and seen["u = 0"] == pvm.BAD_INPUT
    assert seen["value 0 + 1"] == pvm.ALGEBRAIC
    assert all(seen["point %d replaced" % k] == pvm.MISMATCH for k in range(9 + nb))
    assert all(seen["public %d + 1" % k] == pvm.ALGEBRAIC for k in range(len(proof.publics)))
    assert all(seen["hashed_cmt %d + 1" % k] == pvm.ALGEBRAIC for k in range(nb))
    assert all(st == pvm.MISMATCH for name, st in seen.items() if name.startswith("second opening"))
    # a wrong key digest
    for k in pvm.KEY_POINTS:
        d = dict(vk.dl)
        d[k] = (d[k] + 1) % c.r
        other = pvm.types.SimpleNamespace(n=vk.n, nb_public=vk.nb_public, rows=vk.rows, dl=d, tau=vk.tau)
        assert pvm.verify(c, other, proof) == pvm.MISMATCH, k
    # a word string >= r in each input array
    for field in ("values", "publics", "hashed", "chal"):
        v = list(getattr(proof, field))
        if v:
            v[-1] = c.r
            assert pvm.verify(c, vk, pvm.clone(proof, **{field: v})) == pvm.BAD_INPUT, field


def test_model_prover_at_n_64():
    c = pyref.CURVES["bls12381"]
    _, vk, proof = pvm.case("bls12381", 64, 2)
    assert pvm.verify(c, vk, proof) == pvm.OK


def test_model_scalars_zero_denominators():
    """zeta on the domain: gnark's inverse of 0 is 0, so the Lagrange term of that row drops out."""
    c = pyref.CURVES["bn254"]
    r = c.r
    vk = pvm.types.SimpleNamespace(n=8, nb_public=2, rows=[3, 5])
    w = pyref.domain_generator(c, 8)
    vals, pub, hc = list(range(1, 10)), [11, 12], [13, 14]
    for zeta in (1, w, pow(w, 3, r)):
        sc, pi, cl, cls = pvm.scalars(c, vk, vals, pub, hc, [2, 3, 4, zeta, 5, 6])
        assert pi == 0 and sc[8 + 2 + 4] == 0  # zh = 0: every term carries it
    sc, pi, _, _ = pvm.scalars(c, vk, vals, pub, hc, [2, 3, 4, 7, 5, 6])
    lag = lambda i: pow(w, i, r) * (pow(7, 8, r) - 1) % r * pow(8 * (7 - pow(w, i, r)) % r, -1, r) % r
    assert pi == (11 * lag(0) + 12 * lag(1) + 13 * lag(3) + 14 * lag(5)) % r


def test_model_kzg():
    c = pyref.CURVES["bls12377"]
    r, tau = c.r, 12345
    z, y, dc = 77, 99, 424242
    dh = (dc - y) * pow(tau - z, -1, r) % r
    assert pvm.kzg_verify(c, tau, dc, dh, z, y) == pvm.OK
    assert pvm.kzg_verify(c, tau, dc, dh, z, y + 1) == pvm.MISMATCH
    assert pvm.kzg_verify(c, tau, dc, dh, r, y) == pvm.BAD_INPUT
    ops = [(dc, dh, z, y, False), (dc + 5, (dc + 5 - y) * pow(tau - z - 1, -1, r) % r, z + 1, y, False)]
    assert pvm.kzg_verify_folded(c, tau, ops, [0, 9]) == pvm.OK   # lambda_0 is taken as 1
    assert pvm.kzg_verify_folded(c, tau, ops, [1, 0]) == pvm.BAD_INPUT
    bad = [ops[0], (dc + 6,) + ops[1][1:]]
    assert pvm.kzg_verify_folded(c, tau, bad, [1, 9]) == pvm.MISMATCH
