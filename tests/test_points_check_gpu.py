"""gm_points_check / gm_points_check_host / gm_g16_pk_check[_dump] on the device
against the Python-integer definition (points_check_cases.classify: limbs < p,
the curve equation, pyref.Group.mul(P, r) being infinity), for all six
curve-and-group pairs: every listed kind of valid, non-reduced, off-curve and
off-subgroup point (low-order points, y = 0 and P beside -P included), their
placement in arrays of 1 to 300 points, the status bytes and the guard behind
them, host streaming across chunk edges, and a Groth16 key from memory and from
a WriteDump-shaped file."""
import ctypes
import hashlib
import os

import numpy as np
import pytest

import points_check_cases as pc

pytestmark = pytest.mark.gpu

GUARD, GUARD_BYTE = 64, 0xA5
GROUP_IDS = ["%s-%s" % (c, "g2" if g2 else "g1") for c, g2 in pc.GROUPS]


def expected(cname, g2, raws):
    """The report and the status bytes the definition gives for a list of raw points."""
    cls = [pc.classify(cname, g2, r) for r in raws]
    st = np.array([k for k, _ in cls], np.uint8)
    bad = np.nonzero(st)[0]
    rep = dict(n=len(raws), infinities=sum(1 for _, inf in cls if inf),
               not_reduced=int((st == pc.NOT_REDUCED).sum()), off_curve=int((st == pc.OFF_CURVE).sum()),
               off_subgroup=int((st == pc.OFF_SUBGROUP).sum()),
               first_bad=int(bad[0]) if len(bad) else len(raws), first_class=int(st[bad[0]]) if len(bad) else 0)
    return rep, st


def blob(cname, raws):
    c = pc.params(cname)
    return b"".join(pc.raw_bytes(c, r) for r in raws)


def run_device(ctx, cname, g2, raws):
    """gm_points_check with a status array that has guard bytes behind it."""
    import gnark_mi355x as gm
    L = gm.load_library()
    n = len(raws)
    pts = ctx.copy_points_to_device(cname, blob(cname, raws), g2)
    st = ctx.copy_to_device(bytes([GUARD_BYTE]) * (n + GUARD))
    rep = gm._PointsReport()
    try:
        rc = L.gm_points_check(ctx.handle, gm.curve_id(cname), int(g2), pts.ptr, n, st.ptr, ctypes.byref(rep))
        assert rc == 0, L.gm_last_error().decode()
        got = np.frombuffer(st.to_host(), np.uint8)
        assert (got[n:] == GUARD_BYTE).all(), "the status array's guard bytes were written"
        # the same launch without a status array gives the same report
        rep2 = ctx.points_check(cname, pts, n, g2)
        assert rep2 == rep.as_dict()
        return rep.as_dict(), got[:n]
    finally:
        pts.free()
        st.free()


@pytest.mark.parametrize("cname,g2", pc.GROUPS, ids=GROUP_IDS)
def test_every_case_has_the_class_of_the_definition(gm_ctx, cname, g2):
    cs = pc.cases(cname, g2)
    raws = [raw for _, raw, _ in cs]
    want_rep, want_st = expected(cname, g2, raws)
    # the cases are what their names say (the oracle decides, the intent is checked against it)
    assert [int(k) for k in want_st] == [k for _, _, k in cs]
    kinds = {k for _, _, k in cs}
    assert kinds == ({0, 1, 2} if (cname, g2) == ("bn254", False) else {0, 1, 2, 3})
    rep, st = run_device(gm_ctx, cname, g2, raws)
    wrong = [(cs[i][0], int(st[i]), int(want_st[i])) for i in range(len(cs)) if st[i] != want_st[i]]
    assert not wrong, wrong
    assert rep == want_rep
    assert rep["infinities"] == 1


def pick(cname, g2, cls):
    """Raw points of one class, infinities left out."""
    return [raw for _, raw, k in pc.cases(cname, g2) if k == cls and any(raw)]


@pytest.mark.parametrize("cname,g2", pc.GROUPS, ids=GROUP_IDS)
def test_placement_counts_and_first_bad(gm_ctx, cname, g2):
    good = pick(cname, g2, pc.OK)
    bad = {k: pick(cname, g2, k) for k in (pc.NOT_REDUCED, pc.OFF_CURVE, pc.OFF_SUBGROUP)}
    last = pc.OFF_SUBGROUP if bad[pc.OFF_SUBGROUP] else pc.OFF_CURVE
    for n in (1, 127, 128, 129, 300):
        base = [good[i % len(good)] for i in range(n)]
        layouts = [{}, {0: last}, {n - 1: pc.NOT_REDUCED}]
        if n > 128:
            layouts += [{127: pc.OFF_CURVE}, {128: last}]           # either side of a block edge
        if n >= 127:
            layouts += [{n - 1: pc.NOT_REDUCED, 64: last},          # two classes: first_bad is the minimum,
                        {63: pc.OFF_CURVE, 5: pc.NOT_REDUCED, n - 2: last}]  # whichever wave or block sees it
        for layout in layouts:
            raws = list(base)
            for idx, k in layout.items():
                raws[idx] = bad[k][idx % len(bad[k])]
            want_rep, want_st = expected(cname, g2, raws)
            rep, st = run_device(gm_ctx, cname, g2, raws)
            assert (st == want_st).all(), (n, layout)
            assert rep == want_rep, (n, layout)
            if layout:
                assert rep["first_bad"] == min(layout) and rep["first_class"] == layout[min(layout)]


@pytest.mark.parametrize("cname,g2", pc.GROUPS, ids=GROUP_IDS)
def test_host_streaming_equals_the_device_entry(gm_ctx, cname, g2):
    import gnark_mi355x as gm
    good = pick(cname, g2, pc.OK)
    last = pick(cname, g2, pc.OFF_SUBGROUP) or pick(cname, g2, pc.OFF_CURVE)
    n = 300
    raws = [good[i % len(good)] for i in range(n)]
    raws[17] = (0,) * len(raws[17])                      # an infinity in the first chunk
    raws[250] = last[0]                                  # the failure sits in the last chunk
    raws[299] = pick(cname, g2, pc.NOT_REDUCED)[0]
    want_rep, _ = expected(cname, g2, raws)
    dev_rep, _ = run_device(gm_ctx, cname, g2, raws)
    data = blob(cname, raws)
    gm_ctx.set_points_check_chunk(100 * gm.point_bytes(cname, g2))   # 300 points: three chunks
    try:
        assert gm_ctx.points_check_host(cname, data, g2) == dev_rep == want_rep
        gm_ctx.set_points_check_chunk(gm.point_bytes(cname, g2) + 1)  # one point per chunk
        assert gm_ctx.points_check_host(cname, data[:7 * gm.point_bytes(cname, g2)], g2) == \
            expected(cname, g2, raws[:7])[0]
    finally:
        gm_ctx.set_points_check_chunk(0)
    assert gm_ctx.points_check_host(cname, data, g2) == want_rep     # the default chunk: one piece
    assert gm_ctx.points_check_host(cname, b"", g2) == expected(cname, g2, [])[0]


# ---- key level --------------------------------------------------------------------
def _key(oracle, cname):
    """(pk byte dict, domain size, wires, public, prove inputs or None)."""
    if cname == "bls12381":
        import bls12381_params as bp
        import pyref
        from test_groth16_gpu import TOXIC
        cons, nb_wires, nb_public, _ = bp.squaring_chain(13)
        pk = pyref.g16_setup(bp.C, cons, nb_wires, nb_public, TOXIC)
        return bp.pk_bytes(pk), pk["n"], nb_wires, nb_public, None
    from test_pk_io_gpu import _setup
    r1, pk, inputs, rb, sb, exp = _setup(oracle, cname, 15)
    return pk, r1.domain_size, r1.nb_wires, r1.nb_public, (inputs, rb, sb, exp)


def _counts(cname, pk):
    import gnark_mi355x as gm
    g1b = gm.point_bytes(cname, False)
    return (len(pk["g1_A"]) // g1b, len(pk["g1_B"]) // g1b, len(pk["g1_K"]) // g1b)


def _clean(rep, sizes):
    for name, n in sizes.items():
        m = rep[name]
        assert m["n"] == n and m["first_bad"] == n and m["first_class"] == 0, name
        assert m["not_reduced"] == m["off_curve"] == m["off_subgroup"] == 0, name
    return rep["first_bad_member"] is None


@pytest.mark.parametrize("cname", pc.CURVE_NAMES)
def test_groth16_key_from_memory(gm_ctx, oracle, cname):
    import gnark_mi355x as gm
    pk, n, nb_wires, nb_public, prove = _key(oracle, cname)
    nbA, nbB, nbK = _counts(cname, pk)
    sizes = dict(g1_alpha=1, g1_beta=1, g1_delta=1, g2_beta=1, g2_delta=1, g1_A=nbA, g1_B=nbB, g1_Z=n - 1, g1_K=nbK,
                 g2_B=nbB)
    assert _clean(gm_ctx.g16_pk_check(cname, pk, n, nb_wires, nb_public), sizes)
    # one G2.B point replaced by a point of the twist outside the subgroup
    g2b = gm.point_bytes(cname, True)
    idx = nbB // 2
    cof = [raw for name, raw, _ in pc.cases(cname, True) if name == "[r]P'"][0]
    badpk = dict(pk)
    b = bytearray(pk["g2_B"])
    b[idx * g2b:(idx + 1) * g2b] = pc.raw_bytes(pc.params(cname), cof)
    badpk["g2_B"] = bytes(b)
    rep = gm_ctx.g16_pk_check(cname, badpk, n, nb_wires, nb_public)
    assert rep["first_bad_member"] == "g2_B"
    assert (rep["g2_B"]["first_bad"], rep["g2_B"]["first_class"], rep["g2_B"]["off_subgroup"]) == (idx, 3, 1)
    assert _clean(rep, {k: v for k, v in sizes.items() if k != "g2_B"}) is False
    # a bad single point is named before the arrays
    badpk["g1_beta"] = pc.raw_bytes(pc.params(cname), pick(cname, False, pc.OFF_CURVE)[0])
    rep = gm_ctx.g16_pk_check(cname, badpk, n, nb_wires, nb_public)
    assert rep["first_bad_member"] == "g1_beta" and rep["g1_beta"]["off_curve"] == 1
    if prove is not None:  # the context still proves
        (W, A, B, C), rb, sb, exp = prove
        dpk = gm.ProvingKey(gm_ctx, cname, pk, n, nb_wires, nb_public)
        try:
            assert dpk.prove(W, A, B, C, rb, sb) == exp
        finally:
            dpk.free()


@pytest.mark.parametrize("cname", ["bn254", "bls12377"])
def test_groth16_key_from_a_dump(gm_ctx, oracle, tmp_path, cname):
    import gnark_mi355x as gm
    from test_pk_io_gpu import _meta
    pk, n, nb_wires, nb_public, prove = _key(oracle, cname)
    counts = _counts(cname, pk)
    nbA, nbB, nbK = counts
    sizes = dict(g1_alpha=0, g1_beta=0, g1_delta=0, g2_beta=0, g2_delta=0, g1_A=nbA, g1_B=nbB, g1_Z=n - 1, g1_K=nbK,
                 g2_B=nbB)
    path = str(tmp_path / "pk.dump")
    off = gm.write_dump_slices(path, cname, pk, os.urandom(777))
    with open(path, "ab") as f:
        f.write(b"what follows G2.B")                    # end_offset is not the end of the file
    before = hashlib.sha256(open(path, "rb").read()).digest()
    gm_ctx.set_points_check_chunk(5 * gm.point_bytes(cname, True))   # every slice spans chunks
    try:
        rep, end = gm_ctx.g16_pk_check_dump(cname, path, off, counts, n)
    finally:
        gm_ctx.set_points_check_chunk(0)
    assert _clean(rep, sizes)
    assert hashlib.sha256(open(path, "rb").read()).digest() == before
    dpk, loader_end = gm.ProvingKey.from_dump(gm_ctx, cname, path, off, _meta(pk), n, nb_wires, nb_public)
    try:
        assert end == loader_end == os.path.getsize(path) - len(b"what follows G2.B")
        (W, A, B, C), rb, sb, exp = prove
        assert dpk.prove(W, A, B, C, rb, sb) == exp         # the context still proves
    finally:
        dpk.free()
    # wrong counts are refused the way the loader refuses them
    with pytest.raises(gm.GmError, match="slice 0"):
        gm_ctx.g16_pk_check_dump(cname, path, off, (nbA + 1, nbB, nbK), n)
    # the same file with one G2.B point replaced
    g2b = gm.point_bytes(cname, True)
    idx = nbB - 1
    cof = [raw for name, raw, _ in pc.cases(cname, True) if name == "[r]P'"][0]
    badpk = dict(pk)
    b = bytearray(pk["g2_B"])
    b[idx * g2b:(idx + 1) * g2b] = pc.raw_bytes(pc.params(cname), cof)
    badpk["g2_B"] = bytes(b)
    bad_path = str(tmp_path / "bad.dump")
    off2 = gm.write_dump_slices(bad_path, cname, badpk, b"h")
    rep, end2 = gm_ctx.g16_pk_check_dump(cname, bad_path, off2, counts, n)
    assert end2 == os.path.getsize(bad_path)
    assert rep["first_bad_member"] == "g2_B"
    assert (rep["g2_B"]["first_bad"], rep["g2_B"]["first_class"], rep["g2_B"]["off_subgroup"]) == (idx, 3, 1)
