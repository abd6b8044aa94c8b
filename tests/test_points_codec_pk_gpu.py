"""gm_g16_pk_upload_encoded: a WriteTo-shaped (compressed) and a WriteRawTo-shaped
(raw) key file, built in Python from the small synthetic key of the
test_pk_io_gpu helpers with the model's encoder, streamed through the device
decoder into a resident key.  The proof from that key equals, byte for byte, the
proof from gm_g16_pk_upload of the same points; refused files name the member
and the record."""
import ctypes
import os
import struct

import pytest

import points_check_cases as pc
import points_codec_model as m

pytestmark = pytest.mark.gpu

TRAILER = b"nbWires follows here"
# writeTo's order (marshal.go:239-311): (key of the pk dict, G2, slice with a u32 length prefix)
ORDER = (("g1_alpha", False, False), ("g1_beta", False, False), ("g1_delta", False, False), ("g1_A", False, True),
         ("g1_B", False, True), ("g1_Z", False, True), ("g1_K", False, True), ("g2_beta", True, False),
         ("g2_delta", True, False), ("g2_B", True, True))


def points_of(cname, g2, data):
    c = pc.params(cname)
    fb, k = 8 * c.fp_limbs, 4 if g2 else 2
    out = []
    for o in range(0, len(data), fb * k):
        raw = [int.from_bytes(data[o + j * fb:o + (j + 1) * fb], "little") for j in range(k)]
        out.append(pc.decode(c, g2, raw) if any(raw) else None)
    return out


def records_of(cname, pk, width):
    """{member: [record]} of a pk dict of gnark-layout arrays."""
    return {key: [m.encode(cname, g2, P, width) for P in points_of(cname, g2, bytes(pk[key]))] for key, g2, _ in ORDER}


def write_key(path, recs, prefix, counts=None):
    """prefix, the members in writeTo's order, TRAILER; counts overrides a slice's length prefix."""
    with open(path, "wb") as f:
        f.write(prefix)
        for key, _, is_slice in ORDER:
            if is_slice:
                f.write(struct.pack(">I", (counts or {}).get(key, len(recs[key]))))
            f.write(b"".join(recs[key]))
        f.write(TRAILER)
    return len(prefix)


def _meta(pk):
    g1b = len(pk["g1_alpha"])
    return dict(infA=pk["infA"], infB=pk["infB"], k_wires=pk.get("k_wires"),
                counts=(len(pk["g1_A"]) // g1b, len(pk["g1_B"]) // g1b, len(pk["g1_K"]) // g1b))


@pytest.fixture(scope="module")
def keys(oracle):
    from test_pk_io_gpu import _setup
    return {cname: _setup(oracle, cname, 15) for cname in ("bn254", "bls12377")}


@pytest.mark.parametrize("precompute", [False, True], ids=["plain", "precompute"])
@pytest.mark.parametrize("width", [m.COMPRESSED, m.RAW], ids=["compressed", "raw"])
@pytest.mark.parametrize("cname", ["bn254", "bls12377"])
def test_key_from_an_encoded_file_proves_like_the_uploaded_key(gm_ctx, keys, tmp_path, cname, width, precompute):
    import gnark_mi355x as gm
    r1, pk, (W, A, B, C), rb, sb, exp = keys[cname]
    path = str(tmp_path / "pk.bin")
    off = write_key(path, records_of(cname, pk, width), os.urandom(333))
    ref = gm.ProvingKey(gm_ctx, cname, pk, r1.domain_size, r1.nb_wires, r1.nb_public, precompute=precompute)
    try:
        want = ref.prove(W, A, B, C, rb, sb)
    finally:
        ref.free()
    assert want == exp
    gm_ctx.set_points_check_chunk(5 * gm.record_bytes(cname, True, width))     # every slice spans chunks
    try:
        dpk, end, rep, singles = gm.ProvingKey.from_encoded(gm_ctx, cname, path, off, _meta(pk), r1.domain_size,
                                                            r1.nb_wires, r1.nb_public, width, precompute=precompute)
    finally:
        gm_ctx.set_points_check_chunk(0)
    try:
        assert dpk.precomputed == precompute
        assert dpk.prove(W, A, B, C, rb, sb) == want
    finally:
        dpk.free()
    assert end == os.path.getsize(path) - len(TRAILER)
    assert singles == b"".join(bytes(pk[k]) for k in ("g1_alpha", "g1_beta", "g1_delta", "g2_beta", "g2_delta"))
    assert rep["first_bad_member"] is None
    g1b = gm.point_bytes(cname, False)
    for key, g2, _ in ORDER:
        n = len(pk[key]) // (g1b * (2 if g2 else 1))
        inf = sum(1 for P in points_of(cname, g2, bytes(pk[key])) if P is None)
        assert rep[key] == dict(n=n, infinities=inf, not_reduced=0, off_curve=0, off_subgroup=0, bad_encoding=0,
                                no_root=0, first_bad=n, first_class=0), key


@pytest.mark.parametrize("cname", ["bn254", "bls12377"])
def test_refused_files_name_the_member_and_the_record(gm_ctx, keys, tmp_path, cname):
    import gnark_mi355x as gm
    r1, pk, (W, A, B, C), rb, sb, exp = keys[cname]
    width = m.COMPRESSED
    recs = records_of(cname, pk, width)
    meta = _meta(pk)
    args = (r1.domain_size, r1.nb_wires, r1.nb_public, width)

    def refused(path, off, meta=meta):
        with pytest.raises(gm.GmError) as e:
            gm.ProvingKey.from_encoded(gm_ctx, cname, path, off, meta, *args)
        assert e.value.rc == -1 and not e.value.handle            # GM_ERR_INVALID, no key
        return e.value.report, str(e.value)

    good = str(tmp_path / "good.bin")
    off = write_key(good, recs, b"hdr")
    # a wrong slice length: the file's prefix, then meta's count
    path = str(tmp_path / "len.bin")
    write_key(path, recs, b"hdr", counts={"g1_B": len(recs["g1_B"]) + 1})
    rep, msg = refused(path, off)
    assert rep["first_bad_member"] == "g1_B" and "expected %d" % len(recs["g1_B"]) in msg
    bad_meta = dict(meta, counts=(meta["counts"][0] + 1,) + meta["counts"][1:])
    rep, msg = refused(good, off, bad_meta)
    assert rep["first_bad_member"] == "g1_A"
    # a truncated file: the middle of G2.B is missing
    cut = os.path.getsize(good) - len(TRAILER) - 3 * len(recs["g2_B"][0]) // 2
    path = str(tmp_path / "cut.bin")
    with open(path, "wb") as f:
        f.write(open(good, "rb").read()[:cut])
    per = 3
    gm_ctx.set_points_check_chunk(per * gm.record_bytes(cname, True, width))
    try:
        rep, msg = refused(path, off)
    finally:
        gm_ctx.set_points_check_chunk(0)
    nb2 = len(recs["g2_B"])
    lost = (nb2 - 2) // per * per                                  # the chunk that holds record nb2 - 2, cut in half
    assert rep["first_bad_member"] == "g2_B" and "end of file" in msg
    assert (rep["g2_B"]["n"], rep["g2_B"]["first_bad"], rep["g2_B"]["first_class"]) == (nb2, lost, 0)
    assert "gm_g16_pk_upload_encoded: member 9: records %d to %d" % (lost, min(lost + per, nb2) - 1) in msg
    assert rep["g1_K"]["first_bad"] == rep["g1_K"]["n"] == len(recs["g1_K"])      # what lies before it was decoded
    # cut inside a length prefix: the member is named, nothing is decoded
    cut = off + sum(len(b"".join(recs[k])) for k in ("g1_alpha", "g1_beta", "g1_delta", "g1_A")) + 4 + 2
    with open(path, "wb") as f:
        f.write(open(good, "rb").read()[:cut])
    rep, msg = refused(path, off)
    assert rep["first_bad_member"] == "g1_B" and "member 6: the length prefix" in msg and "end of file" in msg
    # one point of the twist outside the subgroup in G2.B
    cof = [pc.decode(pc.params(cname), True, raw) for name, raw, _ in pc.cases(cname, True) if name == "[r]P'"][0]
    idx = len(recs["g2_B"]) - 2
    bad = dict(recs, g2_B=recs["g2_B"][:idx] + [m.encode(cname, True, cof, width)] + recs["g2_B"][idx + 1:])
    path = str(tmp_path / "sub.bin")
    write_key(path, bad, b"hdr")
    gm_ctx.set_points_check_chunk(3 * gm.record_bytes(cname, True, width))   # the record sits in a later chunk
    try:
        rep, msg = refused(path, off)
    finally:
        gm_ctx.set_points_check_chunk(0)
    assert rep["first_bad_member"] == "g2_B"
    assert (rep["g2_B"]["first_bad"], rep["g2_B"]["first_class"], rep["g2_B"]["off_subgroup"]) == (idx, 3, 1)
    assert rep["g1_K"]["first_bad"] == rep["g1_K"]["n"] == len(recs["g1_K"])
    # one x without a root in G1.K
    noroot = [rec for kind, _, rec, _ in m.decode_cases(cname, False, width) if kind == "no root"][0]
    idx = 1
    bad = dict(recs, g1_K=recs["g1_K"][:idx] + [noroot] + recs["g1_K"][idx + 1:])
    path = str(tmp_path / "root.bin")
    write_key(path, bad, b"hdr")
    rep, msg = refused(path, off)
    assert rep["first_bad_member"] == "g1_K"
    assert (rep["g1_K"]["first_bad"], rep["g1_K"]["first_class"], rep["g1_K"]["no_root"]) == (idx, 5, 1)
    assert rep["g2_B"]["n"] == rep["g2_beta"]["n"] == 0            # decoding stopped at G1.K: what follows it in the file
    assert rep["g1_Z"]["first_bad"] == rep["g1_Z"]["n"] == len(recs["g1_Z"])
    # the members are decoded in the file's order: a bad G1.A is named before a bad G2 beta,
    # and a bad G2 beta before G2.B, after every G1 slice
    bad = dict(recs, g2_beta=[m.reflag(cname, recs["g2_beta"][0], 0)], g1_A=[noroot] + recs["g1_A"][1:])
    write_key(path, bad, b"hdr")
    rep, msg = refused(path, off)
    assert rep["first_bad_member"] == "g1_A" and (rep["g1_A"]["first_bad"], rep["g1_A"]["first_class"]) == (0, 5)
    assert rep["g1_delta"]["n"] == 1 and rep["g1_B"]["n"] == rep["g2_beta"]["n"] == 0
    write_key(path, dict(bad, g1_A=recs["g1_A"]), b"hdr")
    rep, msg = refused(path, off)
    assert rep["first_bad_member"] == "g2_beta" and (rep["g2_beta"]["first_bad"], rep["g2_beta"]["first_class"]) == (0, 4)
    assert rep["g1_K"]["first_bad"] == rep["g1_K"]["n"] == len(recs["g1_K"])
    assert rep["g2_delta"]["n"] == rep["g2_B"]["n"] == 0
    # with the subgroup check off the off-subgroup file loads; the right file loads and proves
    dpk, end, rep, _ = gm.ProvingKey.from_encoded(gm_ctx, cname, str(tmp_path / "sub.bin"), off, meta, *args,
                                                  flags=gm.DECODE_NO_SUBGROUP_CHECK)
    dpk.free()
    assert rep["first_bad_member"] is None
    dpk, end, rep, _ = gm.ProvingKey.from_encoded(gm_ctx, cname, good, off, meta, *args)
    try:
        assert dpk.prove(W, A, B, C, rb, sb) == exp
    finally:
        dpk.free()


def test_curve_id_2_is_refused(gm_ctx, tmp_path):
    import gnark_mi355x as gm
    L = gm.load_library()
    rep, end, pk = gm._G16PkDecodeReport(), ctypes.c_uint64(), ctypes.c_void_p(0x1234)
    h = gm._PkHost()
    h.domain_size = 8
    singles = ctypes.create_string_buffer(1024)
    rc = L.gm_g16_pk_upload_encoded(gm_ctx.handle, 2, ctypes.byref(h), 0, 0, 0, 0, singles, ctypes.byref(rep),
                                    ctypes.byref(end), ctypes.byref(pk))
    assert rc == -4 and not pk.value
    msg = L.gm_last_error().decode()
    assert "gm_g16_pk_upload_encoded" in msg and "BLS12-381" in msg
