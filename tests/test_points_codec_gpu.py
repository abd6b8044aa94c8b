"""gm_points_decode / gm_points_decode_host / gm_points_encode and the square
roots behind them on the device, against the Python-integer model
(points_codec_model), for all six curve-and-group pairs: roots of every kind
of element, every kind of record in both widths with and without the subgroup
check, placement in arrays of 1 to 300 records, the encoder byte for byte and
decode(encode(P)) = P, and host streaming across chunk edges."""
import ctypes
import random

import numpy as np
import pytest

import points_check_cases as pc
import points_codec_model as m
from points_check_cases import sub

pytestmark = pytest.mark.gpu

GUARD, GUARD_BYTE = 64, 0xA5
GROUP_IDS = ["%s-%s" % (c, "g2" if g2 else "g1") for c, g2 in pc.GROUPS]
WIDTHS = (m.COMPRESSED, m.RAW)
WIDTH_IDS = {m.COMPRESSED: "compressed", m.RAW: "raw"}


# ---- roots ------------------------------------------------------------------------
def _two_sylow_squares(c):
    """For p - 1 = 2^S s: one square a per k = 0 .. S - 1 with a^s of order exactly
    2^k, so that every trip count of the Tonelli-Shanks loop occurs (BLS12-377:
    k = 0 .. 45; test_fp_roots places them inside one wave)."""
    p = c.p
    s, S = p - 1, 0
    while s % 2 == 0:
        s //= 2
        S += 1
    z = 2
    while pow(z, (p - 1) // 2, p) != p - 1:
        z += 1
    root = pow(z, s, p)
    sinv = pow(s, -1, 1 << S)
    rng = random.Random(0x77 + S)
    out = []
    for k in range(S):
        t = pow(root, 1 << (S - k), p)                       # order 2^k
        a = pow(t, sinv, p) * pow(rng.randrange(2, p), 1 << S, p) % p
        at = pow(a, s, p)
        assert pow(at, 1 << k, p) == 1 and (k == 0 or pow(at, 1 << (k - 1), p) != 1)
        out.append(a)
    return S, out


@pytest.mark.parametrize("cname", pc.CURVE_NAMES)
def test_fp_roots(gm_ctx, cname):
    c = pc.params(cname)
    p, fb = c.p, 8 * c.fp_limbs
    rng = random.Random(0x51 + len(cname))
    z = 2
    while pow(z, (p - 1) // 2, p) != p - 1:
        z += 1
    sq = [rng.randrange(1, p) ** 2 % p for _ in range(24)]
    S, sylow = _two_sylow_squares(c)
    assert len(sylow) == S and (cname != "bls12377" or S == 46)
    import gnark_mi355x as gm
    # the Sylow squares go first: element i runs in lane i % 64 of the hook's block i // 64
    # (one wave per block), so lanes 0 .. S - 1 of one wave see every trip count at once
    elems = sylow + [0, 1, p - 1, 4, z] + sq + [a * z % p for a in sq[:12]]
    first = elems.index(sylow[0])
    assert elems[first:first + S] == sylow and gm.FE_SQRT_HOOK_BLOCK == 64
    assert first // gm.FE_SQRT_HOOK_BLOCK == (first + S - 1) // gm.FE_SQRT_HOOK_BLOCK, "the squares span two waves"
    want = [sub.sqrt_fp(a, p) is not None for a in elems]
    assert want.count(False) >= 12 and want[S:S + 2] == [True, True] and all(want[:S])
    assert want[S + 2] == (p % 4 == 1)                       # -1 is a square iff p = 1 mod 4
    data = b"".join(pc.mont(c, a).to_bytes(fb, "little") for a in elems)
    roots, ex = gm_ctx.test_fe_sqrt(cname, data, fp2=False)
    assert [bool(e) for e in ex] == want
    rinv = pow(1 << (8 * fb), -1, p)
    for i, a in enumerate(elems):
        if want[i]:
            raw = int.from_bytes(roots[i * fb:(i + 1) * fb], "little")
            assert raw < p
            r = raw * rinv % p
            assert r * r % p == a, (i, a)


@pytest.mark.parametrize("cname", pc.CURVE_NAMES)
def test_fp2_roots(gm_ctx, cname):
    import pyref
    c = pc.params(cname)
    p, fb, beta = c.p, 8 * c.fp_limbs, c.beta
    F = pyref.F2(c)
    rng = random.Random(0x52 + len(cname))
    z = 2
    while pow(z, (p - 1) // 2, p) != p - 1:
        z += 1
    rnd = [(rng.randrange(p), rng.randrange(1, p)) for _ in range(16)]
    squares = [F.mul(x, x) for x in rnd]
    # the second candidate (a0 - n) / 2 is the square for one sign of the norm's root n and
    # the first for the other: both happen among these whichever root the device takes
    firsts = [sub.sqrt_fp((a[0] + sub.sqrt_fp((a[0] * a[0] - beta * a[1] * a[1]) % p, p)) * pow(2, -1, p) % p, p)
              is not None for a in squares]
    assert True in firsts and False in firsts
    nonsq = [a for a in ((rng.randrange(p), rng.randrange(1, p)) for _ in range(40)) if sub.sqrt_fp2(a, c) is None]
    assert len(nonsq) >= 8
    real = [(a * a % p, 0) for a in (rng.randrange(1, p) for _ in range(4))]           # a1 = 0, a0 a square
    real += [(a * a * z % p, 0) for a in (rng.randrange(1, p) for _ in range(4))]      # a1 = 0, a0 not: (0, s)
    imag = [(0, rng.randrange(1, p)) for _ in range(8)]                                  # a0 = 0
    elems = [(0, 0), (1, 0), (p - 1, 0), (0, 1), (beta % p, 0)] + squares + nonsq + real + imag
    want = [sub.sqrt_fp2(a, c) is not None for a in elems]
    assert all(want[5:5 + len(squares)]) and all(want[5 + len(squares) + len(nonsq):][:8])
    data = b"".join(pc.mont(c, v).to_bytes(fb, "little") for a in elems for v in a)
    roots, ex = gm_ctx.test_fe_sqrt(cname, data, fp2=True)
    assert [bool(e) for e in ex] == want
    rinv = pow(1 << (8 * fb), -1, p)
    for i, a in enumerate(elems):
        if want[i]:
            raw = [int.from_bytes(roots[(2 * i + j) * fb:(2 * i + j + 1) * fb], "little") for j in (0, 1)]
            assert all(v < p for v in raw)
            r = tuple(v * rinv % p for v in raw)
            assert F.mul(r, r) == (a[0] % p, a[1] % p), (i, a)


# ---- decode ---------------------------------------------------------------------------
def run_decode(ctx, cname, g2, recs, width, flags=0):
    """gm_points_decode with guard bytes behind the status and the point arrays:
    (report, status, point bytes)."""
    import gnark_mi355x as gm
    L = gm.load_library()
    n, pb = len(recs), gm.point_bytes(cname, g2)
    enc = ctx.copy_to_device(b"".join(recs))
    pts = ctx.copy_to_device(bytes([GUARD_BYTE]) * (n * pb + GUARD))
    st = ctx.copy_to_device(bytes([GUARD_BYTE]) * (n + GUARD))
    rep = gm._PointsDecodeReport()
    try:
        rc = L.gm_points_decode(ctx.handle, gm.curve_id(cname), int(g2), width, flags, enc.ptr, n, pts.ptr, st.ptr,
                                ctypes.byref(rep))
        assert rc == 0, L.gm_last_error().decode()
        got_st = np.frombuffer(st.to_host(), np.uint8)
        got_pts = pts.to_host()
        assert (got_st[n:] == GUARD_BYTE).all(), "the status array's guard bytes were written"
        assert got_pts[n * pb:] == bytes([GUARD_BYTE]) * GUARD, "the point array's guard bytes were written"
        # the same launch without a status array gives the same report and points
        pts2, rep2 = ctx.points_decode(cname, enc, n, g2, width, flags)
        try:
            assert rep2 == rep.as_dict() and pts2.to_host(n * pb) == got_pts[:n * pb]
        finally:
            pts2.free()
        return rep.as_dict(), [int(v) for v in got_st[:n]], got_pts[:n * pb]
    finally:
        for b in (enc, pts, st):
            b.free()


def check_against_model(ctx, cname, g2, recs, width, flags=0, names=None):
    want_rep, want_st, want_pts = m.decode_all(cname, g2, recs, width, flags)
    rep, st, pts = run_decode(ctx, cname, g2, recs, width, flags)
    wrong = [(names[i] if names else i, st[i], want_st[i]) for i in range(len(recs)) if st[i] != want_st[i]]
    assert not wrong, wrong
    assert rep == want_rep
    pb = len(want_pts) // max(len(recs), 1)
    diff = [names[i] if names else i for i in range(len(recs)) if pts[i * pb:(i + 1) * pb] != want_pts[i * pb:(i + 1) * pb]]
    assert not diff, diff
    return rep, st


@pytest.mark.parametrize("flags", [0, m.NO_SUBGROUP_CHECK], ids=["checked", "no-subgroup-check"])
@pytest.mark.parametrize("width", WIDTHS, ids=WIDTH_IDS.values())
@pytest.mark.parametrize("cname,g2", pc.GROUPS, ids=GROUP_IDS)
def test_every_case_decodes_as_the_model(gm_ctx, cname, g2, width, flags):
    cs = m.decode_cases(cname, g2, width)
    kinds = {k for k, _, _, _ in cs}
    # every kind is there wherever the curve admits it (the CPU suite asserts the full sets):
    # BN254 G1 has no off-subgroup point and BN254 no invalid flag
    assert ("off subgroup" in kinds) == ((cname, g2) != ("bn254", False))
    assert ("invalid flag" in kinds) == (cname != "bn254")
    assert {"valid", "infinity", "other width", "not reduced"} <= kinds
    assert ("y = 0" in kinds) == ((cname, g2) == ("bls12377", False))    # the one group of even order
    assert ("no root" in kinds, "off curve" in kinds) == ((True, False) if width == m.COMPRESSED else (False, True))
    recs = [rec for _, _, rec, _ in cs]
    names = ["%s: %s" % (k, nm) for k, nm, _, _ in cs]
    rep, st = check_against_model(gm_ctx, cname, g2, recs, width, flags, names)
    if flags == 0:
        assert st == [want for _, _, _, want in cs]
    else:
        assert rep["off_curve"] == rep["off_subgroup"] == 0
    assert rep["infinities"] == sum(1 for k, _, _, _ in cs if k == "infinity")


def pick(cname, g2, width, cls):
    return [rec for _, _, rec, want in m.decode_cases(cname, g2, width) if want == cls and m.decode(
        cname, g2, rec, width)[1] is False]


@pytest.mark.parametrize("cname,g2", pc.GROUPS, ids=GROUP_IDS)
def test_placement_counts_and_first_bad(gm_ctx, cname, g2):
    for width, sizes in ((m.COMPRESSED, (1, 127, 128, 129, 300)), (m.RAW, (129,))):
        good = pick(cname, g2, width, m.OK)
        bad = {k: pick(cname, g2, width, k) for k in range(1, 6)}
        mid = m.NO_ROOT if width == m.COMPRESSED else m.OFF_CURVE
        last = m.OFF_SUBGROUP if bad[m.OFF_SUBGROUP] else mid
        for n in sizes:
            base = [good[i % len(good)] for i in range(n)]
            layouts = [{}, {0: last}, {n - 1: m.BAD_ENCODING}]
            if n > 128:
                layouts += [{127: mid}, {128: last}]                # either side of a block edge
            if n >= 127:
                layouts += [{n - 1: m.NOT_REDUCED, 64: last},       # two classes: first_bad is the minimum,
                            {63: mid, 5: m.BAD_ENCODING, n - 2: last}]  # whichever wave or block sees it
            for layout in layouts:
                recs = list(base)
                for idx, k in layout.items():
                    recs[idx] = bad[k][idx % len(bad[k])]
                rep, st = check_against_model(gm_ctx, cname, g2, recs, width)
                if layout:
                    assert rep["first_bad"] == min(layout) and rep["first_class"] == layout[min(layout)]
                    assert sorted(i for i, k in enumerate(st) if k) == sorted(layout)


# ---- encode ---------------------------------------------------------------------------
@pytest.mark.parametrize("width", WIDTHS, ids=WIDTH_IDS.values())
@pytest.mark.parametrize("cname,g2", pc.GROUPS, ids=GROUP_IDS)
def test_encode_is_the_model_and_decode_inverts_it(gm_ctx, cname, g2, width):
    import gnark_mi355x as gm
    c = pc.params(cname)
    raws = [raw for _, raw, _ in pc.cases(cname, g2)]        # valid, infinity, non-reduced, off curve, off subgroup
    raws = (raws * 8)[:131]                                  # more than one block, not a multiple of the wave
    reduced = [all(v < c.p for v in raw) for raw in raws]
    assert reduced.count(False) >= 6 and any(not any(r) for r in raws)
    want = [m.encode(cname, g2, pc.decode(c, g2, raw) if any(raw) else None, width) if ok
            else bytes(m.record_bytes(c, g2, width)) for raw, ok in zip(raws, reduced)]
    n, rb = len(raws), gm.record_bytes(cname, g2, width)
    pts = gm_ctx.copy_points_to_device(cname, b"".join(pc.raw_bytes(c, r) for r in raws), g2)
    enc, not_reduced = gm_ctx.points_encode(cname, pts, n, g2, width)
    try:
        got = enc.to_host(n * rb)
        diff = [i for i in range(n) if got[i * rb:(i + 1) * rb] != want[i]]
        assert not diff, diff
        assert not_reduced == reduced.count(False)
        # decode(encode(P)) = P on the device, for the points the decoder accepts
        back, rep, st = gm_ctx.points_decode(cname, enc, n, g2, width, status=True)
        try:
            out = back.to_host(n * gm.point_bytes(cname, g2))
        finally:
            back.free()
        pb = gm.point_bytes(cname, g2)
        ok = [i for i in range(n) if reduced[i] and pc.classify(cname, g2, raws[i])[0] == pc.OK]
        assert len(ok) >= 20 and all(st[i] == 0 for i in ok)
        assert all(out[i * pb:(i + 1) * pb] == pc.raw_bytes(c, raws[i]) for i in ok)
        assert m.decode_all(cname, g2, want, width)[:2] == (rep, [int(v) for v in st])
    finally:
        pts.free()
        enc.free()


# ---- host streaming ------------------------------------------------------------------
@pytest.mark.parametrize("cname,g2", pc.GROUPS, ids=GROUP_IDS)
def test_host_streaming_equals_the_resident_entry(gm_ctx, cname, g2):
    import gnark_mi355x as gm
    for width in WIDTHS:
        good = pick(cname, g2, width, m.OK)
        n = 300
        recs = [good[i % len(good)] for i in range(n)]
        recs[17] = m.encode(cname, g2, None, width)                  # an infinity in the first chunk
        recs[200] = pick(cname, g2, width, m.NOT_REDUCED)[0]         # the last record of 201: a chunk of its own
        recs[250] = (pick(cname, g2, width, m.OFF_SUBGROUP) or pick(cname, g2, width, m.BAD_ENCODING))[0]
        recs[299] = pick(cname, g2, width, m.BAD_ENCODING)[0]
        rb, pb = gm.record_bytes(cname, g2, width), gm.point_bytes(cname, g2)
        for count in (300, 201):                                     # chunks of 100, 100, 100 and of 100, 100, 1
            sub_recs = recs[:count]
            want_rep, _, want_pts = m.decode_all(cname, g2, sub_recs, width)
            dev_rep, _, dev_pts = run_decode(gm_ctx, cname, g2, sub_recs, width)
            assert dev_rep == want_rep and dev_pts == want_pts
            data = b"".join(sub_recs)
            gm_ctx.set_points_check_chunk(100 * rb)
            try:
                host_pts, rep = gm_ctx.points_decode_host(cname, data, g2, width)              # points_host only
                assert rep == dev_rep and host_pts == dev_pts
                buf = gm_ctx.copy_to_device(bytes([GUARD_BYTE]) * (count * pb + GUARD))
                try:
                    none, rep = gm_ctx.points_decode_host(cname, data, g2, width, points_dev=buf, to_host=False)
                    assert none is None and rep == dev_rep                                     # points_dev only
                    assert buf.to_host() == dev_pts + bytes([GUARD_BYTE]) * GUARD
                    buf.write(bytes([GUARD_BYTE]) * (count * pb))
                    host_pts, rep = gm_ctx.points_decode_host(cname, data, g2, width, points_dev=buf)  # both
                    assert rep == dev_rep and host_pts == dev_pts
                    assert buf.to_host() == dev_pts + bytes([GUARD_BYTE]) * GUARD
                finally:
                    buf.free()
            finally:
                gm_ctx.set_points_check_chunk(0)
        host_pts, rep = gm_ctx.points_decode_host(cname, b"".join(recs), g2, width,
                                                  flags=m.NO_SUBGROUP_CHECK)                   # the default chunk
        assert (rep, host_pts) == m.decode_all(cname, g2, recs, width, m.NO_SUBGROUP_CHECK)[::2]
