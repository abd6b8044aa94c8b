"""The MSM bucket sort with 4-byte entries between its passes and without sorted
keys for G1 plans (csrc/msm_sort.hip, SortGeom in csrc/msm.hpp).

Between the passes an entry is one 32-bit word -- the low kb = F + G bits of the
bucket, the point index, the sign -- when kb + vb <= 32 (vb = 1 + the bits of the
largest value), else 8 bytes; GM_MSM_SORT_WIDE=1 forces 8 bytes.  A G1 MSM's plan
has no sorted keys, a G2 MSM's has.  Every result is compared as an affine point,
bit for bit, with the CPU oracle or pyref, and the two entry widths with each
other; the width a run took is read from the profile counters msm_sort_compact /
msm_sort_wide."""
import pytest

import pyref
import r1cs as R

pytestmark = pytest.mark.gpu

GROUPS = [("bn254", False), ("bn254", True), ("bls12377", False), ("bls12381", False), ("bls12381", True)]
NMAX = (1 << 12) + 3
FR_BITS = {"bn254": 254, "bls12377": 253, "bls12381": 255}


def _plain_geometry(cname, n, c):
    """msm_plan's sort geometry of a plain MSM without GLV at window c (uniform
    rule, no middle pass at these sizes): (W, first narrow window, F)."""
    bits = FR_BITS[cname]
    W = (bits + 1 + c - 1) // c
    narrow = c * W - (bits + 1)
    wn = W - narrow if narrow < W else W
    T, M, F = W << (c - 1), W * n, 4
    while F < 13 and M << (F + 1) <= 2048 * T:
        F += 1
    return W, wn, F


def _digits(cname, k, c):
    """Signed digits (|d|, negative) of scalar k, as k_msm_digits cuts them."""
    W, wn, _ = _plain_geometry(cname, 1, c)
    out, carry = [], 0
    for w in range(W):
        off = w * c - (w - wn if w > wn else 0)
        cw = c - 1 if w >= wn else c
        raw = ((k >> off) & ((1 << cw) - 1)) + carry
        if raw > 1 << (cw - 1):
            out.append(((1 << cw) - raw, True))
            carry = 1
        else:
            out.append((raw, False))
            carry = 0
    return out


def _shared_bits(n, stride, c, W, ming):
    """kb and vb of a precomputed (shared-bucket) MSM of n scalars over W copies
    at `stride`, window c, GM_MSM_SORT_MING = ming (msm_plan, no bins to coarsen
    further at these sizes)."""
    T, M, F = 1 << (c - 1), W * n, 4
    while F < 13 and M << (F + 1) <= 4096 * T:
        F += 1
    return F + ming, 1 + (W * stride - 1).bit_length()


@pytest.fixture(scope="module")
def data(gm_ctx, oracle):
    """Per (curve, group): NMAX random scalars and points as host bytes, made
    once, and a cache of oracle results per input."""
    import device_points
    st, exp = {}, {}

    def get(cname, g2):
        if (cname, g2) not in st:
            S = gm_ctx.random_scalars(cname, NMAX, seed=0xC0DE + g2)
            K = gm_ctx.random_scalars(cname, NMAX, seed=0xC1DE + g2)
            P = device_points.batch_mul_generator(gm_ctx, cname, g2, K, NMAX)
            st[(cname, g2)] = (S.to_host(), P.to_host())
            for b in (S, K, P):
                b.free()
        return st[(cname, g2)]

    def expected(cname, g2, sb, pb):
        key = (cname, g2, sb, pb)
        if key not in exp:
            exp[key] = oracle.msm(cname, g2, sb, pb)
        return exp[key]

    return get, expected


def _both_widths(gm_ctx, monkeypatch, run, rule="msm_sort_compact"):
    """run() once by the rule and once with the wide switch; asserts the width
    each took (`rule`: the width the rule must choose) and returns both results."""
    out = []
    for wide in (False, True):
        if wide:
            monkeypatch.setenv("GM_MSM_SORT_WIDE", "1")
        else:
            monkeypatch.delenv("GM_MSM_SORT_WIDE", raising=False)
        gm_ctx.profile_reset()
        gm_ctx.profile(True)
        try:
            out.append(run())
        finally:
            gm_ctx.profile(False)
            monkeypatch.delenv("GM_MSM_SORT_WIDE", raising=False)
        st = gm_ctx.profile_stats()
        took = {k for k in ("msm_sort_compact", "msm_sort_wide") if st.get(k, (0, 0))[1]}
        assert took == {"msm_sort_wide" if wide else rule}, (wide, took)
    gm_ctx.profile_reset()
    return out


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 1000, NMAX])
@pytest.mark.parametrize("cname,g2", GROUPS)
def test_compact_equals_wide_equals_oracle(gm_ctx, data, monkeypatch, cname, g2, n):
    import gnark_mi355x as gm
    get, expected = data
    sb, pb = get(cname, g2)
    sb, pb = sb[:32 * n], pb[:gm.point_bytes(cname, g2) * n]
    exp = expected(cname, g2, sb, pb)
    S, P = gm_ctx.copy_to_device(sb), gm_ctx.copy_to_device(pb)
    try:
        for window in (8, 16):
            for glv in (1, 0):
                gm_ctx.set_msm_window(window)
                gm_ctx.set_msm_glv(glv)
                a, b = _both_widths(gm_ctx, monkeypatch, lambda: gm_ctx.msm(cname, S, P, n, g2)[1])
                assert a == exp, (window, glv, "compact")
                assert b == exp, (window, glv, "wide")
    finally:
        gm_ctx.set_msm_window(0)
        gm_ctx.set_msm_glv(-1)
        S.free()
        P.free()


@pytest.mark.parametrize("window", [8, 16])
@pytest.mark.parametrize("g2", [False, True])
def test_top_of_packed_range(gm_ctx, data, monkeypatch, g2, window):
    """Constant scalars whose digit in every used window is negative with
    |d| = 2^(c-2): |d| - 1 has its low c - 2 bits set, which covers the kb bits a
    compact entry keeps, in the entry of the last point index as in all others.
    Among them the scalars r - 1, 0 and 1 and points at infinity."""
    import gnark_mi355x as gm
    cname = "bn254"
    c = pyref.CURVES[cname]
    get, expected = data
    n = NMAX
    W, wn, F = _plain_geometry(cname, n, window)
    kb = F
    assert kb <= window - 2
    used = wn - 1                       # full-width windows below the carry's last stop
    k = ((1 << window) - (1 << (window - 2)))            # window 0: raw = 2^c - 2^(c-2)
    for w in range(1, used):
        k |= ((1 << window) - (1 << (window - 2)) - 1) << (window * w)   # + carry
    assert k < c.r
    dg = _digits(cname, k, window)
    assert all(d == 1 << (window - 2) and neg for d, neg in dg[:used]) and dg[used] == (1, False)
    assert all(((d - 1) & ((1 << kb) - 1)) == (1 << kb) - 1 for d, _ in dg[:used])
    sc = [k] * n
    sc[5], sc[77], sc[n - 2] = c.r - 1, 0, 1
    assert sc[n - 1] == k               # the last point index carries the pattern
    sb = b"".join(pyref.encode_fr(c, s) for s in sc)
    pbytes = gm.point_bytes(cname, g2)
    pb = bytearray(get(cname, g2)[1][:pbytes * n])
    for i in (0, 6, 1000, n - 3):
        pb[i * pbytes:(i + 1) * pbytes] = bytes(pbytes)  # infinity
    pb = bytes(pb)
    exp = expected(cname, g2, sb, pb)
    S, P = gm_ctx.copy_to_device(sb), gm_ctx.copy_to_device(pb)
    try:
        gm_ctx.set_msm_window(window)
        gm_ctx.set_msm_glv(0)
        a, b = _both_widths(gm_ctx, monkeypatch, lambda: gm_ctx.msm(cname, S, P, n, g2)[1])
        assert a == exp and b == exp
    finally:
        gm_ctx.set_msm_window(0)
        gm_ctx.set_msm_glv(-1)
        S.free()
        P.free()


@pytest.mark.parametrize("g2", [False, True])
def test_rule_boundary_precomputed(gm_ctx, monkeypatch, g2):
    """Shared-bucket layout: values are w * stride + i, so vb counts W * stride.
    Window 16 (W = 16 copies), GM_MSM_SORT_MING = 9: 32 points give kb + vb =
    22 + 10 = 32 (compact), 33 points 22 + 11 = 33 (wide)."""
    cname, window, ming = "bn254", 16, 9
    c = pyref.CURVES[cname]
    G = pyref.Group(c, g2)
    W = (FR_BITS[cname] + 1 + window - 1) // window
    pts = pyref.random_points(c, 33, 0xB0 + g2, g2)
    pts[3] = None
    sc = pyref.random_scalars(c, 33, 0xB1)
    sc[0], sc[1], sc[2] = c.r - 1, 0, 1
    monkeypatch.setenv("GM_MSM_SORT_MING", str(ming))
    for n, total, path in ((32, 32, "msm_sort_compact"), (33, 33, "msm_sort_wide")):
        kb, vb = _shared_bits(n, n, window, W, ming)
        assert kb + vb == total
        sb = b"".join(pyref.encode_fr(c, s) for s in sc[:n])
        pb = b"".join(pyref.encode_point(c, p, g2) for p in pts[:n])
        S = gm_ctx.copy_to_device(sb)
        pre = gm_ctx.points_upload_precomputed(cname, pb, g2, window)
        try:
            a, b = _both_widths(gm_ctx, monkeypatch, lambda: gm_ctx.msm_precomputed(cname, S, pre, n, g2)[1],
                                rule=path)
        finally:
            S.free()
            pre.free()
        exp = G.msm(sc[:n], pts[:n])
        assert pyref.decode_point(c, a, g2) == exp, (n, "rule")
        assert pyref.decode_point(c, b, g2) == exp, (n, "wide")


@pytest.mark.parametrize("g2", [False, True])
def test_split_coarse_bin_compact(gm_ctx, oracle, monkeypatch, g2):
    """All scalars equal: one bucket of 2^16 + 5 entries, the smallest above
    S2_BIG, so its coarse bin is split (k_msm_s2_scan / k_msm_s2_scatter), with
    4-byte entries, without keys (G1) and with them (G2)."""
    import gnark_mi355x as gm
    cname = "bn254"
    c = pyref.CURVES[cname]
    n = (1 << 16) + 5
    sb = pyref.encode_fr(c, 3) * n
    K = gm_ctx.random_scalars(cname, n, seed=0x5119 + g2)
    P = gm_ctx.batch_mul_base(cname, g2, gm.generator(cname, g2), K, n)
    S = gm_ctx.copy_to_device(sb)
    try:
        exp = oracle.msm(cname, g2, sb, P.to_host())
        a, b = _both_widths(gm_ctx, monkeypatch, lambda: gm_ctx.msm(cname, S, P, n, g2)[1])
        assert a == exp and b == exp
    finally:
        for x in (S, K, P):
            x.free()


@pytest.mark.parametrize("ming", [1, 2])
@pytest.mark.parametrize("g2", [False, True])
def test_middle_pass_compact(gm_ctx, data, monkeypatch, g2, ming):
    """GM_MSM_SORT_MING forces the middle pass (k_msm_sm_count / _scatter) at
    n = 2^12 + 3, on 4-byte entries by the rule and 8-byte ones by the switch."""
    import gnark_mi355x as gm
    cname = "bn254"
    get, expected = data
    sb, pb = get(cname, g2)
    exp = expected(cname, g2, sb, pb)
    monkeypatch.setenv("GM_MSM_SORT_MING", str(ming))
    S, P = gm_ctx.copy_to_device(sb), gm_ctx.copy_to_device(pb)
    try:
        a, b = _both_widths(gm_ctx, monkeypatch, lambda: gm_ctx.msm(cname, S, P, NMAX, g2)[1])
        assert a == exp and b == exp
    finally:
        S.free()
        P.free()


def test_no_stale_keys(gm_ctx, oracle, data):
    """One context: a G2 MSM of 3000 points writes keys into the arena, a G1 MSM
    of 1000 then writes none over them, a G2 MSM of 1000 writes its own.  A
    Groth16 prove (2^10) follows, whose B plan is shared by a G1 and a G2 MSM and
    keeps its keys; last, the G2 launch refuses a plan built without keys."""
    import gnark_mi355x as gm
    cname = "bn254"
    get, expected = data
    bufs = []
    try:
        for g2, n in ((True, 3000), (False, 1000), (True, 1000)):
            sb, pb = get(cname, g2)
            sb, pb = sb[:32 * n], pb[:gm.point_bytes(cname, g2) * n]
            S, P = gm_ctx.copy_to_device(sb), gm_ctx.copy_to_device(pb)
            bufs += [S, P]
            assert gm_ctx.msm(cname, S, P, n, g2)[1] == expected(cname, g2, sb, pb), (g2, n)
        c = pyref.CURVES[cname]
        r1, Wt = R.squaring_chain(1023, cname, x=2)
        assert r1.domain_size == 1 << 10
        tox = R.encode_vec(cname, [(0x1D5A2B3C + 0x11 * i) % c.r for i in range(1, 6)])
        pk = oracle.g16_setup(cname, r1, tox)
        a, b, cc = r1.solve_abc(Wt)
        enc = lambda v: R.encode_vec(cname, v)
        rb, sbs = enc([0xABCDEF0123]), enc([0x13579BDF])
        exp = oracle.g16_prove(cname, pk, r1.nb_public, enc(Wt), enc(a), enc(b), enc(cc), rb, sbs)
        dpk = gm.ProvingKey(gm_ctx, cname, pk, r1.domain_size, r1.nb_wires, r1.nb_public)
        try:
            assert dpk.prove(enc(Wt), enc(a), enc(b), enc(cc), rb, sbs) == exp
        finally:
            dpk.free()
        S, P = bufs[-2], bufs[-1]   # 1000 scalars, 1000 G2 points
        with pytest.raises(gm.GmError, match="no sorted keys"):
            gm_ctx.test_msm_g2_keyless_plan(cname, S, P, 1000)
        sb, pb = get(cname, True)
        assert gm_ctx.msm(cname, S, P, 1000, True)[1] == expected(cname, True, sb[:32000], pb[:128 * 1000])
    finally:
        for x in bufs:
            x.free()
