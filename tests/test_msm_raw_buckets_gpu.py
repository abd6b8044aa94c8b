"""G1 buckets are stored as the accumulation leaves them (x < 8p, the rest < 2p;
msm_impl.hpp "Storage contract"), each run of equal keys once, and the fixup /
reduction kernels take such operands.  These cases steer raw values into every
consumer and compare the affine result with the CPU oracle, bit for bit.

Every case is built from the scalars' signed digits, and `_layout` recomputes on
the CPU which buckets and accumulation slices the construction yields (from the
kernels' constants below), so a case fails loudly instead of going vacuous when
a constant changes.  With the GLV split on, scalars below 2^64 split trivially
(k1 = k, k2 = 0), so the same model holds with the GLV plan's window count; the
r - k scalars of the sign case do not, and that case checks its layout with GLV
off only.  Each case runs right after a larger MSM of another shape on the same
context, so its buckets and parts land in used workspace memory."""
import numpy as np
import pytest

import pyref

pytestmark = pytest.mark.gpu

# msm_impl.hpp: entries per accumulation thread (msm_launch), serial fixup span,
# longest level-1 segment of k_msm_seg
K_G1, K_G2, FIX_SERIAL, L_MAX = 24, 64, 8, 32
C = 16          # forced window
N = 1 << 12
GROUPS = [("bn254", False), ("bn254", True), ("bls12377", False), ("bls12381", False), ("bls12381", True)]
FR_BITS = {"bn254": 254, "bls12377": 253, "bls12381": 255}


def _digits(cname, k, glv):
    """Signed digits (window, |d|, negative) of the canonical scalar k at window C:
    k_msm_digits / emit_digits of msm_impl.hpp.  glv: trivial split only."""
    if glv:
        assert k < 1 << 64
        W, wn = (127 + 1 + C - 1) // C, None
    else:
        bits = FR_BITS[cname]
        W = (bits + 1 + C - 1) // C
        narrow = C * W - (bits + 1)
        wn = W - narrow if narrow < W else W
    out, carry = [], 0
    for w in range(W):
        if glv or w < wn:
            off, cw = (w * C if glv else w * C - max(0, w - wn)), C
        else:
            off, cw = w * C - (w - wn), C - 1
        raw = ((k >> off) & ((1 << cw) - 1)) + carry
        if raw > 1 << (cw - 1):
            d, neg, carry = (1 << cw) - raw, True, 1
        else:
            d, neg, carry = raw, False, 0
        if d:
            out.append((w, d, neg))
    assert carry == 0
    return out


class _Layout:
    """Buckets of the sorted entry list: b -> (first entry, end entry, all negative)."""

    def __init__(self, cname, g2, scalars, glv):
        nb = 1 << (C - 1)
        self.K = K_G2 if g2 else K_G1
        cnt, allneg = {}, {}
        for k in scalars:
            for w, d, neg in _digits(cname, k, glv):
                b = w * nb + d - 1
                cnt[b] = cnt.get(b, 0) + 1
                allneg[b] = allneg.get(b, True) and neg
        self.b = {}
        pos = 0
        for b in sorted(cnt):
            self.b[b] = (pos, pos + cnt[b], allneg[b])
            pos += cnt[b]
        assert pos <= 1 << 25  # msm_launch keeps K_G1 up to 2^25 entries

    def span(self, b):
        bs, be, _ = self.b[b]
        return (be - 1) // self.K - bs // self.K

    def whole(self):       # stored straight from the accumulation
        return [b for b in self.b if self.span(b) == 0]

    def cut(self):         # merged by k_msm_fixup / k_msm_fixup_edge
        return [b for b in self.b if 1 <= self.span(b) <= FIX_SERIAL]

    def long(self):        # k_msm_fix_tree + k_msm_fixup_long
        return [b for b in self.b if self.span(b) > FIX_SERIAL]

    def fills_slice(self):  # a slice inside one bucket that goes on: part_first only
        K = self.K
        return [b for b, (bs, be, _) in self.b.items() if (be - 1) // K - bs // K >= 2]

    def starts_on_edge(self):  # begins with a slice and goes on: part_last only
        return [b for b, (bs, be, _) in self.b.items() if bs % self.K == 0 and self.span(b) >= 1]

    def lone(self, L=L_MAX):  # the only non-empty bucket of its level-1 segment
        seg = {}
        for b in self.b:
            seg.setdefault(b // L, []).append(b)
        return [v[0] for v in seg.values() if len(v) == 1]


@pytest.fixture(scope="module")
def env(gm_ctx, oracle):
    """Per group: N random points (host bytes) and a larger random MSM to run first."""
    import device_points
    import gnark_mi355x as gm
    st = {}

    def get(cname, g2):
        if (cname, g2) not in st:
            n_big = (1 << 13) + 37
            Kk = gm_ctx.random_scalars(cname, n_big, seed=0xB0 + g2)
            P = device_points.batch_mul_generator(gm_ctx, cname, g2, Kk, n_big)
            S = gm_ctx.random_scalars(cname, n_big, seed=0xB8 + g2)
            Kk.free()
            pb = gm.point_bytes(cname, g2)
            st[(cname, g2)] = (S, P, n_big, P.to_host()[: N * pb])
        return st[(cname, g2)]

    yield get
    for S, P, _, _ in st.values():
        S.free()
        P.free()


def _run(gm_ctx, oracle, env, cname, g2, scalars, glv, points=None, precomputed=False):
    c = pyref.CURVES[cname]
    S_big, P_big, n_big, pts = env(cname, g2)
    pb = points if points is not None else pts
    sb = b"".join(pyref.encode_fr(c, k) for k in scalars)
    assert len(scalars) == N
    exp = oracle.msm(cname, g2, sb, pb)
    S = gm_ctx.copy_to_device(sb)
    P = gm_ctx.points_upload_precomputed(cname, pb, g2, 0) if precomputed else gm_ctx.copy_to_device(pb)
    try:
        gm_ctx.set_msm_window(0)
        gm_ctx.set_msm_glv(-1)
        gm_ctx.msm(cname, S_big, P_big, n_big, g2)  # another shape first: used workspace
        if precomputed:
            got = gm_ctx.msm_precomputed(cname, S, P, N, g2=g2)[1]
        else:
            gm_ctx.set_msm_window(C)
            gm_ctx.set_msm_glv(glv)
            got = gm_ctx.msm(cname, S, P, N, g2)[1]
    finally:
        gm_ctx.set_msm_window(0)
        gm_ctx.set_msm_glv(-1)
        S.free()
        P.free()
    assert got == exp


def _lone_scalars():
    """64 digits of window 0, 40 apart (more than L_MAX), all other windows zero:
    the even ones hold 2-5 points, the odd ones 61-67; the rest are zero scalars
    (no entries at all)."""
    sc = []
    for j in range(64):
        sc += [40 * j + 1] * (2 + j % 4 if j % 2 == 0 else 61 + j % 7)
    assert len(sc) <= N
    return sc + [0] * (N - len(sc))


@pytest.mark.parametrize("glv", [0, 1])
@pytest.mark.parametrize("cname,g2", GROUPS)
def test_lone_raw_bucket(gm_ctx, oracle, env, cname, g2, glv):
    sc = _lone_scalars()
    lay = _Layout(cname, g2, sc, glv)
    lone = set(lay.lone())
    assert len(lone) == 64 == len(lay.b)           # every segment: one non-empty bucket
    assert lone & set(lay.whole()) and lone & set(lay.cut())
    assert any(lay.b[b][1] - lay.b[b][0] <= 5 for b in lay.whole())
    _run(gm_ctx, oracle, env, cname, g2, sc, glv)


@pytest.mark.parametrize("cname,g2", [("bn254", False), ("bn254", True)])
def test_lone_raw_bucket_precomputed(gm_ctx, oracle, env, cname, g2):
    _run(gm_ctx, oracle, env, cname, g2, _lone_scalars(), 0, precomputed=True)


@pytest.mark.parametrize("glv", [0, 1])
@pytest.mark.parametrize("cname,g2", GROUPS)
def test_sign_at_bucket_start(gm_ctx, oracle, env, cname, g2, glv):
    """r - k: the low window's digit is negative for every point, so whichever
    entry the sort puts first in those buckets takes the negated copy path; the
    upper windows are the same for all points (spans of N / K slices)."""
    r = pyref.CURVES[cname].r
    ks = [1 + 3 * (i % 200) for i in range(N)]
    sc = [r - k for k in ks]
    if not glv:
        lay = _Layout(cname, g2, sc, 0)
        neg = [b for b in lay.b if lay.b[b][2]]
        assert len(neg) >= 100
        assert any(lay.b[b][0] % lay.K for b in neg) and set(neg) & set(lay.whole())
        assert lay.long()
    _run(gm_ctx, oracle, env, cname, g2, sc, glv)


@pytest.mark.parametrize("glv", [0, 1])
@pytest.mark.parametrize("cname,g2", GROUPS)
def test_edges_inside_a_bucket(gm_ctx, oracle, env, cname, g2, glv):
    """Equal points with equal digits.  Bucket 0 holds 2 K copies of one point
    from entry 0 on, so the two slices it fills sum to the same point and the
    fixup's add of the two raw parts is a doubling.  Further buckets hold P and
    -P pairs only (they sum to infinity: whole, cut, and over many slices) and
    pairs mixed with other points (infinity inside the run, then on)."""
    import gnark_mi355x as gm
    c = pyref.CURVES[cname]
    G = pyref.Group(c, g2)
    K = K_G2 if g2 else K_G1
    pbytes = gm.point_bytes(cname, g2)
    pts = bytearray(env(cname, g2)[3])
    P0 = bytes(pts[:pbytes])
    P1 = bytes(pts[pbytes:2 * pbytes])
    N1 = pyref.encode_point(c, G.neg(pyref.decode_point(c, P1, g2)), g2)
    sc, i = [], 0

    def put(point, digit):
        nonlocal i
        if point is not None:
            pts[i * pbytes:(i + 1) * pbytes] = point
        sc.append(digit)
        i += 1

    for _ in range(2 * K):
        put(P0, 1)
    for _ in range(3):                      # whole: P - P
        put(P1, 50), put(N1, 50)
    for _ in range(K):                      # cut: only pairs
        put(P1, 100), put(N1, 100)
    for _ in range(6 * K):                  # long: only pairs
        put(P1, 150), put(N1, 150)
    for j in range(3 * K):                  # pairs among other points
        put(P1, 200), put(N1, 200), put(None, 200)
    for j in range(K):                      # a run of equal points after others
        put(None, 250), put(P0, 250)
    while i < N:
        put(None, 300 + 40 * (i % 64))
    lay = _Layout(cname, g2, sc, glv)
    assert lay.b[0][:2] == (0, 2 * K) and lay.span(0) == 1 and 0 in lay.starts_on_edge()
    assert 49 in lay.whole() and 99 in lay.cut() and 149 in lay.long()
    assert 199 in lay.fills_slice() and 249 in lay.cut()
    _run(gm_ctx, oracle, env, cname, g2, sc, glv, points=bytes(pts))


@pytest.mark.parametrize("glv", [0, 1])
@pytest.mark.parametrize("cname,g2", GROUPS)
def test_long_span(gm_ctx, oracle, env, cname, g2, glv):
    """All scalars equal: one bucket over N / K slices (tree fixup over raw
    parts); every slice but the first lies inside it."""
    sc = [12345] * N
    lay = _Layout(cname, g2, sc, glv)
    assert lay.long() == [12344] == lay.fills_slice() == lay.starts_on_edge()
    _run(gm_ctx, oracle, env, cname, g2, sc, glv)
