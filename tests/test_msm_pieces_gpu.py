"""G1 MSMs accumulate a piece plan (MsmPlan in csrc/msm.hpp): every bucket of
len entries is cut into ceil(len / T) pieces of nearly equal length, the pieces
are sorted by length, one lane adds one piece, and the parts of a cut bucket are
merged from contiguous slots (serially up to FIX_SERIAL adds, by tree levels and
a redone reduction above that).

Scalars are built from their digits at a forced window of 8 bits: windows 0..7
only, digits 1..128, so they are below 2^64 -- the GLV split of such a scalar is
trivial (k1 = k, k2 = 0) and the same layout holds with the split on and off.
`_Plan` recomputes the piece plan on the CPU and every case asserts that its
input produces the layout it is meant to hit.  Every result is compared with the
CPU oracle as an affine point, bit for bit."""
import pytest

import pyref

pytestmark = pytest.mark.gpu

C = 8                    # forced window: 128 buckets per window
NB = 1 << (C - 1)
FIX_SERIAL = 8           # msm_impl.hpp: serial fixup up to this many adds per bucket
T_DEFAULT = 48           # capi.hip msm_piece_len: plans of at most 2^25 entries
WAVE = 64
N = 4096


def _scalar(digits):
    """digits: {window: d}, 1 <= d <= 128 (non-negative signed digits, no carry)."""
    k = 0
    for w, d in digits.items():
        assert 0 <= w < 8 and 1 <= d <= NB
        k |= d << (C * w)
    return k


def _digits(k):
    assert k < 1 << 64
    out = {}
    for w in range(8):
        d = (k >> (C * w)) & 0xFF
        assert d <= NB      # a larger value would become a negative digit with a carry
        if d:
            out[w] = d
    return out


class _Plan:
    """The piece plan of a scalar list at piece length T: bucket lengths, pieces
    per bucket, and the piece lengths in accumulation order (longest first)."""

    def __init__(self, scalars, T):
        self.T = T
        self.len = {}
        for k in scalars:
            for w, d in _digits(k).items():
                self.len[(w, d)] = self.len.get((w, d), 0) + 1
        self.p = {b: (n + T - 1) // T for b, n in self.len.items()}
        self.pieces = []
        for b, n in self.len.items():
            p = self.p[b]
            q, r = divmod(n, p)
            self.pieces += [q + 1] * r + [q] * (p - r)
        self.pieces.sort(reverse=True)
        assert all(1 <= x <= T for x in self.pieces)

    def cut(self):       # merged serially by k_msm_fixup
        return [b for b, p in self.p.items() if 2 <= p <= FIX_SERIAL + 1]

    def long(self):      # k_msm_fix_tree levels, k_msm_fixup_long, redone reduction
        return [b for b, p in self.p.items() if p > FIX_SERIAL + 1]

    def whole(self):     # stored by the accumulation itself
        return [b for b, p in self.p.items() if p == 1]

    def mixed_waves(self):
        return [i for i in range(0, len(self.pieces), WAVE) if len(set(self.pieces[i:i + WAVE])) > 1]

    def windows(self):
        return {w for w, _ in self.len}


@pytest.fixture(scope="module")
def env(gm_ctx, oracle):
    """Per curve: N random G1 points as host bytes, a larger MSM of another shape
    to dirty the workspace, and a cache of oracle results per (scalars, points)."""
    import device_points
    import gnark_mi355x as gm
    st, exp = {}, {}

    def get(cname):
        if cname not in st:
            n_big = (1 << 13) + 37
            K = gm_ctx.random_scalars(cname, n_big, seed=0xC0)
            P = device_points.batch_mul_generator(gm_ctx, cname, False, K, n_big)
            S = gm_ctx.random_scalars(cname, n_big, seed=0xC8)
            K.free()
            st[cname] = (S, P, n_big, P.to_host()[: N * gm.point_bytes(cname, False)])
        return st[cname]

    def expected(cname, sb, pb):
        key = (cname, sb, pb)
        if key not in exp:
            exp[key] = oracle.msm(cname, False, sb, pb)
        return exp[key]

    yield get, expected
    for S, P, _, _ in st.values():
        S.free()
        P.free()


def _run(gm_ctx, env, cname, scalars, T, glv=0, points=None, precomputed=False, dirty=False, window=C, twice=False):
    import gnark_mi355x as gm
    get, expected = env
    S_big, P_big, n_big, pts = get(cname)
    n = len(scalars)
    c = pyref.CURVES[cname]
    pb = points if points is not None else pts[: n * gm.point_bytes(cname, False)]
    sb = b"".join(pyref.encode_fr(c, k) for k in scalars)
    exp = expected(cname, sb, pb)
    S = gm_ctx.copy_to_device(sb)
    P = gm_ctx.points_upload_precomputed(cname, pb, False, 0) if precomputed else gm_ctx.copy_to_device(pb)
    try:
        if dirty:
            gm_ctx.msm(cname, S_big, P_big, n_big, False)
        gm_ctx.set_msm_piece_len(T)
        got = []
        for _ in range(2 if twice else 1):
            if precomputed:
                got.append(gm_ctx.msm_precomputed(cname, S, P, n, g2=False)[1])
            else:
                gm_ctx.set_msm_window(window)
                gm_ctx.set_msm_glv(glv)
                got.append(gm_ctx.msm(cname, S, P, n, False)[1])
    finally:
        gm_ctx.set_msm_piece_len(0)
        gm_ctx.set_msm_window(0)
        gm_ctx.set_msm_glv(-1)
        S.free()
        P.free()
    for g in got:
        assert g == exp
    return got


def _uniform(n, digits_hi, seed, windows=8):
    """n scalars whose digits of `windows` windows are uniform in 1..digits_hi."""
    import random
    rng = random.Random(seed)
    return [_scalar({w: rng.randint(1, digits_hi) for w in range(windows)}) for _ in range(n)]


@pytest.mark.parametrize("T", [4, 24, 0])
@pytest.mark.parametrize("glv", [0, 1])
def test_many_pieces_per_bucket(gm_ctx, env, glv, T):
    """64 entries per bucket on average: at T = 4 every bucket has more parts than
    the serial fixup takes (tree levels, the reduction redone after the max-parts
    readback); at 24 it has 2 to 4 parts, merged serially; at the default some
    buckets are whole and the others two parts."""
    sc = _uniform(N, 64, seed=1)
    plan = _Plan(sc, T or T_DEFAULT)
    assert len(plan.len) == 8 * 64 and min(plan.len.values()) >= 37
    if T == 4:
        assert len(plan.long()) == len(plan.len) and not plan.cut()
    else:
        assert plan.cut() and not plan.long()
        assert {plan.p[b] for b in plan.len} >= ({2, 3} if T else {1, 2})
        assert T == 0 or len(plan.cut()) == len(plan.len)
    _run(gm_ctx, env, "bn254", sc, T, glv)


@pytest.mark.parametrize("T", [24, 0])
@pytest.mark.parametrize("glv", [0, 1])
def test_one_huge_bucket(gm_ctx, env, glv, T):
    """All scalars equal: one bucket of n entries, n / T parts through the tree
    levels, found only by the readback (uniform scalars would have none)."""
    sc = [5] * N
    plan = _Plan(sc, T or T_DEFAULT)
    assert plan.long() == [(0, 5)] and plan.p[(0, 5)] == -(-N // (T or T_DEFAULT))
    _run(gm_ctx, env, "bn254", sc, T, glv)


@pytest.mark.parametrize("T", [4, 0])
def test_huge_bucket_among_uniform_ones(gm_ctx, env, T):
    sc = _uniform(N // 2, 64, seed=2) + [_scalar({0: 7, 3: 9})] * (N // 2)
    plan = _Plan(sc, T or T_DEFAULT)
    assert {(0, 7), (3, 9)} <= set(plan.long()) and plan.p[(0, 7)] > 4 * FIX_SERIAL
    assert plan.whole() if T == 0 else len(plan.long()) > 2
    _run(gm_ctx, env, "bn254", sc, T, glv=0)


def _sparse_scalars():
    """Mostly zero; 60 scalars with one small digit in window 0 or 2: single-entry
    buckets, a few of two and three entries, window 1 and 3..7 empty."""
    sc = [0] * N
    for j in range(40):
        sc[17 + 97 * j] = _scalar({0 if j % 2 else 2: 1 + j})          # 40 buckets of one entry
    for j in range(20):
        sc[5 + 201 * j] = _scalar({0: 100 + j // 3}) if j < 12 else _scalar({2: 90 + (j - 12) // 2})
    return sc


@pytest.mark.parametrize("mode", ["plain", "glv", "precomputed"])
def test_sparse_plan_in_dirty_arena(gm_ctx, env, mode):
    """After a larger MSM on the same context: empty buckets must read as infinity
    although their memory holds the other MSM's sums, and every non-empty bucket
    -- most of them one entry: a copy and a store, no add -- must be written."""
    sc = _sparse_scalars()
    plan = _Plan(sc, T_DEFAULT)
    assert plan.windows() == {0, 2} and not plan.cut() and not plan.long()
    assert sorted(set(plan.len.values())) == [1, 2, 3] and plan.pieces.count(1) >= 40
    assert len(plan.pieces) % WAVE
    _run(gm_ctx, env, "bn254", sc, 0, glv=int(mode == "glv"), precomputed=mode == "precomputed", dirty=True)


@pytest.mark.parametrize("T", [1, 4, 0])
@pytest.mark.parametrize("glv", [0, 1])
def test_group_law_edges(gm_ctx, env, glv, T):
    """Buckets whose content decides the add's branch whatever order the sort
    leaves: {P, P} (a doubling inside a piece; at T = 1 two parts with equal sums,
    so the fixup doubles), {P, -P} (infinity inside a piece; at T = 1 two opposite
    parts), 2 T' equal points (parts with equal sums at T' = 4), infinity points
    alone, among others, and as a whole piece."""
    import gnark_mi355x as gm
    cname = "bn254"
    c = pyref.CURVES[cname]
    G = pyref.Group(c, False)
    pbytes = gm.point_bytes(cname, False)
    n = 256
    pts = bytearray(env[0](cname)[3][: n * pbytes])
    P0, P1 = bytes(pts[:pbytes]), bytes(pts[pbytes:2 * pbytes])
    N1 = pyref.encode_point(c, G.neg(pyref.decode_point(c, P1, False)), False)
    INF = bytes(pbytes)
    sc, i = [], 0

    def put(point, d, w=0):
        nonlocal i
        if point is not None:
            pts[i * pbytes:(i + 1) * pbytes] = point
        sc.append(_scalar({w: d}))
        i += 1

    put(P0, 1), put(P0, 1)                      # doubling
    put(P1, 2), put(N1, 2)                      # P - P
    put(P1, 3), put(N1, 3), put(None, 3)        # P - P and one more
    for _ in range(8):
        put(P0, 4)                              # 8 equal points: equal parts at T = 4
    for _ in range(4):
        put(P1, 5), put(N1, 5)                  # sums to infinity over two parts at T = 4
    put(INF, 6)                                 # a piece that is one infinity point
    put(INF, 7), put(None, 7)                   # infinity beside a point
    put(INF, 8), put(INF, 8), put(INF, 8)       # only infinity points
    for _ in range(5):
        put(INF, 9), put(None, 9)               # infinity points among others, over parts
    while i < n:
        put(None, 20 + i % 50, w=1)
    plan = _Plan(sc, T or T_DEFAULT)
    assert [plan.len[(0, d)] for d in range(1, 10)] == [2, 2, 3, 8, 8, 1, 2, 3, 10]
    if T == 1:
        assert plan.p[(0, 1)] == 2 == plan.p[(0, 2)] and plan.p[(0, 9)] == 10 and (0, 9) in plan.long()
    elif T == 4:
        assert plan.p[(0, 4)] == 2 == plan.p[(0, 5)] and plan.p[(0, 1)] == 1 and plan.p[(0, 9)] == 3
    else:
        assert not plan.cut() and not plan.long()
    _run(gm_ctx, env, cname, sc, T, glv, points=bytes(pts))


@pytest.mark.parametrize("T", [4, 0])
def test_wave_shape(gm_ctx, env, T):
    """A piece count that is no multiple of the wave size, and waves whose lanes
    hold pieces of two lengths (they loop to the longest)."""
    sc = _uniform(1000, 13, seed=3, windows=6) + [_scalar({7: 3})] * 5
    plan = _Plan(sc, T or T_DEFAULT)
    assert len(plan.pieces) % WAVE and len(plan.pieces) > 2 * WAVE
    assert plan.mixed_waves() and len(set(plan.pieces)) >= 3
    _run(gm_ctx, env, "bn254", sc, T)


@pytest.mark.parametrize("T", [4, 0])
def test_bls12377_g1(gm_ctx, env, T):
    """The prefetching body (14-limb field)."""
    sc = _uniform(2048, 32, seed=4) + []
    plan = _Plan(sc, T or T_DEFAULT)
    assert plan.long() if T == 4 else plan.cut()
    _run(gm_ctx, env, "bls12377", sc, T, dirty=True)


@pytest.mark.parametrize("T", [4, 0])
def test_bls12381_g1(gm_ctx, env, T):
    """The same body over BLS12-381's 14-limb field (curve id 2)."""
    sc = _uniform(2048, 32, seed=4) + []
    plan = _Plan(sc, T or T_DEFAULT)
    assert plan.long() if T == 4 else plan.cut()
    _run(gm_ctx, env, "bls12381", sc, T, dirty=True)


@pytest.mark.parametrize("T", [4, 0])
def test_precomputed_shared_buckets(gm_ctx, env, T):
    """One bucket set shared by all windows (the library picks the window)."""
    sc = _uniform(2048, 64, seed=5)
    _run(gm_ctx, env, "bn254", sc, T, precomputed=True)


def test_full_width_scalars(gm_ctx, env):
    """Random scalars of the whole field (negative digits, carries, the GLV split
    proper) at the automatic window, default and small piece length."""
    get, _ = env
    c = pyref.CURVES["bn254"]
    import random
    rng = random.Random(6)
    sc = [rng.randrange(c.r) for _ in range(1024)]
    for T in (0, 3):
        for glv in (0, 1):
            _run(gm_ctx, env, "bn254", sc, T, glv, window=0)


def test_repeatable(gm_ctx, env):
    sc = _uniform(N, 64, seed=1)
    a, b = _run(gm_ctx, env, "bn254", sc, 0, glv=1, twice=True)
    assert a == b


def test_piece_len_setter_bounds(gm_ctx):
    import gnark_mi355x as gm
    L = gm.load_library()
    assert L.gm_set_msm_piece_len(gm_ctx.handle, 129) != 0
    assert L.gm_set_msm_piece_len(gm_ctx.handle, -1) != 0
    assert L.gm_set_msm_piece_len(gm_ctx.handle, 128) == 0
    assert L.gm_set_msm_piece_len(gm_ctx.handle, 0) == 0
