"""The MSM at every window width and bucket-reduction shape.

Each window width c = 2..24 of gm_set_msm_window has its own reduction shape
(msm.hpp msm_seg_geom, msm_tree_geom: segment length L, LDS tree levels, points
per node Q) and its own split of the scalar into full and narrow windows
(msm_plan_geom), per curve, group and layout -- plain, GLV and shared-bucket
precomputed.  The reduction walks all W * 2^(c-1) buckets whatever n is, so one
MSM of a few thousand points per (group, layout, c) runs every shape; only the
plain cases at c = 23 and 24 whose buckets, nodes and offsets exceed 16 GiB are
left out (OMITTED; test_msm_geometry.EXPECTED_OMITTED names them).

Inputs of a case: structured scalars with one chosen digit +-b in one window,
for every window and the edge buckets of the reduction (1, 2, L - 1, L, L + 1,
nb/2, nb - 1, nb, the ends of the first tree group), then r - 1, 0, 1, then
2^12 + 37 random scalars over points with an infinity point, a duplicate and a
P, -P pair.  The expected value is the oracle's MSM of the same bytes (its
window is its own).  tests/test_msm_geometry.py (no GPU) checks that this case
list covers every class of the geometry and that the structured scalars reach
those buckets."""
import os
import time

import pytest

import pyref

pytestmark = pytest.mark.gpu

GROUPS = [("bn254", False), ("bn254", True), ("bls12377", False), ("bls12377", True),
          ("bls12381", False), ("bls12381", True)]
LAYOUTS = ("plain", "glv", "pre")
WIDTHS = tuple(range(2, 25))          # what gm_set_msm_window admits
N_RANDOM = (1 << 12) + 37
MEM_CAP = 16 << 30                    # bytes of buckets + nodes + offsets of one case
TRIM_ABOVE = 2 << 30                  # cases above this give their arena back (gm_trim)
FR_BITS = {"bn254": 254, "bls12377": 253, "bls12381": 255}
FP_LIMBS29 = {"bn254": 9, "bls12377": 14, "bls12381": 14}   # radix-2^29 limbs of a base field element


def xyzz_bytes(cname, g2):
    """sizeof(XYZZ<DF>): four coordinates of 4-byte limbs, two components in G2."""
    return 4 * 4 * FP_LIMBS29[cname] * (2 if g2 else 1)


def case_alloc_bytes(cname, g2, layout, c):
    """Buckets, two node buffers and offsets of one case, restated from msm_plan
    and msm_launch (the geometry report's bucket_bytes + node_bytes +
    offset_bytes; test_msm_geometry.py holds the two equal)."""
    bits = 127 if layout == "glv" else FR_BITS[cname]
    Wred = 1 if layout == "pre" else (bits + c) // c
    nb = 1 << (c - 1)
    L = 4
    while L < 32 and Wred * nb // (2 * L) >= (1 << 17):
        L *= 2
    L = min(L, nb)
    nseg = nb // L
    x = xyzz_bytes(cname, g2)
    return x * Wred * nb + 2 * x * 2 * Wred * nseg + 4 * (Wred * nb + 1)


def sweep_cases():
    """(cname, g2, layout, c) of the sweep and of the cases the memory cap leaves
    out.  The cap applies to the plain layout, whose c = 23 and 24 reach 21 to 41
    GB; GLV and precomputed cases all run (the largest, the BLS12-377 and
    BLS12-381 G2 GLV cases at c = 24, take 25 GB)."""
    run, omitted = [], []
    for cname, g2 in GROUPS:
        for layout in LAYOUTS:
            for c in WIDTHS:
                over = layout == "plain" and case_alloc_bytes(cname, g2, layout, c) > MEM_CAP
                (omitted if over else run).append((cname, g2, layout, c))
    return run, omitted


CASES, OMITTED = sweep_cases()


def geometry(cname, g2, layout, c, n):
    import gnark_mi355x as gm
    lay = {"plain": gm.TGEOM_PLAIN, "glv": gm.TGEOM_GLV, "pre": gm.TGEOM_PRECOMP}[layout]
    return gm.msm_geometry(cname, g2, n, c, lay)


# ---------------------------------------------------------------------------
# structured scalars
# ---------------------------------------------------------------------------
def window_geom(g, w):
    """Bit offset and width of window w (msm_impl.hpp window_geom)."""
    c, wn = g["c"], g["wn"]
    return w * c - max(0, w - wn), (c - 1 if w >= wn else c)


def edge_buckets(g, w):
    """Digit magnitudes (bucket b holds |d| = b) at the edges of the reduction of
    window w: the ends of the window, of the first segment and of the first tree
    group, and the largest digits of a narrow window."""
    nb, L = g["nb"], g["L"]
    _, cw = window_geom(g, w)
    top = 1 << (cw - 1)                      # largest digit of this window
    e = {1, 2, L - 1, L, L + 1, nb // 2, nb - 1, nb, top - 1, top}
    if g["levels"]:
        nt = (1 << g["lg"][0]) * L           # buckets of the first tree group
        e |= {nt - 1, nt, nt + 1}
    return sorted(b for b in e if 1 <= b <= top)


def glv_limit():
    """One-digit scalars below 2^126 split as (k, 0) on every curve: lambda of
    BLS12-377, r / b2 of BN254 and lambda / 2 of BLS12-381's balanced split lie
    above it (msm_impl.hpp GlvBn254, GlvBls377, GlvBls381; test_msm_geometry.py
    checks the last against tools/glv_constants.py)."""
    return 1 << 126


def one_digit_scalars(cname, layout, g):
    """[(w, sign, b, k)]: k recodes to the digit sign * b in window w (a negative
    digit is 2^cw - b there and carries +1 into window w + 1).  Left out: digits
    the window cannot hold, negative digits of the top window, and scalars at or
    above r (GLV: above glv_limit())."""
    r = pyref.CURVES[cname].r
    limit = glv_limit() if layout == "glv" else r
    out = []
    for w in range(g["W"]):
        off, cw = window_geom(g, w)
        for b in edge_buckets(g, w):
            k = b << off
            if k < limit:
                out.append((w, 1, b, k))
            k = ((1 << cw) - b) << off
            if b < (1 << (cw - 1)) and w + 1 < g["W"] and k < limit:
                out.append((w, -1, b, k))
    return out


def structured_scalars(cname, layout, g):
    """The structured prefix of a case: the one-digit scalars; for GLV also
    lambda times each positive one (the digits of the k2 half); then r - 1, 0, 1."""
    r = pyref.CURVES[cname].r
    ks = [k for _, _, _, k in one_digit_scalars(cname, layout, g)]
    if layout == "glv":
        lam = glv_lambda(cname)
        ks += [k * lam % r for _, s, _, k in one_digit_scalars(cname, layout, g) if s > 0]
    return ks + [r - 1, 0, 1]


_GLV = {}


def glv_constants(cname):
    if cname not in _GLV:
        import importlib.util
        spec = importlib.util.spec_from_file_location(
            "glv_constants", os.path.join(os.path.dirname(__file__), "..", "tools", "glv_constants.py"))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        derive = {"bn254": mod.derive, "bls12377": mod.derive_bls12377, "bls12381": mod.derive_bls12381}
        _GLV[cname] = (mod, derive[cname]())
    return _GLV[cname]


def glv_lambda(cname):
    return glv_constants(cname)[1]["lam"]


# ---------------------------------------------------------------------------
# inputs shared by the cases of a group
# ---------------------------------------------------------------------------
N_STRUCT_MAX = 4096
_shared = {}


def _group_inputs(ctx, cname, g2):
    """Host bytes: N_STRUCT_MAX points for the structured prefix, and the random
    tail (scalars, points) with the edge points of test_msm_gpu._edge_inputs."""
    import device_points
    import gnark_mi355x as gm
    key = (cname, g2)
    if key not in _shared:
        c = pyref.CURVES[cname]
        G = pyref.Group(c, g2)
        pbytes = gm.point_bytes(cname, g2)
        n = N_STRUCT_MAX + N_RANDOM
        K = ctx.random_scalars(cname, n, seed=0x5EED3000 + 2 * GROUPS.index(key))
        P = device_points.batch_mul_generator(ctx, cname, g2, K, n)
        S = ctx.random_scalars(cname, N_RANDOM, seed=0x5EED3001 + 2 * GROUPS.index(key))
        pb, sb = P.to_host(), bytearray(S.to_host())
        for b in (K, P, S):
            b.free()
        head, tail = pb[:N_STRUCT_MAX * pbytes], bytearray(pb[N_STRUCT_MAX * pbytes:])

        def pt(i):
            return bytes(tail[i * pbytes:(i + 1) * pbytes])

        def put(i, b):
            tail[i * pbytes:(i + 1) * pbytes] = b
        put(1, pyref.encode_point(c, None, g2))                      # an infinity point
        put(6, pt(5))                                                # a duplicate, same scalar
        sb[6 * 32:7 * 32] = sb[5 * 32:6 * 32]
        put(8, pyref.encode_point(c, G.neg(pyref.decode_point(c, pt(7), g2)), g2))  # P and -P
        sb[8 * 32:9 * 32] = sb[7 * 32:8 * 32]
        _shared[key] = (head, bytes(tail), bytes(sb))
    return _shared[key]


def case_inputs(ctx, cname, g2, layout, c):
    """(geometry, scalar bytes, point bytes, structured count) of one case."""
    import gnark_mi355x as gm
    cp = pyref.CURVES[cname]
    pbytes = gm.point_bytes(cname, g2)
    g = geometry(cname, g2, layout, c, N_RANDOM)   # the class does not depend on n (test_msm_geometry.py)
    ks = structured_scalars(cname, layout, g)
    ns = len(ks)
    assert ns <= N_STRUCT_MAX
    head, tail, stail = _group_inputs(ctx, cname, g2)
    sb = b"".join(pyref.encode_fr(cp, k) for k in ks) + stail
    pb = head[:ns * pbytes] + tail
    return g, sb, pb, ns


@pytest.mark.parametrize("cname,g2,layout,c", CASES,
                         ids=["%s-%s-%s-c%d" % (cn, "g2" if g2 else "g1", lay, c) for cn, g2, lay, c in CASES])
def test_msm_window_sweep(gm_ctx, oracle, cname, g2, layout, c):
    import gnark_mi355x as gm
    pbytes = gm.point_bytes(cname, g2)
    g, sb, pb, ns = case_inputs(gm_ctx, cname, g2, layout, c)
    n = ns + N_RANDOM
    assert g["c"] == c and len(sb) == 32 * n and len(pb) == pbytes * n
    prefixes = [n, ns] + ([ns + 1000] if layout == "pre" else [])
    exp = {m: oracle.msm(cname, g2, sb[:32 * m], pb[:pbytes * m]) for m in prefixes}
    S = gm_ctx.copy_to_device(sb)
    P = None
    t0 = time.perf_counter()
    try:
        if layout == "pre":
            P = gm_ctx.points_upload_precomputed(cname, pb, g2, c)
            got = {m: gm_ctx.msm_precomputed(cname, S, P, m, g2)[1] for m in prefixes}
        else:
            P = gm_ctx.copy_to_device(pb)
            gm_ctx.set_msm_window(c)
            gm_ctx.set_msm_glv(1 if layout == "glv" else 0)
            got = {m: gm_ctx.msm(cname, S, P, m, g2)[1] for m in prefixes}
    finally:
        gm_ctx.set_msm_window(0)
        gm_ctx.set_msm_glv(-1)
        S.free()
        if P is not None:
            P.free()
        if case_alloc_bytes(cname, g2, layout, c) > TRIM_ABOVE:
            gm_ctx.trim()
    print("device calls %.3f s" % (time.perf_counter() - t0))
    for m in prefixes:
        assert got[m] == exp[m], (cname, g2, layout, c, m, "L=%d lg=%s Q=%d wn=%d/%d" % (
            g["L"], g["lg"], g["Q"], g["wn"], g["W"]))


# ---------------------------------------------------------------------------
# the default windows above 2^20 at their real size
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("logn,c,L", [(21, 17, 4), (23, 19, 16)])
def test_msm_default_window_real_size(gm_ctx, oracle, logn, c, L):
    """BN254 G1 on the default path: 2^21 + 37 is the first size without the
    default GLV split (c = 17, the PLONK commits of a 2^22 circuit), 2^23 + 37
    takes c = 19 and segments of 16 buckets; each with its real sort geometry."""
    import gnark_mi355x as gm
    n = (1 << logn) + 37
    g = gm.msm_geometry("bn254", False, n, 0, gm.TGEOM_DEFAULT)
    assert (g["glv"], g["c"], g["L"]) == (0, c, L)
    S = gm_ctx.random_scalars("bn254", n, seed=0x5EED4000 + logn)
    K = gm_ctx.random_scalars("bn254", n, seed=0x5EED4100 + logn)
    P = gm_ctx.batch_mul_base("bn254", False, gm.generator("bn254"), K, n)
    K.free()
    try:
        t0 = time.perf_counter()
        got = gm_ctx.msm("bn254", S, P, n)[1]
        t1 = time.perf_counter()
        exp = oracle.msm("bn254", False, S.to_host(), P.to_host())
        print("msm %.3f s, oracle and readback %.3f s" % (t1 - t0, time.perf_counter() - t1))
        assert got == exp
    finally:
        S.free()
        P.free()
        gm_ctx.trim()
