"""The MSM's derived geometry on the host (no GPU): the report
gm_test_msm_geometry calls the functions the driver calls (msm.hpp
msm_plan_geom, msm_seg_geom, msm_tree_geom).  Checked here: the class table of
every curve, group, layout and window width; that the GPU sweep
(test_msm_windows_gpu.CASES) holds every class but the four the 16 GiB cap
leaves out; that every default choice of window lies inside the sweep; and,
with a Python restatement of the signed-digit recoding, that the sweep's
structured scalars reach the edge buckets of every window."""
import pytest

import gnark_mi355x as gm
import pyref
import test_msm_windows_gpu as sweep

ALL = [(cn, g2, lay, c) for cn, g2 in sweep.GROUPS for lay in sweep.LAYOUTS for c in sweep.WIDTHS]
# what the cap leaves out, from sizeof(XYZZ): 144 B (BN254 G1), 288, 224, 448 B per bucket
EXPECTED_OMITTED = {("bn254", True, "plain", 24), ("bls12377", False, "plain", 24),
                    ("bls12377", True, "plain", 24), ("bls12377", True, "plain", 23)}


def klass(g):
    """What makes two MSMs run the same reduction and digit layout."""
    return (g["W"], g["wn"], g["narrow"], g["L"], g["lg"], g["Q"])


@pytest.fixture(scope="module")
def table():
    return {k: sweep.geometry(*k, sweep.N_RANDOM) for k in ALL}


def test_report_fields_are_consistent(table):
    for (cname, g2, layout, c), g in table.items():
        assert g["c"] == c and g["nb"] == 1 << (c - 1) and g["total"] == g["Wred"] * g["nb"]
        assert g["Wred"] == (1 if layout == "pre" else g["W"])
        assert (g["glv"], g["shared"]) == (int(layout == "glv"), int(layout == "pre"))
        assert g["bits"] == (127 if layout == "glv" else sweep.FR_BITS[cname])
        assert g["W"] == -(-(g["bits"] + 1) // c) and g["narrow"] == g["W"] - g["wn"] < g["W"]
        # the windows cover bits + 1 bits; the excess is spread one bit per window: the precomputed
        # layout up to W - 1 windows (precomp_narrow), the plain one only when it is below W, GLV never
        excess = c * g["W"] - (g["bits"] + 1)
        assert 0 <= excess < c
        assert g["narrow"] == {"glv": 0, "pre": min(excess, g["W"] - 1),
                               "plain": excess if excess < g["W"] else 0}[layout]
        assert g["L"] * g["nseg"] == g["nb"] and g["L"] in (g["nb"], 4, 8, 16, 32)
        assert 1 << sum(g["lg"]) == g["nseg"] and g["Q"] == 2 + sum(g["lg"]) and len(g["lg"]) == g["levels"]
        assert g["xyzz_bytes"] == sweep.xyzz_bytes(cname, g2)
        assert g["n"] == sweep.N_RANDOM * (2 if layout == "glv" else 1) and g["M"] == g["W"] * g["n"]
        assert g["NS"] <= 8192 and g["NC"] == -(-g["total"] // (1 << g["F"]))
        # every level fits the LDS budget and two tasks per thread (msm_tree_geom)
        Q = 2
        for lg in g["lg"]:
            assert (2 << (lg - 1)) * Q * g["xyzz_bytes"] <= 96 << 10 and (1 << (lg - 1)) * (Q + 1) <= 512
            Q += lg
        assert (g["bucket_bytes"] + g["node_bytes"] + g["offset_bytes"]
                == sweep.case_alloc_bytes(cname, g2, layout, c))


def test_class_does_not_depend_on_n(table):
    """The sweep runs each class at a few thousand points: W, the narrow windows,
    L and the tree come from c, the scalar bits and sizeof(XYZZ) alone."""
    for k, g in table.items():
        for n in (1, 1 << 20):
            assert klass(sweep.geometry(*k, n)) == klass(g), (k, n)


def test_sweep_covers_every_class(table):
    run, omitted = set(sweep.CASES), set(sweep.OMITTED)
    assert len(sweep.CASES) == len(run) and not run & omitted and run | omitted == set(ALL)
    classes = {}
    for (cname, g2, layout, c), g in table.items():
        classes.setdefault((cname, g2, layout), {})[c] = klass(g)
    print("class table: %d (curve, group, layout, c) entries" % len(table))
    for key, per_c in classes.items():
        # every width is its own class: no width can stand in for another
        assert len(set(per_c.values())) == len(sweep.WIDTHS), key
        shapes = sorted({(k[3], len(k[4])) for k in per_c.values()})
        print(" ", key, "(L, levels):", shapes)
    over = []
    for k, g in table.items():
        alloc = g["bucket_bytes"] + g["node_bytes"] + g["offset_bytes"]
        # the only exception: a reported allocation above 16 GiB
        assert k in run or alloc > sweep.MEM_CAP, k
        if k in run and alloc > sweep.MEM_CAP:
            over.append((k, alloc))
    print("left out by the 16 GiB cap:", sorted(omitted))
    print("run although above it:", over)
    assert omitted <= EXPECTED_OMITTED, sorted(omitted - EXPECTED_OMITTED)
    assert omitted == EXPECTED_OMITTED
    # one GLV case lies above the cap too (6 windows of 2^23 buckets of 448 B); it runs
    assert [k for k, _ in over] == [("bls12377", True, "glv", 24)] and over[0][1] < 32 << 30
    # the shapes the suite did not run before: L = 8 and 16, no tree at all, four-level G2 trees
    Ls = {(k[2], g["L"]) for k, g in table.items() if k in run}
    assert {(lay, L) for lay in sweep.LAYOUTS for L in (2, 4, 8, 16, 32)} <= Ls
    assert table[("bn254", False, "plain", 18)]["L"] == 8 and table[("bn254", False, "plain", 19)]["L"] == 16
    assert table[("bn254", False, "pre", 21)]["L"] == 8 and table[("bn254", False, "pre", 22)]["L"] == 16
    assert all(table[("bn254", False, "plain", c)]["levels"] == 0 for c in (2, 3))
    assert max(g["levels"] for k, g in table.items() if k in run and k[1]) >= 4


def test_default_choices_are_inside_the_sweep():
    """n = 2^k and 2^k + 1 up to the plan's own limits: the window the cost model
    takes (with the default GLV switch at 2^21) and the one msm_choose_precomp
    takes are cases of the sweep -- none is left out by the memory cap."""
    run = set(sweep.CASES)
    seen = set()
    for cname, g2 in sweep.GROUPS:
        accepted = 0
        for k in range(31):
            for n in ((1 << k), (1 << k) + 1):
                try:
                    g = gm.msm_geometry(cname, g2, n, 0, gm.TGEOM_DEFAULT)
                except gm.GmError:
                    assert n * 32 >= 1 << 31    # refused only by n * W < 2^31; W <= 32 at c >= 8
                else:
                    accepted += 1
                    assert g["glv"] == int(n <= 1 << 21)
                    key = (cname, g2, "glv" if g["glv"] else "plain", g["c"])
                    assert key in run, (key, n)
                    seen.add(key)
                try:
                    g = gm.msm_geometry(cname, g2, n, 0, gm.TGEOM_PRECOMP)
                except gm.GmError:
                    assert n * 32 >= 1 << 31    # copies * n < 2^31, at most 32 copies (c >= 8)
                else:
                    assert 8 <= g["c"] <= 24 and (cname, g2, "pre", g["c"]) in run, (g["c"], n)
                    seen.add((cname, g2, "pre", g["c"]))
        assert accepted >= 50
    d = gm.msm_geometry("bn254", False, (1 << 21) + 37, 0, gm.TGEOM_DEFAULT)
    assert (d["glv"], d["c"]) == (0, 17)
    d = gm.msm_geometry("bn254", False, 1 << 22, 0, gm.TGEOM_DEFAULT)
    assert (d["glv"], d["c"]) == (0, 17)
    d = gm.msm_geometry("bn254", False, (1 << 23) + 37, 0, gm.TGEOM_DEFAULT)
    assert (d["glv"], d["c"], d["L"]) == (0, 19, 16)
    print("default choices:", len(seen), "cases of the sweep")


def test_report_refuses_what_the_plan_refuses():
    with pytest.raises(gm.GmError):
        gm.msm_geometry("bn254", False, 1 << 31, 16, gm.TGEOM_PLAIN)
    with pytest.raises(gm.GmError, match="windows"):
        gm.msm_geometry("bn254", False, 1 << 28, 8, gm.TGEOM_PLAIN)
    for c in (1, 25, -3):
        with pytest.raises(gm.GmError):
            gm.msm_geometry("bn254", False, 1000, c, gm.TGEOM_PLAIN)
        with pytest.raises(gm.GmError):
            gm.msm_geometry("bn254", False, 1000, c, gm.TGEOM_PRECOMP)
    with pytest.raises(gm.GmError):
        gm.msm_geometry("bn254", False, 0, 16, gm.TGEOM_PLAIN)
    with pytest.raises(gm.GmError):
        gm.msm_geometry("bn254", False, 1000, 16, 4)


# ---------------------------------------------------------------------------
# the structured scalars reach the edge buckets
# ---------------------------------------------------------------------------
def recode(k, g):
    """Signed digits of k, one per window (msm_impl.hpp k_msm_digits, emit_digits):
    a raw digit above half the window's range becomes negative and carries."""
    out, carry = [], 0
    for w in range(g["W"]):
        off, cw = sweep.window_geom(g, w)
        raw = ((k >> off) & ((1 << cw) - 1)) + carry
        if raw > 1 << (cw - 1):
            out.append(raw - (1 << cw))
            carry = 1
        else:
            out.append(raw)
            carry = 0
    assert carry == 0 and k >> (sweep.window_geom(g, g["W"] - 1)[0] + sweep.window_geom(g, g["W"] - 1)[1]) == 0
    return out


def glv_split(cname, k):
    """(k1, k2) with k = k1 + k2 lambda, as the device computes them (tools/glv_constants.py)."""
    mod, d = sweep.glv_constants(cname)
    return mod.split(k, d) if cname == "bn254" else mod.split_bls12377(k, d)


def digits(cname, layout, g, k):
    """(window, signed digit) of every non-zero digit the kernel derives from scalar k."""
    if layout != "glv":
        return [(w, d) for w, d in enumerate(recode(k, g)) if d]
    k1, k2 = glv_split(cname, k)
    assert 0 <= k1 < 1 << 127 and abs(k2) < 1 << 127
    out = [(w, d) for w, d in enumerate(recode(k1, g)) if d]
    return out + [(w, d if k2 >= 0 else -d) for w, d in enumerate(recode(abs(k2), g)) if d]


def required_edges(g, w):
    """The issue's list for window w, as bucket numbers b = |digit|: 1, 2, L - 1, L,
    L + 1, nb/2, nb - 1, nb and the first and last bucket of the first tree group;
    a bucket above the window's largest digit does not exist."""
    _, cw = sweep.window_geom(g, w)
    e = {1, 2, g["L"] - 1, g["L"], g["L"] + 1, g["nb"] // 2, g["nb"] - 1, g["nb"]}
    if g["levels"]:
        e.add((1 << g["lg"][0]) * g["L"])
    return {b for b in e if 1 <= b <= 1 << (cw - 1)}


@pytest.mark.parametrize("cname,g2", sweep.GROUPS)
def test_structured_scalars_reach_the_edges(table, cname, g2):
    r = pyref.CURVES[cname].r
    total = 0
    for layout in sweep.LAYOUTS:
        limit = sweep.glv_limit() if layout == "glv" else r
        for c in sweep.WIDTHS:
            g = table[(cname, g2, layout, c)]
            W = g["W"]
            for w, s, b, k in sweep.one_digit_scalars(cname, layout, g):
                ds = dict(digits(cname, layout, g, k))
                assert ds.get(w) == s * b and set(ds) <= {w, w + 1}, (layout, c, w, s, b)
            ks = sweep.structured_scalars(cname, layout, g)
            assert len(ks) <= sweep.N_STRUCT_MAX and ks[-3:] == [r - 1, 0, 1]
            reached = set()
            for k in ks:
                reached.update(digits(cname, layout, g, k))
            total += len(ks)
            for w in range(W):
                off, cw = sweep.window_geom(g, w)
                for b in required_edges(g, w):
                    if (b << off) < limit:
                        assert (w, b) in reached, (layout, c, w, b)
                    else:
                        assert w == W - 1          # only the top window is cut short by the scalar's range
                    # a negative digit: not the window's largest (2^(cw-1) stays positive), not in the top
                    # window (nothing above it takes the carry), and the scalar stays in range
                    if b < 1 << (cw - 1) and w + 1 < W:
                        if (((1 << cw) - b) << off) < limit:
                            assert (w, -b) in reached, (layout, c, w, -b)
                        else:
                            assert w >= W - 2
            if layout == "glv":   # the k2 half is filled too, with both signs on BN254
                k2_digits = set()
                for k in ks[:-3]:
                    k1, k2 = glv_split(cname, k)
                    if k2:
                        k2_digits.update((w, d if k2 > 0 else -d) for w, d in enumerate(recode(abs(k2), g)) if d)
                assert {w for w, _ in k2_digits} >= set(range(W - 1)), (c, sorted(k2_digits)[:4])
    print(cname, "g2" if g2 else "g1", "structured scalars over all cases:", total)
