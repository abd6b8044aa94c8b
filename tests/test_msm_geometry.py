"""The MSM's derived geometry on the host (no GPU): the report
gm_test_msm_geometry calls the functions the driver calls (msm.hpp
msm_plan_geom, msm_seg_geom, msm_tree_geom).  Checked here: the class table of
every curve, group, layout and window width; that the GPU sweep
(test_msm_windows_gpu.CASES) holds every class but the seven the 16 GiB cap
leaves out; that every default choice of window lies inside the sweep; and,
with a Python restatement of the signed-digit recoding, that the sweep's
structured scalars reach the edge buckets of every window."""
import pytest

import gnark_mi355x as gm
import pyref
import test_msm_windows_gpu as sweep

ALL = [(cn, g2, lay, c) for cn, g2 in sweep.GROUPS for lay in sweep.LAYOUTS for c in sweep.WIDTHS]
# what the cap leaves out, from sizeof(XYZZ): 144 B (BN254 G1), 288, 224, 448 B per bucket; BLS12-381 has
# BLS12-377's 14 limbs and, at c = 23 and 24, its window counts (12 and 11), hence the same three cases
EXPECTED_OMITTED = {("bn254", True, "plain", 24), ("bls12377", False, "plain", 24),
                    ("bls12377", True, "plain", 24), ("bls12377", True, "plain", 23),
                    ("bls12381", False, "plain", 24), ("bls12381", True, "plain", 24),
                    ("bls12381", True, "plain", 23)}


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
    assert all(lay == "plain" and c in (23, 24) for _, _, lay, c in omitted)
    assert {k for k in omitted if k[0] == "bls12381"} == {
        (cn, g2, lay, c) for cn, g2, lay, c in ALL
        if cn == "bls12381" and lay == "plain" and sweep.case_alloc_bytes(cn, g2, lay, c) > sweep.MEM_CAP}
    # one GLV case per 14-limb curve lies above the cap too (6 windows of 2^23 buckets of 448 B); they run
    assert [k for k, _ in over] == [("bls12377", True, "glv", 24), ("bls12381", True, "glv", 24)]
    assert all(alloc < 32 << 30 for _, alloc in over)
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
    """Signed (k1, k2) with k = k1 + k2 lambda mod r, as the device computes them
    (tools/glv_constants.py): k1 >= 0 on BN254, both >= 0 on BLS12-377, either
    sign for both on BLS12-381."""
    mod, d = sweep.glv_constants(cname)
    if cname == "bls12381":
        k1, n1, k2, n2 = mod.split_bls12381(k, d)
        return (-k1 if n1 else k1), (-k2 if n2 else k2)
    return mod.split(k, d) if cname == "bn254" else mod.split_bls12377(k, d)


def digits(cname, layout, g, k):
    """(window, signed digit) of every non-zero digit the kernel derives from scalar k."""
    if layout != "glv":
        return [(w, d) for w, d in enumerate(recode(k, g)) if d]
    k1, k2 = glv_split(cname, k)
    assert abs(k1) < 1 << 127 and abs(k2) < 1 << 127 and (k1 >= 0 or cname == "bls12381")
    out = [(w, d if k1 >= 0 else -d) for w, d in enumerate(recode(abs(k1), g)) if d]
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


# ---------------------------------------------------------------------------
# BLS12-381: the GLV limit and the top window of a 255-bit scalar
# ---------------------------------------------------------------------------
def test_bls12381_scalars_below_the_glv_limit_split_trivially(table):
    """The balanced split of BLS12-381 (tools/glv_constants.split_bls12381) rounds
    k1 up only above (lambda - 1) / 2 and flips only above (r - 1) / 2; both lie
    above glv_limit() = 2^126, so every one-digit scalar of the GLV cases splits
    as (k, 0) with no sign on either half, as on the other curves."""
    mod, d = sweep.glv_constants("bls12381")
    lim = sweep.glv_limit()
    assert lim == 1 << 126 and d["lam"] >> 1 >= lim and d["half"] >= lim
    ks = {0, 1, 2, lim - 1, lim >> 1, (lim >> 1) + 1}
    for c in sweep.WIDTHS:
        ks.update(k for _, _, _, k in sweep.one_digit_scalars("bls12381", "glv", table[("bls12381", False, "glv", c)]))
    assert len(ks) > 1000 and max(ks) < lim
    for k in ks:
        assert mod.split_bls12381(k, d) == (k, 0, 0, 0), k
        assert glv_split("bls12381", k) == (k, 0)
    # the first scalar that does not: k1 rounds up to -(lambda - 1) / 2
    assert mod.split_bls12381((d["lam"] >> 1) + 1, d) == (d["lam"] >> 1, 1, 1, 0)


@pytest.mark.parametrize("g2", [False, True])
def test_bls12381_top_window_at_widths_dividing_255(table, g2):
    """255 = 3 * 5 * 17: at c = 3, 5, 15 and 17 the windows below the top one
    would hold all 255 bits of the scalar and leave the top window the carry
    alone.  The plans cover bits + 1 = 256 bits exactly, so that happens only
    where no window is narrowed: the plain layout at c = 17 (16 windows of 17
    bits, excess 16 = W; msm_plan_geom narrows only below W), whose top window
    starts at bit 255.  At c = 3, 5 and 15, and in the shared-bucket layout at
    all four, the narrow windows pull the top window down to bit 254 or below,
    so it holds scalar bits as well as the carry.  Either way the sweep's structured scalars reach digit 1
    of the top window through a carry out of a negative digit below it, which is
    the only way into a carry-only window; r - 1 is one of them."""
    cname, r = "bls12381", pyref.CURVES["bls12381"].r
    carry_only = set()
    for layout in ("plain", "pre"):
        for c in (3, 5, 15, 17):
            g = table[(cname, g2, layout, c)]
            W = g["W"]
            assert W == 255 // c + 1
            off, cw = sweep.window_geom(g, W - 1)
            assert off + cw >= 256
            if off >= 255:
                carry_only.add((layout, c))
                assert (g["narrow"], off, cw) == (0, 255, c)
            else:
                assert g["narrow"] == (c - 1 if c - 1 < W else W - 1) and off <= 254
            by_carry = [k for k in sweep.structured_scalars(cname, layout, g)
                        if k >> off == 0 and dict(digits(cname, layout, g, k)).get(W - 1) == 1]
            assert by_carry, (layout, c)
            assert all(dict(digits(cname, layout, g, k))[W - 2] < 0 for k in by_carry)
            top = dict(digits(cname, layout, g, r - 1)).get(W - 1)
            assert top == 1 if off >= 255 else top >= 1, (layout, c, top)
    assert carry_only == {("plain", 17)}
    # no other curve has a carry-only top window at these widths
    for cn, g2_ in sweep.GROUPS:
        for layout in ("plain", "pre"):
            for c in (3, 5, 15, 17):
                g = table[(cn, g2_, layout, c)]
                off, _ = sweep.window_geom(g, g["W"] - 1)
                assert (off >= sweep.FR_BITS[cn]) == ((cn, layout, c) == ("bls12381", "plain", 17))
