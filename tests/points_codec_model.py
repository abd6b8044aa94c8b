"""gnark-crypto's point encodings in Python integers: the model the device codec
(gm_points_decode / gm_points_encode) is tested against.

A coordinate is 8 * fp_limbs bytes, big-endian, canonical.  G1: X or X || Y; G2:
X.A1 || X.A0 or X.A1 || X.A0 || Y.A1 || Y.A0.  The flag is the top bits of the
first byte (BN254 two bits, the BLS12 curves three).  Roots come from
tools/subgroup_constants.py (sqrt_fp / sqrt_fp2), the curve and subgroup verdicts
from points_check_cases.classify.  A point is an affine tuple of integers (G2:
((x0, x1), (y0, y1))), None the infinity."""
import functools

import points_check_cases as pc
from points_check_cases import sub

OK, NOT_REDUCED, OFF_CURVE, OFF_SUBGROUP, BAD_ENCODING, NO_ROOT = range(6)
COMPRESSED, RAW = 0, 1
NO_SUBGROUP_CHECK = 0x100
REPORT_KEYS = ("not_reduced", "off_curve", "off_subgroup", "bad_encoding", "no_root")


def is_bn(cname):
    return cname == "bn254"


def flag_bits(cname):
    return 2 if is_bn(cname) else 3


def fp_bytes(c):
    return 8 * c.fp_limbs


def record_bytes(c, g2, width):
    return fp_bytes(c) * (2 if g2 else 1) * (2 if width == RAW else 1)


def larger_fp(c, y):
    """LexicographicallyLargest on Fp."""
    return y % c.p > (c.p - 1) // 2


def larger(c, g2, y):
    if not g2:
        return larger_fp(c, y)
    return larger_fp(c, y[1]) if y[1] % c.p else larger_fp(c, y[0])


def components(P, g2, width):
    """The integers of a record in its order: X [, Y]; G2: A1 before A0."""
    coords = P[:2] if width == RAW else P[:1]
    return [v for co in coords for v in ((co[1], co[0]) if g2 else (co,))]


def with_flag(cname, body, flag):
    b = bytearray(body)
    b[0] |= flag << (8 - flag_bits(cname))
    return bytes(b)


def flag_of_point(cname, width, is_larger):
    if width == RAW:
        return 0
    return (0b10 if is_bn(cname) else 0b100) | int(is_larger)


def flag_of_infinity(cname, width):
    if is_bn(cname):
        return 0b00 if width == RAW else 0b01
    return 0b010 if width == RAW else 0b110


def encode(cname, g2, P, width):
    c = pc.params(cname)
    if P is None:
        return with_flag(cname, bytes(record_bytes(c, g2, width)), flag_of_infinity(cname, width))
    body = b"".join((v % c.p).to_bytes(fp_bytes(c), "big") for v in components(P, g2, width))
    return with_flag(cname, body, flag_of_point(cname, width, larger(c, g2, P[1])))


def split(cname, rec):
    """(flag, the record's integers with the flag bits cleared)."""
    c = pc.params(cname)
    fb, k = fp_bytes(c), flag_bits(cname)
    flag = rec[0] >> (8 - k)
    body = bytes([rec[0] & ((1 << (8 - k)) - 1)]) + rec[1:]
    return flag, [int.from_bytes(body[i:i + fb], "big") for i in range(0, len(body), fb)]


def kind(cname, width, flag, any_bits):
    """'point', 'inf' or 'bad', and whether the larger y is asked for."""
    want_larger = bool(flag & 1)
    if is_bn(cname):
        if width == RAW:
            return ("point" if any_bits else "inf") if flag == 0 else "bad", want_larger
        if flag >= 2:
            return "point", want_larger
        return ("inf" if flag == 1 and not any_bits else "bad"), want_larger
    if width == RAW:
        if flag == 0:
            return ("point" if any_bits else "inf"), want_larger
        return ("inf" if flag == 0b010 and not any_bits else "bad"), want_larger
    if flag in (0b100, 0b101):
        return "point", want_larger
    return ("inf" if flag == 0b110 and not any_bits else "bad"), want_larger


@functools.lru_cache(maxsize=None)
def decode(cname, g2, rec, width, flags=0):
    """(class, is_infinity, point): the point is None unless the class is OK and
    the record is not an infinity."""
    c = pc.params(cname)
    assert len(rec) == record_bytes(c, g2, width)
    flag, v = split(cname, rec)
    what, want_larger = kind(cname, width, flag, any(v))
    if what == "bad":
        return BAD_ENCODING, False, None
    if what == "inf":
        return OK, True, None
    if any(x >= c.p for x in v):
        return NOT_REDUCED, False, None
    G = pc.pyref.Group(c, g2)
    F = G.F
    x = (v[1], v[0]) if g2 else v[0]
    if width == RAW:
        y = (v[3], v[2]) if g2 else v[1]
    else:
        rhs = F.add(F.mul(F.mul(x, x), x), G.b)
        y = sub.sqrt_fp2(rhs, c) if g2 else sub.sqrt_fp(rhs, c.p)
        if y is None:
            return NO_ROOT, False, None
        if larger(c, g2, y) != want_larger:
            y = F.neg(y)
    P = (x, y)
    if flags & NO_SUBGROUP_CHECK:
        return OK, False, P
    cls, inf = pc.classify(cname, g2, pc.raw_of_point(c, P, g2))
    assert not inf and cls in (OK, OFF_CURVE, OFF_SUBGROUP)
    assert not (cls == OFF_CURVE and width == COMPRESSED)
    return cls, False, (P if cls == OK else None)


def gnark_bytes(cname, g2, P):
    """The point in gnark's memory layout (None -> (0, 0))."""
    c = pc.params(cname)
    return pc.raw_bytes(c, pc.raw_of_point(c, P, g2))


def decode_all(cname, g2, recs, width, flags=0):
    """(report dict as gm_points_decode gives it, status list, the points' bytes)."""
    res = [decode(cname, g2, r, width, flags) for r in recs]
    st = [k for k, _, _ in res]
    bad = [i for i, k in enumerate(st) if k != OK]
    rep = dict(n=len(recs), infinities=sum(1 for _, inf, _ in res if inf),
               not_reduced=st.count(NOT_REDUCED), off_curve=st.count(OFF_CURVE), off_subgroup=st.count(OFF_SUBGROUP),
               bad_encoding=st.count(BAD_ENCODING), no_root=st.count(NO_ROOT),
               first_bad=bad[0] if bad else len(recs), first_class=st[bad[0]] if bad else 0)
    return rep, st, b"".join(gnark_bytes(cname, g2, P) for _, _, P in res)


# ---- case lists ----------------------------------------------------------------------
def corpus_points(cname, g2, cls):
    """The affine points of points_check_cases.cases of one class (infinity left out)."""
    c = pc.params(cname)
    return [(name, pc.decode(c, g2, raw)) for name, raw, k in pc.cases(cname, g2)
            if k == cls and any(raw) and all(v < c.p for v in raw)]


def other_width_flags(cname, width):
    """The flags that belong to the other width (points and infinity)."""
    if is_bn(cname):
        return [0b10, 0b11, 0b01] if width == RAW else [0b00]
    return [0b100, 0b101, 0b110] if width == RAW else [0b000, 0b010]


def invalid_flags(cname):
    return [] if is_bn(cname) else [0b001, 0b011, 0b111]


def reflag(cname, rec, flag):
    k = flag_bits(cname)
    return with_flag(cname, bytes([rec[0] & ((1 << (8 - k)) - 1)]) + rec[1:], flag)


def _no_root_x(cname, g2):
    c = pc.params(cname)
    G = pc.pyref.Group(c, g2)
    F = G.F
    for t in range(1, 200):
        x = (t, 1) if g2 else t
        rhs = F.add(F.mul(F.mul(x, x), x), G.b)
        if (sub.sqrt_fp2(rhs, c) if g2 else sub.sqrt_fp(rhs, c.p)) is None:
            return x
    raise AssertionError("no x without a root found")


@functools.lru_cache(maxsize=None)
def decode_cases(cname, g2, width):
    """[(kind, name, record, class under the full check)] for one curve, group and
    width.  `kind` groups the cases the way the tests count them; the class is what
    the case is meant to be, and the model decides what it is."""
    c = pc.params(cname)
    p, fb, k = c.p, fp_bytes(c), flag_bits(cname)
    G = pc.pyref.Group(c, g2)
    valid = corpus_points(cname, g2, pc.OK)
    out = []
    for name, P in valid:
        out.append(("valid", name, encode(cname, g2, P, width), OK))
    P = dict(valid)["P"]
    assert larger(c, g2, P[1]) != larger(c, g2, G.neg(P)[1])
    if width == COMPRESSED:
        for name, Q in (("P", P), ("-P", G.neg(P))):
            rec = encode(cname, g2, Q, width)
            out.append(("flip", name + " other y", reflag(cname, rec, (rec[0] >> (8 - k)) ^ 1), OK))
    inf = encode(cname, g2, None, width)
    out.append(("infinity", "infinity", inf, OK))
    if width == RAW:
        out.append(("infinity", "all-zero", bytes(len(inf)), OK))
    for pos, bit in ((len(inf) - 1, 1), (0, 1), (len(inf) // 2, 0x80)):
        b = bytearray(inf)
        b[pos] |= bit
        if is_bn(cname) and width == RAW:
            continue  # the raw infinity has no flag: a stray bit makes it a point
        out.append(("stray", "infinity with a bit at byte %d" % pos, bytes(b), BAD_ENCODING))
    good = encode(cname, g2, P, width)
    for f in invalid_flags(cname):
        out.append(("invalid flag", "flag %s" % bin(f), reflag(cname, good, f), BAD_ENCODING))
        out.append(("invalid flag", "flag %s, zero body" % bin(f), reflag(cname, bytes(len(good)), f), BAD_ENCODING))
    for f in other_width_flags(cname, width):
        out.append(("other width", "flag %s" % bin(f), reflag(cname, good, f), BAD_ENCODING))
        if not (is_bn(cname) and f == 0):
            out.append(("other width", "flag %s, zero body" % bin(f), reflag(cname, bytes(len(good)), f), BAD_ENCODING))
    # not reduced: the integers behind the flag
    pflag = flag_of_point(cname, width, False)
    avail = 1 << (8 * fb - k)
    ncomp = len(components(P, g2, width))

    def put(vals):
        return with_flag(cname, b"".join(v.to_bytes(fb, "big") for v in vals), pflag)

    base = components(P, g2, width)
    # "x + p where it fits": behind BLS12-381's three flag bits only a first component below
    # 2^381 - p does, about one point in five; small multiples of the generator are searched
    fits, Q = [], G.generator()
    for _ in range(64):
        if components(Q, g2, width)[0] + p < avail:
            fits.append(components(Q, g2, width))
            break
        Q = G.add(Q, G.generator())
    assert fits, "no point whose first component + p fits behind the flag"
    out.append(("not reduced", "first = p", put([p] + base[1:]), NOT_REDUCED))
    out.append(("not reduced", "first + p", put([fits[0][0] + p] + fits[0][1:]), NOT_REDUCED))
    out.append(("not reduced", "all-ones", put([avail - 1] + [(1 << (8 * fb)) - 1] * (ncomp - 1)), NOT_REDUCED))
    out.append(("not reduced", "last = p", put(base[:-1] + [p]), NOT_REDUCED))
    if g2:
        out.append(("not reduced a1", "x.a1 = p", put([p] + base[1:]), NOT_REDUCED))
        out.append(("not reduced a0", "x.a0 = p", put([base[0], p] + base[2:]), NOT_REDUCED))
    if width == COMPRESSED:
        x = _no_root_x(cname, g2)
        for f in (False, True):
            body = b"".join(v.to_bytes(fb, "big") for v in ((x[1], x[0]) if g2 else (x,)))
            out.append(("no root", "x = %s" % (x,), with_flag(cname, body, flag_of_point(cname, width, f)), NO_ROOT))
    else:
        for name, Q in corpus_points(cname, g2, pc.OFF_CURVE):
            out.append(("off curve", name, encode(cname, g2, Q, width), OFF_CURVE))
    for name, Q in corpus_points(cname, g2, pc.OFF_SUBGROUP):
        out.append(("off subgroup", name, encode(cname, g2, Q, width), OFF_SUBGROUP))
        if G.F.is_zero(Q[1]):
            rec = encode(cname, g2, Q, width)
            out.append(("y = 0", name, rec, OFF_SUBGROUP))
            if width == COMPRESSED:
                out.append(("y = 0", name + " other flag", reflag(cname, rec, (rec[0] >> (8 - k)) ^ 1), OFF_SUBGROUP))
    return out
