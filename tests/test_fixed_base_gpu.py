"""gm_batch_mul_fixed against two independent references, byte for byte: the CPU
oracle's batch multiplication and the library's own double-and-add entry
(gm_batch_mul_base).  Both curves, G1 and G2; every window width that takes
another path through the recoding (c = 4, 8, 13, 16 and the model's choice); the
sizes around a block of the normaliser; scalars that sit on every edge of the
signed-digit recoding, the ones whose top window doubles the running sum among
them; and zeros wherever the batch inversion could trip over them."""
import random

import numpy as np
import pytest

import gnark_mi355x as gm
import pyref

pytestmark = pytest.mark.gpu

CURVE_NAMES = ("bn254", "bls12377")
GROUPS = [(c, g2) for c in CURVE_NAMES for g2 in (False, True)]
WINDOWS = (4, 8, 13, 16)
SIZES = (1, 255, 256, 257, 1000)
NMAX = max(SIZES)
# (curve, c) pairs for which a top-window doubling scalar is known to exist
DOUBLING_PAIRS = {("bn254", 4), ("bn254", 8), ("bn254", 16), ("bls12377", 4), ("bls12377", 13), ("bls12377", 16)}
GUARD = 4096


def windows(r: int, c: int) -> int:
    """W = ceil((bits of r + 1) / c)."""
    return (r.bit_length() + 1 + c - 1) // c


def recode(k: int, c: int, W: int) -> list:
    """The signed digits of k, low window first: raw digits above 2^(c-1) borrow
    2^c from the next window."""
    digits, carry = [], 0
    for w in range(W):
        raw = ((k >> (c * w)) & ((1 << c) - 1)) + carry
        carry = 1 if raw > (1 << (c - 1)) else 0
        digits.append(raw - (carry << c))
    assert carry == 0 and sum(d << (c * w) for w, d in enumerate(digits)) == k
    return digits


def doubling_scalars(r: int, c: int) -> list:
    """k in [0, r) whose lower windows sum to the top window's addend (mod r), so
    that the last addition of a low-to-high accumulation is a doubling:
    k = 2 d 2^(c (W-1)) - r."""
    W = windows(r, c)
    top = 1 << (c * (W - 1))
    out = []
    for d in range(1, (1 << (c - 1)) + 1):
        k = 2 * d * top - r
        if not 0 <= k < r:
            continue
        dg = recode(k, c, W)
        if dg[-1] == d and (sum(x << (c * w) for w, x in enumerate(dg[:-1])) - d * top) % r == 0:
            out.append(k)
    return out


def edge_scalars(r: int, c: int) -> list:
    W = windows(r, c)
    half = 1 << (c - 1)
    s = [0, 1, 2, r - 1, r - 2, (r - 1) // 2]
    for w in range(W):
        s += [(1 << (c * w)) - 1, 1 << (c * w), (1 << (c * w)) + 1]
    # a digit exactly 2^(c-1) (stays positive) and one at 2^(c-1) + 1 (goes negative,
    # carries) in the lowest, a middle and the top window that can hold it below r
    top = max(w for w in range(W) if ((half + 1) << (c * w)) < r)
    for w in (0, W // 2, top):
        s += [half << (c * w), (half + 1) << (c * w)]
    # every window at 2^c - 1: the carry runs through all of them
    s.append(((1 << (c * (W - 1))) - 1) % r)
    s.append((1 << (r.bit_length() - 1)) - 1)
    s += doubling_scalars(r, c)
    return [k % r for k in s]


def scalar_set(cname: str, c: int) -> list:
    r = pyref.CURVES[cname].r
    s = edge_scalars(r, c)
    assert len(s) < SIZES[1], "the edge cases fit the second-smallest size"
    rng = random.Random(f"fixed-base {cname} {c}")
    return s + [rng.randrange(r) for _ in range(NMAX - len(s))]


def enc(cname: str, ks) -> bytes:
    c = pyref.CURVES[cname]
    return b"".join(pyref.encode_fr(c, k) for k in ks)


def bases(cname: str, g2: bool, oracle) -> dict:
    gen = gm.generator(cname, g2)
    rnd = oracle.batch_mul_base(cname, g2, gen, enc(cname, [random.Random(f"base {cname} {g2}").randrange(
        1, pyref.CURVES[cname].r)]))
    return {"generator": gen, "random": rnd, "infinity": bytes(gm.point_bytes(cname, g2))}


@pytest.fixture(scope="module")
def reference(gm_ctx, oracle):
    """(curve, g2, base name, scalar bytes) -> the expected points, computed once:
    the oracle's, asserted equal to gm_batch_mul_base's."""
    cache = {}

    def get(cname, g2, base_name, base, scalars: bytes):
        key = (cname, g2, base_name, scalars)
        if key not in cache:
            n = len(scalars) // gm.FR_BYTES
            want = oracle.batch_mul_base(cname, g2, base, scalars)
            K = gm_ctx.copy_to_device(scalars)
            P = gm_ctx.batch_mul_base(cname, g2, base, K, n)
            try:
                assert P.to_host() == want, "the two references disagree"
            finally:
                K.free()
                P.free()
            cache[key] = want
        return cache[key]

    return get


def run_fixed(ctx, cname, g2, base, scalars: bytes, n: int) -> bytes:
    """n points through gm_batch_mul_fixed into a buffer with a guard behind it."""
    pb = gm.point_bytes(cname, g2)
    K = ctx.copy_to_device(scalars[:gm.FR_BYTES * n])
    out = ctx.malloc(pb * n + GUARD)
    try:
        out.write(np.full(pb * n + GUARD, 0xA5, np.uint8))
        ctx.batch_mul_fixed(cname, g2, base, K, n, out=out)
        got = out.to_host()
    finally:
        K.free()
        out.free()
    assert got[pb * n:] == b"\xa5" * GUARD, "wrote past n points"
    return got[:pb * n]


def test_doubling_scalars_exist():
    """The plain-Python recoder finds a top-window doubling scalar at least for the
    listed (curve, c) pairs, so the sets below exercise the doubling branch."""
    for cname, c in sorted(DOUBLING_PAIRS):
        assert doubling_scalars(pyref.CURVES[cname].r, c), (cname, c)


@pytest.mark.parametrize("c", WINDOWS + (0,), ids=lambda c: f"c{c}" if c else "model")
@pytest.mark.parametrize("cname,g2", GROUPS, ids=lambda v: v if isinstance(v, str) else ("g2" if v else "g1"))
def test_matches_both_references(gm_ctx, oracle, reference, cname, g2, c):
    # the model's own choice runs on the c = 8 scalars
    scalars = enc(cname, scalar_set(cname, c or 8))
    pb = gm.point_bytes(cname, g2)
    gm_ctx.set_fixed_base_window(c)
    try:
        for name, base in bases(cname, g2, oracle).items():
            want = reference(cname, g2, name, base, scalars)
            if name == "infinity":
                assert want == bytes(pb * NMAX)
            for n in SIZES:
                got = run_fixed(gm_ctx, cname, g2, base, scalars, n)
                bad = [i for i in range(n) if got[pb * i:pb * (i + 1)] != want[pb * i:pb * (i + 1)]]
                assert not bad, (name, n, bad[:8])
    finally:
        gm_ctx.set_fixed_base_window(0)


@pytest.mark.parametrize("cname,g2", GROUPS, ids=lambda v: v if isinstance(v, str) else ("g2" if v else "g1"))
def test_zeros_inside_the_normaliser(gm_ctx, oracle, reference, cname, g2):
    """Infinity contributes 1 to a block's product: a whole block of zero scalars
    between non-zero blocks (256 lanes, two blocks where a block is 128), zero at a
    block's first and last position, and nothing but zeros."""
    r = pyref.CURVES[cname].r
    rng = random.Random(f"zeros {cname}")
    pb = gm.point_bytes(cname, g2)
    base = gm.generator(cname, g2)
    whole = [rng.randrange(1, r) for _ in range(256)] + [0] * 256 + [rng.randrange(1, r) for _ in range(300)]
    ends = [rng.randrange(1, r) for _ in range(600)]
    for i in (0, 127, 128, 255, 256, 511, 512, 599):
        ends[i] = 0
    for ks in (whole, ends, [0] * 300):
        scalars = enc(cname, ks)
        want = reference(cname, g2, "generator", base, scalars)
        for i, k in enumerate(ks):
            assert (want[pb * i:pb * (i + 1)] == bytes(pb)) == (k == 0)
        assert run_fixed(gm_ctx, cname, g2, base, scalars, len(ks)) == want


def test_window_setter_bounds(gm_ctx):
    for c in (1, 17, -1):
        with pytest.raises(gm.GmError, match="gm_set_fixed_base_window"):
            gm_ctx.set_fixed_base_window(c)
    gm_ctx.set_fixed_base_window(0)
    # a refused setting leaves the context usable
    K = gm_ctx.copy_to_device(enc("bn254", [5]))
    try:
        P = gm_ctx.batch_mul_fixed("bn254", False, gm.generator("bn254"), K, 1)
        Q = gm_ctx.batch_mul_base("bn254", False, gm.generator("bn254"), K, 1)
        assert P.to_host() == Q.to_host()
        P.free()
        Q.free()
    finally:
        K.free()
