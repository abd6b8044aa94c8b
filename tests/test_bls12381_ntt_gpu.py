"""BLS12-381 (curve id 2) NTT, poly ops and computeH against pyref with the curve's
CurveParams, bit for bit.  Fr is 255 bits with R' / r ~ 70.66: the sizes run every
pass shape (t < 2, one pass with odd and even t, two passes -- the growing-bound
DIF rounds and the inter-pass twiddle store -- and three), the inputs include the
all-(r - 1) vector that drives every lazy bound to its top."""
import random

import pytest

import pyref
import bls12381_params as bp

pytestmark = pytest.mark.gpu
C, R = bp.C, bp.R
MODES = [(inv, dit, coset) for inv in (False, True) for dit in (False, True) for coset in (False, True)]


def _inputs(n, seed):
    rng = random.Random(seed)
    return {"random": [rng.randrange(R) for _ in range(n)], "all r-1": [R - 1] * n,
            "alternating": [0 if i & 1 else R - 1 for i in range(n)], "single 1": [1] + [0] * (n - 1)}


def _ref(x, inv, dit, coset):
    return (pyref.fft_inverse if inv else pyref.fft)(C, x, "DIT" if dit else "DIF", coset)


def _device(ctx, x, inv, dit, coset):
    X = ctx.copy_to_device(bp.enc_fr(x))
    try:
        ctx.ntt(2, X, len(x), inv, dit, coset)
        return X.to_host()
    finally:
        X.free()


@pytest.mark.parametrize("logn", [1, 2, 3, 5, 8, 10, 11])
def test_ntt_all_modes(gm_ctx, logn):
    n = 1 << logn
    for name, x in _inputs(n, 100 + logn).items():
        for inv, dit, coset in MODES:
            assert _device(gm_ctx, x, inv, dit, coset) == bp.enc_fr(_ref(x, inv, dit, coset)), (logn, name, inv, dit, coset)


_BIG = {}


def _big_input(logn, kind):
    if logn not in _BIG:
        _BIG[logn] = _inputs(1 << logn, 200 + logn)
    return _BIG[logn][kind]


@pytest.mark.parametrize("inv,dit,coset", MODES)
@pytest.mark.parametrize("kind", ["random", "all r-1", "alternating", "single 1"])
@pytest.mark.parametrize("logn", [16, 17])
def test_ntt_multi_pass(gm_ctx, logn, kind, inv, dit, coset):
    """two passes of t = 8 (2^16: the B = 16 growing DIF round, the inter-pass twiddle
    store and this field's < 2p DIT store) and three passes (2^17), every input kind"""
    x = _big_input(logn, kind)
    assert _device(gm_ctx, x, inv, dit, coset) == bp.enc_fr(_ref(x, inv, dit, coset)), (logn, kind)


def test_ntt_refuses_past_two_adicity_and_curve(gm_ctx):
    import gnark_mi355x as gm
    X = gm_ctx.copy_to_device(bytes(32 * 3))
    try:
        with pytest.raises(gm.GmError):
            gm_ctx.ntt(2, X, 3, False, False, False)
        with pytest.raises(gm.GmError):
            gm_ctx.ntt(3, X, 2, False, False, False)
    finally:
        X.free()


def test_poly_ops_and_reverse(gm_ctx):
    n = 1 << 10
    rng = random.Random(7)
    a, b, c = ([rng.randrange(R) for _ in range(n)] for _ in range(3))
    a[0], b[0], c[0] = R - 1, R - 1, R - 1
    den = rng.randrange(1, R)
    A, B, Cc = (gm_ctx.copy_to_device(bp.enc_fr(v)) for v in (a, b, c))
    try:
        gm_ctx.poly_ops(2, A, B, Cc, n, bp.enc_fr([den]))
        assert A.to_host() == bp.enc_fr([(x * y - z) * den % R for x, y, z in zip(a, b, c)])
        gm_ctx.reverse_scalars(2, B, n)
        assert B.to_host() == bp.enc_fr(pyref.bit_reverse(b))
    finally:
        for x in (A, B, Cc):
            x.free()


@pytest.mark.parametrize("n,length", [(4, 3), (16, 16), (1024, 1000), (2048, 2048)])
def test_compute_h(gm_ctx, n, length):
    rng = random.Random(n)
    a, b = ([rng.randrange(R) for _ in range(length)] for _ in range(2))
    c = [x * y % R for x, y in zip(a, b)]  # a satisfied system: h is a polynomial
    c[-1] = (c[-1] + 1) % R if length < 8 else c[-1]  # and one that is not (the arithmetic is the same)
    bufs = [gm_ctx.malloc(32 * n) for _ in range(3)]
    try:
        for B_, v in zip(bufs, (a, b, c)):
            B_.write(bp.enc_fr(v))
        gm_ctx.compute_h(2, *bufs, length, n)
        assert bufs[0].to_host() == bp.enc_fr(pyref.compute_h(C, a, b, c, n))
    finally:
        for x in bufs:
            x.free()


def test_random_scalars_are_canonical(gm_ctx):
    S = gm_ctx.random_scalars(2, 4096, 5)
    try:
        raw = S.to_host()
        vals = [int.from_bytes(raw[i:i + 32], "little") for i in range(0, len(raw), 32)]
        assert all(v < R for v in vals) and len(set(vals)) > 4000
    finally:
        S.free()
