"""BLS12-381 (curve id 2) KZG on the device: commit, evaluation, fold, division by
X - z and the openings, against integer arithmetic and pyref's group law with an
SRS [tau^i]G of a known tau."""
import random

import pytest

import pyref
import bls12381_params as bp

pytestmark = pytest.mark.gpu
C, R = bp.C, bp.R
TAU = 0x5a3c9e1f7b2d4c6a8e0f1a2b3c4d5e6f708192a3b4c5d6e7f8091a2b3c4d5e6f % R
M = 1027


@pytest.fixture(scope="module")
def srs(gm_ctx):
    G = pyref.Group(C, False)
    pts, t = [], 1
    for _ in range(M):
        pts.append(G.mul(C.g1, t))
        t = t * TAU % R
    buf = gm_ctx.points_upload(2, bp.enc_points(pts, False), False)
    yield buf
    buf.free()


def _ev(f, z):
    acc = 0
    for c in reversed(f):
        acc = (acc * z + c) % R
    return acc


def _pt(k):
    return bp.enc_points([pyref.Group(C, False).mul(C.g1, k % R)], False)


def _poly(m, seed):
    rng = random.Random(seed)
    f = [rng.randrange(R) for _ in range(m)]
    f[0], f[-1] = R - 1, R - 1
    return f


@pytest.mark.parametrize("m", [8, 64, 1027])
def test_commit(gm_ctx, srs, m):
    f = _poly(m, m)
    assert gm_ctx.kzg_commit(2, srs, bp.enc_fr(f)) == _pt(_ev(f, TAU))


def test_eval_fold_divide(gm_ctx):
    rng = random.Random(11)
    lens = [1027, 64, 1, 600]
    fs = [_poly(m, 20 + m) for m in lens]
    z, gamma = rng.randrange(R), rng.randrange(R)
    bufs = [gm_ctx.copy_to_device(bp.enc_fr(f)) for f in fs]
    out = gm_ctx.malloc(32 * max(lens))
    q = gm_ctx.malloc(32 * max(lens))
    try:
        for zz in (z, 0, 1, R - 1):
            assert gm_ctx.kzg_eval(2, bufs, bp.enc_fr([zz])) == [bp.enc_fr([_ev(f, zz)]) for f in fs], zz
        gm_ctx.poly_fold(2, bufs, bp.enc_fr([gamma]), out)
        folded = [sum(pow(gamma, i, R) * (f[j] if j < len(f) else 0) for i, f in enumerate(fs)) % R
                  for j in range(max(lens))]
        assert out.to_host() == bp.enc_fr(folded)
        for f, b in zip(fs, bufs):
            if len(f) < 2:
                continue
            val = gm_ctx.poly_div_linear(2, b, bp.enc_fr([z]), q)
            # synthetic division: q_{m-2} = f_{m-1}, q_{j-1} = f_j + z q_j
            qq, carry = [0] * (len(f) - 1), 0
            for j in range(len(f) - 1, 0, -1):
                carry = (f[j] + z * carry) % R
                qq[j - 1] = carry
            assert val == bp.enc_fr([_ev(f, z)])
            assert q.to_host(32 * (len(f) - 1)) == bp.enc_fr(qq)
    finally:
        for x in bufs + [out, q]:
            x.free()


def test_open_and_batch_open(gm_ctx, srs):
    """H = [q(tau)]G with q(tau) (tau - z) = f(tau) - f(z)"""
    rng = random.Random(12)
    z, gamma = rng.randrange(R), rng.randrange(R)
    fs = [_poly(m, 40 + m) for m in (1027, 64, 9)]
    bufs = [gm_ctx.copy_to_device(bp.enc_fr(f)) for f in fs]
    inv = pow((TAU - z) % R, -1, R)
    try:
        for f, b in zip(fs, bufs):
            val, h = gm_ctx.kzg_open(2, srs, b, bp.enc_fr([z]))
            assert val == bp.enc_fr([_ev(f, z)])
            assert h == _pt((_ev(f, TAU) - _ev(f, z)) * inv)
        folded = [sum(pow(gamma, i, R) * (f[j] if j < len(f) else 0) for i, f in enumerate(fs)) % R
                  for j in range(1027)]
        val, h = gm_ctx.kzg_batch_open(2, srs, bufs, bp.enc_fr([z]), bp.enc_fr([gamma]))
        assert val == bp.enc_fr([_ev(folded, z)])
        assert h == _pt((_ev(folded, TAU) - _ev(folded, z)) * inv)
    finally:
        for x in bufs:
            x.free()
