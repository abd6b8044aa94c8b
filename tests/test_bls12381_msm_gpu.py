"""BLS12-381 (curve id 2) MSM on the device against pyref's group law: G1 and G2,
the plain path with the GLV split forced on and off, prepared and precomputed
point sets, special scalars of the balanced split (each half at its largest
magnitude, every sign combination) and special points.  The points are small
multiples of the generator, so a large MSM's expected value is ONE scalar
multiplication by sum_i k_i t_i; up to n = 1000 the expected value also comes
from pyref's own Group.msm."""
import os
import random
import sys

import numpy as np
import pytest

import pyref
import bls12381_params as bp

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import glv_constants as glv  # noqa: E402

pytestmark = pytest.mark.gpu
C, R = bp.C, bp.R
NB = 64  # distinct bases


@pytest.fixture(scope="module")
def bases():
    """per group: the points [1]G..[64]G, their encodings and those of their negatives"""
    out = {}
    for g2 in (False, True):
        G = pyref.Group(C, g2)
        pts = bp.multiples(g2, NB)
        pb = 192 if g2 else 96
        pos = np.frombuffer(bp.enc_points(pts, g2), np.uint8).reshape(NB, pb)
        neg = np.frombuffer(bp.enc_points([G.neg(P) for P in pts], g2), np.uint8).reshape(NB, pb)
        out[g2] = (G, pts, pos, neg)
    return out


def _specials():
    d = glv.derive_bls12381()
    return glv.specials_bls12381(d)


def _case(bases, g2, n, seed):
    """n (point, scalar) pairs: special scalars first, then random; points cycle
    through the bases with (0,0), a repeated point and a P / -P pair mixed in.
    Returns (scalars, points, logs) with points[i] = [logs[i]]G (log 0: infinity)."""
    G, pts, _, _ = bases[g2]
    rng = random.Random(seed)
    sp = _specials()
    sc = [sp[i] if i < len(sp) else rng.randrange(R) for i in range(n)]
    rng.shuffle(sc)
    logs = [rng.randrange(1, NB + 1) * rng.choice((1, -1)) for _ in range(n)]
    if n >= 8:
        logs[1] = 0                      # (0, 0)
        logs[3] = logs[2]                # P twice in a row
        logs[5] = -logs[4]               # P and -P
        sc[5] = sc[4]                    # ... with the same scalar: they cancel
    P = [None if t == 0 else (pts[t - 1] if t > 0 else G.neg(pts[-t - 1])) for t in logs]
    return sc, P, logs


def _expected(bases, g2, sc, logs):
    G = bases[g2][0]
    return bp.enc_points([G.mul(G.generator(), sum(k * t for k, t in zip(sc, logs)) % R)], g2)


@pytest.mark.parametrize("glv_mode", [1, 0])
@pytest.mark.parametrize("g2", [False, True])
def test_msm_small_sizes(gm_ctx, bases, g2, glv_mode):
    G = bases[g2][0]
    gm_ctx.set_msm_glv(glv_mode)
    try:
        for n in (1, 2, 63, 64, 65, 1000):
            sc, P, logs = _case(bases, g2, n, 1000 * n + g2)
            exp = bp.enc_points([G.msm(sc, P)], g2)
            assert exp == _expected(bases, g2, sc, logs)
            S = gm_ctx.copy_to_device(bp.enc_fr(sc))
            Pd = gm_ctx.copy_points_to_device(2, bp.enc_points(P, g2), g2)
            try:
                assert gm_ctx.msm(2, S, Pd, n, g2)[1] == exp, (g2, glv_mode, n)
            finally:
                S.free()
                Pd.free()
    finally:
        gm_ctx.set_msm_glv(-1)


@pytest.mark.parametrize("g2", [False, True])
def test_msm_each_special_scalar_alone(gm_ctx, bases, g2):
    """one scalar per MSM: a wrong sign or a wrong half of the split cannot cancel"""
    G, pts, _, _ = bases[g2]
    gm_ctx.set_msm_glv(1)
    try:
        Pd = gm_ctx.copy_points_to_device(2, bp.enc_points([pts[6]], g2), g2)
        for k in _specials():
            S = gm_ctx.copy_to_device(bp.enc_fr([k]))
            try:
                assert gm_ctx.msm(2, S, Pd, 1, g2)[1] == bp.enc_points([G.mul(pts[6], k)], g2), hex(k)
            finally:
                S.free()
        Pd.free()
    finally:
        gm_ctx.set_msm_glv(-1)


@pytest.mark.parametrize("g2", [False, True])
def test_msm_prepared_and_precomputed(gm_ctx, bases, g2):
    n = 1000
    sc, P, logs = _case(bases, g2, n, 77 + g2)
    exp = _expected(bases, g2, sc, logs)
    S = gm_ctx.copy_to_device(bp.enc_fr(sc))
    enc = bp.enc_points(P, g2)
    sets = [gm_ctx.points_upload(2, enc, g2)] + [gm_ctx.points_upload_precomputed(2, enc, g2, window=w) for w in (9, 16)]
    try:
        assert gm_ctx.msm_prepared(2, S, sets[0], n, g2)[1] == exp
        assert gm_ctx.msm_precomputed(2, S, sets[1], n, g2)[1] == exp
        assert gm_ctx.msm_precomputed(2, S, sets[2], n, g2)[1] == exp
        assert gm_ctx.msm_precomputed(2, S, sets[2], 65, g2)[1] == _expected(bases, g2, sc[:65], logs[:65])
    finally:
        S.free()
        for x in sets:
            x.free()


def _large(bases, g2, n, seed):
    _, _, pos, neg = bases[g2]
    rng = np.random.default_rng(seed)
    idx = rng.integers(0, NB, n)
    sgn = rng.integers(0, 2, n).astype(bool)
    enc = np.where(sgn[:, None], neg[idx], pos[idx]).reshape(-1)
    prng = random.Random(seed)
    sc = [prng.randrange(R) for _ in range(n)]
    logs = [-(int(i) + 1) if s else int(i) + 1 for i, s in zip(idx, sgn)]
    return sc, enc, logs


@pytest.mark.parametrize("g2,n", [(False, (1 << 15) + 37), (False, (1 << 17) + 5), (True, (1 << 15) + 37)])
@pytest.mark.parametrize("glv_mode", [1, 0])
def test_msm_large(gm_ctx, bases, g2, n, glv_mode):
    """multi-bin sort and the piece plan: 64 bases with random signs"""
    sc, enc, logs = _large(bases, g2, n, n + glv_mode)
    exp = _expected(bases, g2, sc, logs)
    gm_ctx.set_msm_glv(glv_mode)
    S = gm_ctx.copy_to_device(bp.enc_fr(sc))
    Pd = gm_ctx.copy_points_to_device(2, enc, g2)
    try:
        assert gm_ctx.msm(2, S, Pd, n, g2)[1] == exp
    finally:
        gm_ctx.set_msm_glv(-1)
        S.free()
        Pd.free()


def test_msm_dirty_arena_and_async(gm_ctx, bases):
    """a larger MSM first, then a mostly-zero-scalar MSM on the same context; three
    MSMs in flight equal the synchronous results"""
    n = (1 << 15) + 37
    sc, enc, logs = _large(bases, False, n, 4242)
    S = gm_ctx.copy_to_device(bp.enc_fr(sc))
    Pd = gm_ctx.copy_points_to_device(2, enc, False)
    m = 3000
    sparse = [0] * m
    for i in (0, 17, 1500, 2999):
        sparse[i] = sc[i]
    S2 = gm_ctx.copy_to_device(bp.enc_fr(sparse))
    try:
        full = gm_ctx.msm(2, S, Pd, n)[1]
        assert full == _expected(bases, False, sc, logs)
        assert gm_ctx.msm(2, S2, Pd, m)[1] == _expected(bases, False, sparse, logs[:m])
        pend = [gm_ctx.msm_async(2, S, Pd, n), gm_ctx.msm_async(2, S2, Pd, m), gm_ctx.msm_async(2, S, Pd, 1000)]
        got = [p.wait()[1] for p in pend]
        assert got[0] == full and got[1] == _expected(bases, False, sparse, logs[:m])
        assert got[2] == _expected(bases, False, sc[:1000], logs[:1000])
    finally:
        for x in (S, S2, Pd):
            x.free()
