"""KZG openings on the device (gm_kzg_eval, gm_poly_div_linear, gm_poly_fold,
gm_kzg_open, gm_kzg_batch_open) against Python big-int Horner evaluation and
synthetic division -- _eval / _quotient of test_plonk_replay_gpu.py, i.e.
kzg_mi355x.go's host code and gnark-crypto's dividePolyByXminusA.

The recurrence s[i] = f[i] + z s[i+1] is linear in f, so the reference of the
element-wise tests runs on the Montgomery integers as they lie in memory (f R
gives s R): no element is converted, and the comparison is byte for byte.

Chunk geometry of csrc/kzg.hip: a thread owns 8 coefficients, a block 128
threads, a chunk C = 1024 coefficients; the carry kernel gives each of its 128
threads a run of 4 chunks, 512 chunks per tile.  The lengths below cover one
thread, one wave, one block, C - 1, C, C + 1, 2C + 1, a ragged last chunk, chunk
counts that leave a carry run partly filled (2^16 + 3: 65, 2^18 + 3: 257) and
one more chunk than a carry tile holds (2^19 + 3: 513 chunks, two tiles).
"""
import numpy as np
import pytest

import pyref

pytestmark = pytest.mark.gpu

CURVE_NAMES = ("bls12377", "bn254", "bls12381")
LENGTHS = [1, 2, 3, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2047, 2048, 2049, 4097, (1 << 16) + 3,
           (1 << 18) + 3, (1 << 19) + 3]
KINDS = ("random", "all_r_minus_1", "mostly_zero", "multiple_of_x_minus_z")


def _ints(b):
    return [int.from_bytes(b[32 * i:32 * i + 32], "little") for i in range(len(b) // 32)]


def _bytes(vals):
    return b"".join(v.to_bytes(32, "little") for v in vals)


def _random_mont(m, seed):
    """m field elements as the integers of their Montgomery words: any value
    below r is one; 2^252 < r for all three scalar fields."""
    a = np.random.RandomState(seed).randint(0, 256, size=(m, 32), dtype=np.uint8)
    a[:, 31] &= 0x0F
    return _ints(a.tobytes())


def _suffix(r, F, z):
    """S[i] = F[i] + z S[i+1], S[m] = 0: S[0] = f(z), S[1:m] = the quotient."""
    S = [0] * (len(F) + 1)
    for i in range(len(F) - 1, -1, -1):
        S[i] = (F[i] + z * S[i + 1]) % r
    return S


def _points(c):
    return [("random", pyref.random_scalars(c, 1, 0x5eed)[0]), ("zero", 0), ("one", 1), ("r-1", c.r - 1)]


def _coefficients(c, kind, m, z):
    r = c.r
    if kind == "random":
        return _random_mont(m, 0xC0 + m % 251)
    if kind == "all_r_minus_1":
        return [int.from_bytes(pyref.encode_fr(c, r - 1), "little")] * m
    if kind == "mostly_zero":
        F = [0] * m
        for j, v in zip((0, m // 2, m - 1), _random_mont(3, 0xD0)):
            F[j] = v
        return F
    # (X - z) g: F[i] = G[i-1] - z G[i]; the value at z is exactly 0
    G = _random_mont(max(m - 1, 0), 0xE0 + m % 251)
    return [((G[i - 1] if i >= 1 else 0) - z * (G[i] if i < m - 1 else 0)) % r for i in range(m)]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("m", LENGTHS)
@pytest.mark.parametrize("cname", CURVE_NAMES)
def test_poly_div_linear_elementwise(gm_ctx, cname, m, kind):
    c = pyref.CURVES[cname]
    q_dev = gm_ctx.malloc(32 * max(m - 1, 1))
    try:
        for zname, z in _points(c):
            F = _coefficients(c, kind, m, z)
            fb = _bytes(F)
            f_dev = gm_ctx.copy_to_device(fb)
            try:
                q_dev.write(b"\xa5" * (32 * max(m - 1, 1)))
                value = gm_ctx.poly_div_linear(cname, f_dev, pyref.encode_fr(c, z), q_dev, m)
                S = _suffix(c.r, F, z)
                assert value == S[0].to_bytes(32, "little"), (zname, "value")
                if kind == "multiple_of_x_minus_z":
                    assert value == bytes(32), (zname, "f(z) != 0")
                if m > 1:
                    assert q_dev.to_host(32 * (m - 1)) == _bytes(S[1:m]), (zname, "quotient")
                assert f_dev.to_host() == fb, (zname, "f changed")
            finally:
                f_dev.free()
    finally:
        q_dev.free()


@pytest.mark.parametrize("cname", CURVE_NAMES)
def test_poly_div_linear_refuses_overlap(gm_ctx, cname):
    import gnark_mi355x as gm
    c = pyref.CURVES[cname]
    m = 70
    buf = gm_ctx.malloc(32 * 3 * m)
    z = pyref.encode_fr(c, 5)
    try:
        buf.write(_bytes(_random_mont(3 * m, 1)))
        f = gm.DeviceBuffer(gm_ctx, buf.ptr + 32 * m, 32 * m)
        for off in (0, 1, m - 1, -1, -(m - 2)):
            q = gm.DeviceBuffer(gm_ctx, f.ptr + 32 * off, 32 * (m - 1))
            with pytest.raises(gm.GmError):
                gm_ctx.poly_div_linear(cname, f, z, q, m)
        # touching ranges do not overlap
        for off in (m, -(m - 1)):
            q = gm.DeviceBuffer(gm_ctx, f.ptr + 32 * off, 32 * (m - 1))
            gm_ctx.poly_div_linear(cname, f, z, q, m)
        with pytest.raises(gm.GmError):
            gm_ctx.poly_div_linear(cname, f, z, buf, 0)
    finally:
        buf.free()


def _ragged(c, n):
    lens = [n + 2, n + 3, n + 3, n + 3, n, 0]
    return lens, [pyref.random_scalars(c, m, 0x90 + i) for i, m in enumerate(lens)]


def _eval(r, f, z):
    acc = 0
    for a in reversed(f):
        acc = (acc * z + a) % r
    return acc


def _quotient(r, f, fz, z):
    f = list(f)
    f[0] = (f[0] - fz) % r
    for i in range(len(f) - 2, -1, -1):
        f[i] = (f[i] + f[i + 1] * z) % r
    return f[1:]


def _fold(r, polys, gamma):
    out = [0] * max(len(f) for f in polys)
    gi = 1
    for f in polys:
        for j, a in enumerate(f):
            out[j] = (out[j] + gi * a) % r
        gi = gi * gamma % r
    return out


def _upload(gm_ctx, c, polys):
    enc = lambda vals: b"".join(pyref.encode_fr(c, v) for v in vals)
    return [gm_ctx.copy_to_device(enc(f)) if f else None for f in polys]


def _free(bufs):
    for b in bufs:
        if b is not None:
            b.free()


@pytest.mark.parametrize("logn", [6, 12])
@pytest.mark.parametrize("cname", CURVE_NAMES)
def test_kzg_eval_and_fold_ragged(gm_ctx, cname, logn):
    c = pyref.CURVES[cname]
    r = c.r
    lens, polys = _ragged(c, 1 << logn)
    bufs = _upload(gm_ctx, c, polys)
    out = gm_ctx.malloc(32 * max(lens))
    try:
        for zname, z in _points(c):
            got = gm_ctx.kzg_eval(cname, bufs, pyref.encode_fr(c, z), lens)
            assert got == [pyref.encode_fr(c, _eval(r, f, z)) for f in polys], zname
        for gname, gamma in (("random", pyref.random_scalars(c, 1, 0x82)[0]), ("zero", 0), ("one", 1)):
            out.write(b"\xa5" * (32 * max(lens)))
            gm_ctx.poly_fold(cname, bufs, pyref.encode_fr(c, gamma), out, lens)
            want = b"".join(pyref.encode_fr(c, v) for v in _fold(r, polys, gamma))
            assert out.to_host() == want, gname
        # polynomials in another order: the short ones first, the empty one in the middle
        order = [4, 5, 0, 3]
        gamma = pyref.random_scalars(c, 1, 0x83)[0]
        out.write(b"\xa5" * (32 * max(lens)))
        gm_ctx.poly_fold(cname, [bufs[i] for i in order], pyref.encode_fr(c, gamma), out, [lens[i] for i in order])
        want = b"".join(pyref.encode_fr(c, v) for v in _fold(r, [polys[i] for i in order], gamma))
        assert out.to_host() == want
    finally:
        _free(bufs)
        out.free()


def test_kzg_eval_more_polynomials_than_one_launch_takes(gm_ctx):
    """65538 short polynomials (views of one buffer): the evaluation runs in more
    than one batch of the grid's second dimension."""
    import gnark_mi355x as gm
    cname = "bls12377"
    c = pyref.CURVES[cname]
    k = 65535 + 3
    vals = pyref.random_scalars(c, k + 2, 0x44)
    buf = gm_ctx.copy_to_device(b"".join(pyref.encode_fr(c, v) for v in vals))
    z = pyref.random_scalars(c, 1, 0x45)[0]
    try:
        lens = [1 + i % 3 for i in range(k)]
        views = [gm.DeviceBuffer(gm_ctx, buf.ptr + 32 * i, 32 * lens[i]) for i in range(k)]
        got = gm_ctx.kzg_eval(cname, views, pyref.encode_fr(c, z), lens)
        for i in (0, 1, 2, 65534, 65535, 65536, k - 1):
            assert got[i] == pyref.encode_fr(c, _eval(c.r, vals[i:i + lens[i]], z)), i
        want = [_eval(c.r, vals[i:i + lens[i]], z) for i in range(k)]
        assert got == [pyref.encode_fr(c, v) for v in want]
    finally:
        buf.free()


def _srs(oracle, gm, cname, size, tau):
    c = pyref.CURVES[cname]
    powers = b"".join(pyref.encode_fr(c, pow(tau, i, c.r)) for i in range(size))
    return oracle.batch_mul_base(cname, False, gm.generator(cname), powers)


@pytest.mark.parametrize("cname,logn", [("bls12377", 6), ("bls12377", 10), ("bn254", 6),
                                        ("bls12381", 6), ("bls12381", 10)])
def test_kzg_open_and_batch_open(gm_ctx, oracle, cname, logn):
    import gnark_mi355x as gm
    c = pyref.CURVES[cname]
    r = c.r
    n = 1 << logn
    pb = gm.point_bytes(cname, False)
    enc = lambda vals: b"".join(pyref.encode_fr(c, v) for v in vals)
    tau = pyref.random_scalars(c, 1, 0x79)[0]
    srs = _srs(oracle, gm, cname, n + 3, tau)
    d_srs = gm_ctx.points_upload(cname, srs)
    gen = gm.generator(cname)
    z = pyref.random_scalars(c, 1, 0x80)[0]
    zb = pyref.encode_fr(c, z)

    def check_h(h, f, fz, what):
        q = _quotient(r, f, fz, z)
        assert h == oracle.msm(cname, False, enc(q), srs[:pb * len(q)]), what
        k = (_eval(r, f, tau) - fz) * pow(tau - z, -1, r) % r
        assert h == oracle.batch_mul_base(cname, False, gen, enc([k])), what + ": != [(f(tau) - f(z)) / (tau - z)] G"

    lens, polys = _ragged(c, n)
    bufs = _upload(gm_ctx, c, polys)
    try:
        # kzg.Open: blinded Z has n + 3 coefficients, the SRS size
        f = polys[1]
        claimed, h = gm_ctx.kzg_open(cname, d_srs, bufs[1], zb)
        assert claimed == pyref.encode_fr(c, _eval(r, f, z))
        check_h(h, f, _eval(r, f, z), "open")
        # kzg.BatchOpenSinglePoint: claimed values, then gamma, then the folded opening
        values = gm_ctx.kzg_eval(cname, bufs, zb, lens)
        assert values == [pyref.encode_fr(c, _eval(r, g, z)) for g in polys]
        gamma = pyref.random_scalars(c, 1, 0x82)[0]
        fv, h = gm_ctx.kzg_batch_open(cname, d_srs, bufs, zb, pyref.encode_fr(c, gamma), lens)
        folded_value = 0
        for v in reversed([_eval(r, g, z) for g in polys]):
            folded_value = (folded_value * gamma + v) % r
        assert fv == pyref.encode_fr(c, folded_value)
        check_h(h, _fold(r, polys, gamma), folded_value, "batch open")
        # constant polynomials: the zero quotient, H = (0, 0)
        one = gm_ctx.copy_to_device(enc([7]))
        padded = gm_ctx.copy_to_device(enc([7, 0, 0, 0]))
        try:
            assert gm_ctx.kzg_open(cname, d_srs, one, zb) == (pyref.encode_fr(c, 7), bytes(pb))
            assert gm_ctx.kzg_open(cname, d_srs, padded, zb) == (pyref.encode_fr(c, 7), bytes(pb))
            fv, h = gm_ctx.kzg_batch_open(cname, d_srs, [one, one], zb, pyref.encode_fr(c, gamma))
            assert (fv, h) == (pyref.encode_fr(c, 7 * (1 + gamma)), bytes(pb))
        finally:
            one.free()
            padded.free()
        # kzg.ErrInvalidPolynomialSize
        long = gm_ctx.copy_to_device(enc([1] * (n + 4)))
        try:
            with pytest.raises(gm.GmError):
                gm_ctx.kzg_open(cname, d_srs, long, zb)
            with pytest.raises(gm.GmError):
                gm_ctx.kzg_batch_open(cname, d_srs, [bufs[0], long], zb, pyref.encode_fr(c, gamma))
            with pytest.raises(gm.GmError):
                gm_ctx.kzg_batch_open(cname, d_srs, [], zb, pyref.encode_fr(c, gamma))
        finally:
            long.free()
    finally:
        _free(bufs)
        d_srs.free()


@pytest.mark.parametrize("cname", CURVE_NAMES)
def test_small_division_after_large_ignores_old_scratch(gm_ctx, cname):
    """The chunk and value scratch comes from the context's workspace, which a
    larger call leaves full of its own values: a small division before and after
    a large one gives the same, correct bytes."""
    c = pyref.CURVES[cname]
    z = pyref.random_scalars(c, 1, 0x51)[0]
    zb = pyref.encode_fr(c, z)

    def divide(F):
        m = len(F)
        f_dev = gm_ctx.copy_to_device(_bytes(F))
        q_dev = gm_ctx.malloc(32 * (m - 1))
        try:
            value = gm_ctx.poly_div_linear(cname, f_dev, zb, q_dev, m)
            return value, q_dev.to_host()
        finally:
            f_dev.free()
            q_dev.free()

    small = _random_mont(65, 0x52)
    S = _suffix(c.r, small, z)
    want = (S[0].to_bytes(32, "little"), _bytes(S[1:65]))
    assert divide(small) == want
    big = [int.from_bytes(pyref.encode_fr(c, c.r - 1), "little")] * ((1 << 16) + 3)
    Sb = _suffix(c.r, big, z)
    assert divide(big) == (Sb[0].to_bytes(32, "little"), _bytes(Sb[1:len(big)]))
    assert divide(small) == want
