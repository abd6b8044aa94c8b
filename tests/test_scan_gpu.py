"""gm_test_scan: the device-wide exclusive u32 scan (csrc/scan.hpp) and the
one-block max scan on their own, against numpy.

device_excl_scan works in blocks of 4096 words whose totals one block of 1024
threads scans in slices, so the lengths sit where a kernel can go wrong: around
a wave (63, 64, 65), around a block (4095, 4096, 4097, 2 * 4096), where every
thread of the top level owns exactly one block total (1024 * 4096), where the
first thread's slice becomes two (1024 * 4096 + 1), and one block beyond the
8192 totals the earlier scans staged in LDS (8192 * 4096 + 1).  Every case runs
out of place and in place, over a workspace of 0xFF bytes, and with a poisoned
word behind the output."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

BLK = 4096
POISON = 0xA5C3E187
SUM_LENGTHS = (0, 1, 63, 64, 65, 4095, 4096, 4097, 2 * BLK, 1024 * BLK, 1024 * BLK + 1, 8192 * BLK + 1)
PATTERNS = ("random", "zeros", "last_one")
MAX_LENGTHS = (0, 1, 1023, 1024, 1025, 98305)


def excl_sum(v):
    """n + 1 words: the exclusive prefix sums and the total, mod 2^32"""
    out = np.zeros(v.size + 1, np.uint64)
    np.cumsum(v, dtype=np.uint64, out=out[1:])
    return out


def sum_case(n, pattern):
    if pattern == "random":
        v = np.random.default_rng(0x5CA9 + n).integers(0, 100, n, dtype=np.uint32)
    else:
        v = np.zeros(n, np.uint32)
        if pattern == "last_one" and n:
            v[-1] = 1
    want = excl_sum(v)
    assert int(want[-1]) < 1 << 32
    return v, want.astype(np.uint32)


def run_sum(ctx, v, want):
    n = v.size
    for in_place in (False, True):
        init = np.full(n + 2, POISON, np.uint32)
        if in_place:
            init[:n] = v
        got = np.frombuffer(ctx.test_scan(0, init, n, None if in_place else v), np.uint32)
        assert got.size == n + 2
        bad = np.flatnonzero(got[:n + 1] != want)
        assert bad.size == 0, (in_place, bad.size, bad[:8].tolist(), got[bad[:8]].tolist(), want[bad[:8]].tolist())
        assert got[n + 1] == POISON, in_place


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("n", SUM_LENGTHS)
def test_excl_scan(gm_ctx, n, pattern):
    run_sum(gm_ctx, *sum_case(n, pattern))


def test_excl_scan_wraps(gm_ctx):
    v = np.full(5, 0xFFFFFFFF, np.uint32)
    run_sum(gm_ctx, v, (excl_sum(v) & 0xFFFFFFFF).astype(np.uint32))


def max_case(n, pattern):
    """Mostly zeros.  "heads": 1 + the index at sparse places, as the wires
    permutation's link scans them (increasing); "mixed": sparse random values, so
    most of them lie below the running maximum."""
    rng = np.random.default_rng(0x3A5 + n)
    v = np.zeros(n, np.uint32)
    at = np.flatnonzero(rng.random(n) < 0.05)
    v[at] = at + 1 if pattern == "heads" else rng.integers(1, 1 << 32, at.size, dtype=np.uint64)
    want = np.zeros(n, np.uint32)
    if n > 1:
        want[1:] = np.maximum.accumulate(v)[:-1]
    return v, want


@pytest.mark.parametrize("pattern", ("heads", "mixed"))
@pytest.mark.parametrize("n", MAX_LENGTHS)
def test_block_max_scan(gm_ctx, n, pattern):
    v, want = max_case(n, pattern)
    for in_place in (False, True):
        init = np.full(n + 1, POISON, np.uint32)
        if in_place:
            init[:n] = v
        got = np.frombuffer(gm_ctx.test_scan(1, init, n, None if in_place else v), np.uint32)
        assert got.size == n + 1
        bad = np.flatnonzero(got[:n] != want)
        assert bad.size == 0, (in_place, bad.size, bad[:8].tolist(), got[bad[:8]].tolist(), want[bad[:8]].tolist())
        assert got[n] == POISON, in_place
