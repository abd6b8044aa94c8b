#!/usr/bin/env python3
"""CPU model of the G1 bucket accumulation's lockstep work: the slice grid (K
consecutive sorted entries per lane, whatever the bucket) against the piece plan
(buckets cut into ceil(len / T) pieces of nearly equal length, pieces sorted by
length, longest first; MsmPlan in csrc/msm.hpp).

Digits are uniform: every window of c bits puts each of the n points into one
of its 2^(c-1) buckets.  Work is counted in wave steps (64 lanes in lockstep):
an accumulation step is one mixed add, a fixup step one full XYZZ add, priced
at FULL_ADD mixed adds.

    python tools/piece_plan_model.py --n 2097152 --c 16 --windows 8 --K 24 --T 32 48 0

T = 0 means whole buckets (no cut)."""
import argparse

import numpy as np

WAVE = 64
FULL_ADD = 1.45   # 12M + 2S against 8M + 2S, plus the heavier glue
FIX_SERIAL = 8


def bucket_lengths(n, c, windows, seed):
    rng = np.random.default_rng(seed)
    nb = 1 << (c - 1)
    return np.concatenate([np.bincount(rng.integers(0, nb, n), minlength=nb) for _ in range(windows)])


def wave_max(a):
    """Sum over waves of 64 consecutive lanes of the lanes' maximum."""
    pad = (-len(a)) % WAVE
    a = np.concatenate([a, np.zeros(pad, a.dtype)])
    return int(a.reshape(-1, WAVE).max(axis=1).sum())


def slice_grid(lens, K):
    off = np.concatenate([[0], np.cumsum(lens)])
    M = int(off[-1])
    nslices = (M + K - 1) // K
    ne = lens > 0
    span = np.where(ne, (off[1:] - 1) // K - off[:-1] // K, 0)
    return {
        "lanes": nslices,
        "waves": (nslices + WAVE - 1) // WAVE,
        "accum_steps": ((nslices + WAVE - 1) // WAVE) * K,   # every step is an add for some lane
        "copy_steps": 0,
        "extra_parts": int(span.sum()),
        "fixup_adds": int(span.sum()),
        "fixup_wave_adds": wave_max(span),                    # one thread per bucket
        "fixup_wave_adds_sorted": wave_max(np.sort(span)[::-1]),
        "long_buckets": int((span > FIX_SERIAL).sum()),
    }


def piece_plan(lens, T):
    lens = lens[lens > 0]
    p = np.ones_like(lens) if T == 0 else (lens + T - 1) // T
    q, r = lens // p, lens % p
    # r pieces of q + 1 entries and p - r of q
    pl = np.concatenate([np.repeat(q + 1, r), np.repeat(q, p - r)])
    pl = np.sort(pl)[::-1]
    pad = (-len(pl)) % WAVE
    lead = np.concatenate([pl, np.zeros(pad, pl.dtype)]).reshape(-1, WAVE)[:, 0]
    adds = p - 1
    return {
        "lanes": len(pl),
        "waves": len(lead),
        "accum_steps": int((lead - 1).sum()),   # the first entry of a piece is a copy
        "copy_steps": len(lead),
        "extra_parts": int(adds.sum()),
        "fixup_adds": int(adds.sum()),
        "fixup_wave_adds": wave_max(adds),
        "fixup_wave_adds_sorted": wave_max(np.sort(adds)[::-1]),
        "long_buckets": int((adds > FIX_SERIAL).sum()),
        "max_piece": int(pl[0]) if len(pl) else 0,
    }


def total(r, sorted_fixup):
    f = r["fixup_wave_adds_sorted"] if sorted_fixup else r["fixup_wave_adds"]
    return r["accum_steps"] + FULL_ADD * f


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--n", type=int, default=1 << 21, help="points per window (2 n0 with the GLV split)")
    ap.add_argument("--c", type=int, default=16)
    ap.add_argument("--windows", type=int, default=8)
    ap.add_argument("--K", type=int, default=24, help="slice length of the grid to compare with")
    ap.add_argument("--T", type=int, nargs="+", default=[24, 32, 48, 0])
    ap.add_argument("--seed", type=int, default=1)
    a = ap.parse_args()
    lens = bucket_lengths(a.n, a.c, a.windows, a.seed)
    print(f"n={a.n} c={a.c} windows={a.windows}: {len(lens)} buckets, {int(lens.sum())} entries, "
          f"len {lens.mean():.1f} +- {lens.std():.1f} (max {lens.max()})")
    base = slice_grid(lens, a.K)
    rows = [(f"slices K={a.K}", base)] + [(f"pieces T={t}" if t else "whole buckets", piece_plan(lens, t)) for t in a.T]
    print(f"{'plan':16s} {'lanes':>9s} {'waves':>7s} {'accum':>9s} {'copy':>7s} {'fix adds':>9s} "
          f"{'fix wave':>9s} {'sorted':>8s} {'total':>9s} {'vs grid':>8s} {'sorted':>8s}")
    t0 = total(base, False)
    for name, r in rows:
        tu, ts = total(r, False), total(r, True)
        print(f"{name:16s} {r['lanes']:9d} {r['waves']:7d} {r['accum_steps']:9d} {r['copy_steps']:7d} "
              f"{r['fixup_adds']:9d} {r['fixup_wave_adds']:9d} {r['fixup_wave_adds_sorted']:8d} "
              f"{tu:9.0f} {100 * (tu / t0 - 1):+7.1f}% {100 * (ts / t0 - 1):+7.1f}%")


if __name__ == "__main__":
    main()
