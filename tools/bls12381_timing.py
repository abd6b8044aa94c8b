#!/usr/bin/env python3
"""Times BLS12-381 (curve id 2) beside its nearest siblings, in one process (not
part of bench.py, not a test).

  python tools/bls12381_timing.py [--reps 5] [--warmup 1] [--sizes 20,22] [--ntt 24] [--g16 20]
                                  [--out profiles/bls12381_timing.json]

Medians of `reps` runs with min and max after `warmup` runs; host wall clock of the
synchronous call (ms).
  msm     gm_msm, G1 and G2, n = 2^k per --sizes, GLV forced on and off, beside
          BLS12-377 (the same limb counts: 14 / 9) at the same size; the winner
          per size decides the curve's GLV default (msm_glv_on)
  precomp gm_msm_precomputed, G1, 2^20, the automatic window
  ntt     gm_ntt forward DIF and inverse DIT at 2^--ntt beside BN254 (9 limbs)
  g16     gm_g16_prove_device at 2^--g16 on a synthetic key (points tiled from the
          bases below; the proof is not checked), plain key, beside BLS12-377
Points: 4096 small multiples of the generator with random signs, tiled (no
fixed-base multiplication exists for this curve yet); scalars: gm_random_scalars.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for sub in ("gnark-icicle_amd", "oracle", "tests"):
    sys.path.insert(0, os.path.join(ROOT, sub))
import pyref  # noqa: E402
import bls12381_params as bp  # noqa: E402

PARAMS = {"bls12381": bp.BLS12_381, "bls12377": pyref.CURVES["bls12377"], "bn254": pyref.CURVES["bn254"]}
NBASES = 4096


def _stats(xs):
    return {"median": round(statistics.median(xs), 4), "min": round(min(xs), 4), "max": round(max(xs), 4)}


def _timed(fn, reps, warmup):
    ms = []
    for it in range(warmup + reps):
        t0 = time.perf_counter()
        fn(it)
        if it >= warmup:
            ms.append((time.perf_counter() - t0) * 1e3)
    return _stats(ms)


_BASES = {}


def points(curve, g2, n, seed):
    """n gnark-layout points: the bases [1]G..[4096]G and their negatives, drawn at random"""
    key = (curve, g2)
    if key not in _BASES:
        c = PARAMS[curve]
        G = pyref.Group(c, g2)
        g, acc, pos, neg = G.generator(), None, [], []
        for _ in range(NBASES):
            acc = G.add(acc, g)
            pos.append(pyref.encode_point(c, acc, g2))
            neg.append(pyref.encode_point(c, G.neg(acc), g2))
        pb = len(pos[0])
        _BASES[key] = np.frombuffer(b"".join(pos + neg), np.uint8).reshape(2 * NBASES, pb)
    rng = np.random.default_rng(seed)
    return _BASES[key][rng.integers(0, 2 * NBASES, n)].reshape(-1)


def time_msm(gm, ctx, curve, g2, n, reps, warmup):
    P = ctx.copy_points_to_device(curve, points(curve, g2, n, 17), g2)
    S = [ctx.random_scalars(curve, n, 100 + i) for i in range(2)]
    out = {}
    try:
        for mode, name in ((1, "glv_on"), (0, "glv_off")):
            ctx.set_msm_glv(mode)
            out[name] = _timed(lambda it: ctx.msm(curve, S[it & 1], P, n, g2), reps, warmup)
        ctx.set_msm_glv(-1)
        out["winner"] = min(("glv_on", "glv_off"), key=lambda k: out[k]["median"])
    finally:
        ctx.set_msm_glv(-1)
        for x in S + [P]:
            x.free()
    return out


def time_precomp(gm, ctx, curve, n, reps, warmup):
    P = ctx.points_upload_precomputed(curve, points(curve, False, n, 19), False, window=0)
    S = [ctx.random_scalars(curve, n, 200 + i) for i in range(2)]
    try:
        return _timed(lambda it: ctx.msm_precomputed(curve, S[it & 1], P, n, False), reps, warmup)
    finally:
        for x in S + [P]:
            x.free()


def time_ntt(gm, ctx, curve, logn, reps, warmup):
    n = 1 << logn
    X = ctx.random_scalars(curve, n, 7)
    try:
        ctx.ntt(curve, X, n, False, False, False)  # builds the domain
        return {"forward_dif": _timed(lambda it: ctx.ntt(curve, X, n, False, False, False), reps, warmup),
                "inverse_dit": _timed(lambda it: ctx.ntt(curve, X, n, True, True, False), reps, warmup),
                "coset_forward_dit": _timed(lambda it: ctx.ntt(curve, X, n, False, True, True), reps, warmup)}
    finally:
        X.free()


def time_g16(gm, ctx, curve, logn, reps, warmup):
    n = 1 << logn
    nb_wires, nb_public = n + 2, 2
    g1 = lambda cnt, seed: points(curve, False, cnt, seed)
    pk = {"g1_alpha": g1(1, 1), "g1_beta": g1(1, 2), "g1_delta": g1(1, 3), "g1_A": g1(nb_wires, 4),
          "g1_B": g1(nb_wires, 5), "g1_Z": g1(n - 1, 6), "g1_K": g1(nb_wires - nb_public, 7),
          "g2_beta": points(curve, True, 1, 8), "g2_delta": points(curve, True, 1, 9),
          "g2_B": points(curve, True, nb_wires, 10),
          "infA": np.zeros(nb_wires, np.uint8), "infB": np.zeros(nb_wires, np.uint8)}
    dpk = gm.ProvingKey(ctx, curve, pk, n, nb_wires, nb_public)
    W = ctx.random_scalars(curve, nb_wires, 31)
    src = [ctx.random_scalars(curve, n, 32 + i) for i in range(3)]
    abc = [ctx.malloc(32 * n) for _ in range(3)]
    r = ctx.random_scalars(curve, 2, 40).to_host()
    try:
        def once(it):
            for d, s in zip(abc, src):
                d.copy_from(s)
            ctx.synchronize()
            dpk.prove_device(W, *abc, n, r[:32], r[32:])
        t_copy = _timed(lambda it: ([d.copy_from(s) for d, s in zip(abc, src)], ctx.synchronize()), reps, warmup)
        return {"prove_device_incl_input_copy": _timed(once, reps, warmup), "input_copy_alone": t_copy}
    finally:
        for x in [W] + src + abc:
            x.free()
        dpk.free()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--sizes", default="20,22")
    ap.add_argument("--ntt", type=int, default=24)
    ap.add_argument("--g16", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bls12381_timing.json"))
    a = ap.parse_args()
    import gnark_mi355x as gm
    res = {"reps": a.reps, "warmup": a.warmup, "unit": "ms, host wall clock of the synchronous call",
           "lib_bytes": os.path.getsize(gm.LIB_PATH), "msm": {}, "precomputed_g1_2p20": {}, "ntt": {}, "g16": {}}
    with gm.Context(0) as ctx:
        for k in [int(x) for x in a.sizes.split(",") if x]:
            for g2 in (False, True):
                for curve in ("bls12381", "bls12377"):
                    key = "%s_%s_2p%d" % (curve, "g2" if g2 else "g1", k)
                    res["msm"][key] = time_msm(gm, ctx, curve, g2, 1 << k, a.reps, a.warmup)
                    print(key, json.dumps(res["msm"][key]), flush=True)
        for curve in ("bls12381", "bls12377"):
            res["precomputed_g1_2p20"][curve] = time_precomp(gm, ctx, curve, 1 << 20, a.reps, a.warmup)
            print("precomp", curve, json.dumps(res["precomputed_g1_2p20"][curve]), flush=True)
        ctx.trim()
        if a.ntt:
            for curve in ("bls12381", "bn254"):
                res["ntt"]["%s_2p%d" % (curve, a.ntt)] = time_ntt(gm, ctx, curve, a.ntt, a.reps, a.warmup)
                print("ntt", curve, json.dumps(res["ntt"]["%s_2p%d" % (curve, a.ntt)]), flush=True)
        ctx.trim()
        if a.g16:
            for curve in ("bls12381", "bls12377"):
                res["g16"]["%s_2p%d" % (curve, a.g16)] = time_g16(gm, ctx, curve, a.g16, a.reps, a.warmup)
                print("g16", curve, json.dumps(res["g16"]["%s_2p%d" % (curve, a.g16)]), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
