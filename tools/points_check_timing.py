#!/usr/bin/env python3
"""Times the point check beside its sibling, in one process (not part of
bench.py, not a test).

  python tools/points_check_timing.py [--reps 5] [--warmup 1] [--sizes 20,22] [--key 20]
                                      [--out profiles/points_check_timing.json]

Medians of `reps` runs with min and max after `warmup` runs (ms).  Per curve and
group, n = 2^k per --sizes:
  device   gm_points_check over resident points: host wall clock of the
           synchronous call, and the kernel's own time (HIP events around the
           launch, gm_profile_*) from a second set of runs
  host     gm_points_check_host over the same points in pageable host memory:
           wall clock, the kernels' summed time from a second set of runs, and
           what is left of the wall clock (staging memcpy and PCIe not hidden
           behind the kernels) as `outside_kernels_share`
  sibling  gm_batch_mul_base at the same n (curve ids 0 and 1, which it serves):
           a per-lane ladder of 254 doublings, about 127 additions and one
           inversion; wall clock of the synchronous call
  key      BN254 and BLS12-377: a synthetic key at 2^--key through gm_g16_pk_check
`ops_per_point` records the counted doublings and additions of each test
(tools/subgroup_constants.py op_counts).  Points: 4096 small multiples of the
generator with random signs, tiled -- all in the subgroup, so every lane runs the
whole test.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for sub_ in ("gnark-icicle_amd", "oracle", "tests", "tools"):
    sys.path.insert(0, os.path.join(ROOT, sub_))
import pyref  # noqa: E402
import subgroup_constants as sub  # noqa: E402

CURVES = ("bn254", "bls12377", "bls12381")
SIBLING_CURVES = ("bn254", "bls12377")
NBASES = 4096
SIBLING_OPS = {"doublings": 254, "additions": 127, "inversions": 1}


def _stats(xs):
    return {"median": round(statistics.median(xs), 4), "min": round(min(xs), 4), "max": round(max(xs), 4)}


def _timed(fn, reps, warmup):
    ms = []
    for it in range(warmup + reps):
        t0 = time.perf_counter()
        fn()
        if it >= warmup:
            ms.append((time.perf_counter() - t0) * 1e3)
    return _stats(ms)


def _kernel_ms(ctx, fn, reps, names):
    """Per-run summed event time of the kernels `names`, profiling switched on for these runs only."""
    ms = []
    ctx.profile(True)
    try:
        for _ in range(reps):
            ctx.profile_reset()
            fn()
            st = ctx.profile_stats()
            ms.append(sum(st[k][0] for k in names if k in st))
    finally:
        ctx.profile(False)
    return _stats(ms)


_BASES = {}


def points(curve, g2, n, seed):
    key = (curve, g2)
    if key not in _BASES:
        c = sub.curve_params(curve)
        G = pyref.Group(c, g2)
        g, acc, pos, neg = G.generator(), None, [], []
        for _ in range(NBASES):
            acc = G.add(acc, g)
            pos.append(pyref.encode_point(c, acc, g2))
            neg.append(pyref.encode_point(c, G.neg(acc), g2))
        _BASES[key] = np.frombuffer(b"".join(pos + neg), np.uint8).reshape(2 * NBASES, len(pos[0]))
    rng = np.random.default_rng(seed)
    return _BASES[key][rng.integers(0, 2 * NBASES, n)].reshape(-1)


def clean(rep, n):
    assert rep["n"] == n and rep["first_bad"] == n and rep["infinities"] == 0, rep


def time_group(gm, ctx, curve, g2, n, reps, warmup):
    host = points(curve, g2, n, 23)
    kname = ["points_check_g2" if g2 else "points_check_g1"]
    out = {"bytes": int(host.size)}
    P = ctx.copy_points_to_device(curve, host, g2)
    try:
        dev = lambda: clean(ctx.points_check(curve, P, n, g2), n)
        out["device_wall"] = _timed(dev, reps, warmup)
        out["device_kernel"] = _kernel_ms(ctx, dev, reps, kname)
        if curve in SIBLING_CURVES:
            S = ctx.random_scalars(curve, n, 77)
            base = gm.generator(curve, g2)
            try:
                out["sibling_batch_mul_base_wall"] = _timed(
                    lambda: ctx.batch_mul_base(curve, g2, base, S, n).free(), reps, warmup)
            finally:
                S.free()
    finally:
        P.free()
    hst = lambda: clean(ctx.points_check_host(curve, host, g2), n)
    out["host_wall"] = _timed(hst, reps, warmup)
    out["host_kernels"] = _kernel_ms(ctx, hst, reps, kname)
    w, k = out["host_wall"]["median"], out["host_kernels"]["median"]
    out["host_outside_kernels_share"] = round(max(w - k, 0.0) / w, 3)
    out["host_gb_per_s"] = round(host.size / w / 1e6, 2)
    return out


def time_key(gm, ctx, curve, logn, reps, warmup):
    n = 1 << logn
    nb_wires, nb_public = n + 2, 2
    g1 = lambda cnt, seed: points(curve, False, cnt, seed)
    pk = {"g1_alpha": g1(1, 1), "g1_beta": g1(1, 2), "g1_delta": g1(1, 3), "g1_A": g1(nb_wires, 4),
          "g1_B": g1(nb_wires, 5), "g1_Z": g1(n - 1, 6), "g1_K": g1(nb_wires - nb_public, 7),
          "g2_beta": points(curve, True, 1, 8), "g2_delta": points(curve, True, 1, 9),
          "g2_B": points(curve, True, nb_wires, 10),
          "infA": np.zeros(nb_wires, np.uint8), "infB": np.zeros(nb_wires, np.uint8)}

    def once():
        rep = ctx.g16_pk_check(curve, pk, n, nb_wires, nb_public)
        assert rep["first_bad_member"] is None
    out = {"g1_points": int(sum(pk[k].size for k in ("g1_A", "g1_B", "g1_Z", "g1_K")) // gm.point_bytes(curve, False)),
           "g2_points": nb_wires, "bytes": int(sum(v.size for k, v in pk.items() if k.startswith("g")))}
    out["wall"] = _timed(once, reps, warmup)
    out["kernels"] = _kernel_ms(ctx, once, reps, ["points_check_g1", "points_check_g2"])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--sizes", default="20,22")
    ap.add_argument("--key", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "points_check_timing.json"))
    a = ap.parse_args()
    import gnark_mi355x as gm
    res = {"reps": a.reps, "warmup": a.warmup, "unit": "ms", "lib_bytes": os.path.getsize(gm.LIB_PATH),
           "ops_per_point": {"sibling_batch_mul_base": SIBLING_OPS}, "groups": {}, "key": {}}
    for curve in CURVES:
        d = sub.derive(curve)
        for g2 in (False, True):
            dbl, add = sub.op_counts(d, g2)
            res["ops_per_point"]["%s_%s" % (curve, "g2" if g2 else "g1")] = {"doublings": dbl, "additions": add}
    with gm.Context(0) as ctx:
        for k in [int(x) for x in a.sizes.split(",") if x]:
            for curve in CURVES:
                for g2 in (False, True):
                    key = "%s_%s_2p%d" % (curve, "g2" if g2 else "g1", k)
                    res["groups"][key] = time_group(gm, ctx, curve, g2, 1 << k, a.reps, a.warmup)
                    print(key, json.dumps(res["groups"][key]), flush=True)
            ctx.trim()
        if a.key:
            for curve in SIBLING_CURVES:
                res["key"]["%s_2p%d" % (curve, a.key)] = time_key(gm, ctx, curve, a.key, a.reps, a.warmup)
                print("key", curve, json.dumps(res["key"]["%s_2p%d" % (curve, a.key)]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
