#!/usr/bin/env python3
"""Times the PLONK quotient on resident polynomials against the device share of
the per-transform path it replaces (not part of bench.py).

  python tools/plonk_quotient_timing.py [--reps 3] [--warmup 1] [--out profiles/plonk_quotient_timing.json]
                                        [--cases bls12377:4194304,bn254:1048576]

Per case (BLS12-377 n = 2^22, BN254 n = 2^20, nb_bsb = 0), in one process, the two
legs alternating after a warm-up:
  (a) quotient_resident   gm_plonk_quotient on resident inputs: the device-event
                          bracket of the whole call (profile scope
                          plonk_quotient_call) and the host wall clock beside it
  (b) per_transform       what the Go hook issues for the same stage today, one
                          transform at a time as gm.NTT does it (gm_copy_to_device,
                          gm_ntt, gm_memcpy_d2h, gm_free): 4 cosets x 12 polynomials
                          x 2 transforms, the 12 restoring inverse transforms, and
                          the 4n inverse coset transform.  Host wall clock.  The
                          host scaling and the host constraint evaluation between
                          those calls are left out, so (b) is a lower bound on the
                          old stage.
The constraint kernel (scope plonk_constraint, four launches per call) is set
against its two bounds over the 4n points:
  HBM      (13 reads + 1 write) x 32 B per point at 8 TB/s
  Fr mul   32 products per point as plonk.hip is written (x and x^2: 2, blinding:
           10, gate: 5, permutation: 13, L1 term: 2) at the 150 Gmul/s the
           radix-2^29 product reaches (field.hpp)
No speed-up over gnark-crypto's CPU stage is claimed (no Go toolchain).
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gnark-icicle_amd"))

HBM_BYTES_PER_S = 8e12
FR_MUL_PER_S = 150e9
BYTES_PER_POINT = 14 * 32
MULS_PER_POINT = 32


def _scopes(ctx):
    """{scope: (total ms, count)} since the last reset."""
    ctx.synchronize()
    st = ctx.profile_stats()
    ctx.profile_reset()
    return st


def _round_trip(gm, L, ctx, cid, host, n, inverse, dit, coset):
    """gm.NTT of the Go binding: copy in, transform, copy out, free."""
    dev = ctypes.c_void_p()
    p = host.ctypes.data_as(ctypes.c_void_p)
    gm._check(L.gm_copy_to_device(ctx.handle, p, host.size, ctypes.byref(dev)))
    try:
        gm._check(L.gm_ntt(ctx.handle, cid, dev, n, int(inverse), int(dit), int(coset)))
        gm._check(L.gm_memcpy_d2h(ctx.handle, p, dev, host.size))
    finally:
        gm._check(L.gm_free(ctx.handle, dev))


def run_case(gm, ctx, curve, n, reps, warmup):
    L = gm.load_library()
    cid = gm.curve_id(curve)
    polys = {k: ctx.random_scalars(curve, n, 21 + i) for i, k in enumerate(gm.PLONK_POLYS)}
    small = ctx.random_scalars(curve, 12, 40).to_host()
    blinds = {"bl": small[:64], "br": small[64:128], "bo": small[128:192], "bz": small[192:288]}
    alpha, beta, gamma = small[288:320], small[320:352], small[352:384]
    h = ctx.malloc(32 * 4 * n)
    host_n = np.frombuffer(polys["l"].to_host(), np.uint8).copy()
    host_4n = np.frombuffer(h.to_host(), np.uint8).copy()

    def leg_a():
        ctx.plonk_quotient(curve, n, polys, [], [], blinds, alpha, beta, gamma, h)

    def leg_b():
        for _coset in range(4):
            for _poly in range(12):
                _round_trip(gm, L, ctx, cid, host_n, n, True, False, False)   # ToCanonical
                _round_trip(gm, L, ctx, cid, host_n, n, False, True, False)   # scaled, ToLagrange
        for _poly in range(12):
            _round_trip(gm, L, ctx, cid, host_n, n, True, False, False)       # restore
        _round_trip(gm, L, ctx, cid, host_4n, 4 * n, True, True, True)        # divideByZH

    legs = {"quotient_resident": {"event_ms": [], "wall_ms": []}, "per_transform": {"wall_ms": []}}
    kern = []
    try:
        for it in range(warmup + reps):
            ctx.profile_reset()
            t0 = time.perf_counter()
            leg_a()
            wall = (time.perf_counter() - t0) * 1e3
            st = _scopes(ctx)
            if it >= warmup:
                legs["quotient_resident"]["event_ms"].append(st["plonk_quotient_call"][0])
                legs["quotient_resident"]["wall_ms"].append(wall)
                kern.append({k: v[0] for k, v in st.items()})
            t0 = time.perf_counter()
            leg_b()
            wall = (time.perf_counter() - t0) * 1e3
            ctx.profile_reset()
            if it >= warmup:
                legs["per_transform"]["wall_ms"].append(wall)
    finally:
        for b in list(polys.values()) + [h]:
            b.free()
    res = {"curve": curve, "n": n, "nb_bsb": 0, "reps": reps, "warmup": warmup}
    for name, v in legs.items():
        res[name] = {k + "_median": statistics.median(x) for k, x in v.items()}
        res[name].update({k + "_min": min(x) for k, x in v.items()})
        res[name].update({k + "_max": max(x) for k, x in v.items()})
    a, b = res["quotient_resident"]["wall_ms_median"], res["per_transform"]["wall_ms_median"]
    res["resident_over_per_transform"] = a / b
    res["resident_is_faster"] = a < b
    res["scope_ms_per_call"] = {k: statistics.median(c[k] for c in kern) for k in kern[0]}
    k_ms = res["scope_ms_per_call"]["plonk_constraint"]
    pts = 4 * n
    t_hbm = BYTES_PER_POINT * pts / HBM_BYTES_PER_S * 1e3
    t_mul = MULS_PER_POINT * pts / FR_MUL_PER_S * 1e3
    res["constraint_kernel"] = {
        "ms_per_call": k_ms, "launches_per_call": 4,
        "bytes_per_s": BYTES_PER_POINT * pts / (k_ms * 1e-3),
        "fr_mul_per_s": MULS_PER_POINT * pts / (k_ms * 1e-3),
        "hbm_bound_ms": t_hbm, "fr_mul_bound_ms": t_mul,
        "bound": "fr_mul_issue" if t_mul > t_hbm else "hbm",
        "frac_of_bound": max(t_hbm, t_mul) / k_ms,
    }
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--cases", default="bls12377:%d,bn254:%d" % (1 << 22, 1 << 20))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "plonk_quotient_timing.json"))
    a = ap.parse_args()
    import gnark_mi355x as gm
    results = []
    with gm.Context(0) as ctx:
        ctx.profile(True)
        for case in a.cases.split(","):
            curve, n = case.split(":")
            r = run_case(gm, ctx, curve, int(n), a.reps, a.warmup)
            results.append(r)
            print(json.dumps(r), flush=True)
            ctx.trim()
    doc = {"tool": "tools/plonk_quotient_timing.py",
           "timing": "leg (a): device events on the context stream (profile scopes) and host wall clock; "
                     "leg (b): host wall clock of the synchronous calls",
           "not_measured": "host scaling and host constraint evaluation of the replaced stage (no Go toolchain)",
           "results": results}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(doc, fh, indent=1)
        fh.write("\n")
    if not all(r["resident_is_faster"] for r in results):
        sys.exit("the resident quotient is not faster than the per-transform path")


if __name__ == "__main__":
    main()
