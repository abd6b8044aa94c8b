#!/usr/bin/env python3
"""Times a KZG opening on resident polynomials against the GPU share of the
opening it replaces (not part of bench.py).

  python tools/kzg_open_timing.py [--reps 10] [--warmup 3] [--out profiles/kzg_open_timing.json]
                                  [--cases bls12377:4194307,bn254:1048579]

Per case (BLS12-377 m = 2^22 + 3, BN254 m = 2^20 + 3), in one process, the two
legs alternating after a warm-up:
  (a) commit_host_quotient  gm_kzg_commit of a host quotient of m - 1 coefficients:
                            the upload and the MSM, all the GPU did for an opening
                            while the division ran on the host
  (b) open_resident         gm_kzg_open on a resident polynomial of m coefficients:
                            evaluation, division and the MSM of the quotient
Both are device-event brackets of the whole call on the context's stream
(profile scopes kzg_commit_call / kzg_open_call), with the host wall clock of the
synchronous call beside them.  The three division kernels and the fold (six
polynomials of m coefficients) are timed on their own the same way, and the
division is set against its two bounds:
  HBM      96 B per coefficient (f read twice, q written once) at 8 TB/s
  Fr mul   3.75 products per coefficient as kzg.hip is written (evaluation: 7/8
           Horner + 1/8 tree; write: 7/8 Horner + 1 recompute + 7/8 scan) at the
           150 Gmul/s the radix-2^29 product reaches (field.hpp)
The host Horner, fold and division time that the opening no longer needs is not
measured here (no Go): no speed-up over gnark-crypto is claimed.
"""
import argparse
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
DIV_BYTES_PER_COEFF = 96
DIV_MULS_PER_COEFF = 3.75
DIV_KERNELS = ("kzg_chunk_eval", "kzg_chunk_carry", "kzg_div_write")


def _scopes(ctx):
    """{scope: (total ms, count)} since the last reset."""
    ctx.synchronize()
    st = ctx.profile_stats()
    ctx.profile_reset()
    return st


def run_case(gm, ctx, curve, m, reps, warmup):
    f = ctx.random_scalars(curve, m, 11)
    qd = ctx.random_scalars(curve, m - 1, 12)
    q_host = np.frombuffer(qd.to_host(), np.uint8)
    qd.free()
    k = ctx.random_scalars(curve, m, 13)
    pts = ctx.batch_mul_base(curve, False, gm.generator(curve), k, m)
    srs = ctx.points_upload(curve, pts.to_host())
    pts.free()
    k.free()
    z = ctx.random_scalars(curve, 2, 14).to_host()
    z, gamma = z[:32], z[32:]
    q_dev = ctx.malloc(32 * (m - 1))
    out = ctx.malloc(32 * m)
    polys = [f] * 6
    legs = {"commit_host_quotient": {"event_ms": [], "wall_ms": []}, "open_resident": {"event_ms": [], "wall_ms": []}}
    try:
        for it in range(warmup + reps):
            for name, scope, call in (
                    ("commit_host_quotient", "kzg_commit_call", lambda: ctx.kzg_commit(curve, srs, q_host)),
                    ("open_resident", "kzg_open_call", lambda: ctx.kzg_open(curve, srs, f, z, m))):
                ctx.profile_reset()
                t0 = time.perf_counter()
                call()
                wall = (time.perf_counter() - t0) * 1e3
                st = _scopes(ctx)
                if it >= warmup:
                    legs[name]["event_ms"].append(st[scope][0])
                    legs[name]["wall_ms"].append(wall)
        for _ in range(warmup):
            ctx.poly_div_linear(curve, f, z, q_dev, m)
            ctx.poly_fold(curve, polys, gamma, out)
        ctx.profile_reset()
        for _ in range(reps):
            ctx.poly_div_linear(curve, f, z, q_dev, m)
            ctx.poly_fold(curve, polys, gamma, out)
        st = _scopes(ctx)
    finally:
        for b in (f, srs, q_dev, out):
            b.free()
    kern = {name: st[name][0] / st[name][1] for name in DIV_KERNELS + ("kzg_fold",)}
    div_ms = sum(kern[name] for name in DIV_KERNELS)
    t_hbm = DIV_BYTES_PER_COEFF * m / HBM_BYTES_PER_S * 1e3
    t_mul = DIV_MULS_PER_COEFF * m / FR_MUL_PER_S * 1e3
    res = {"curve": curve, "m": m, "reps": reps, "warmup": warmup}
    for name, v in legs.items():
        res[name] = {"event_ms_median": statistics.median(v["event_ms"]), "event_ms_min": min(v["event_ms"]),
                     "event_ms_max": max(v["event_ms"]), "wall_ms_median": statistics.median(v["wall_ms"])}
    a, b = res["commit_host_quotient"]["event_ms_median"], res["open_resident"]["event_ms_median"]
    res["open_over_commit"] = b / a
    res["kernel_avg_ms"] = kern
    res["division"] = {
        "ms": div_ms,
        "bytes_per_s": DIV_BYTES_PER_COEFF * m / (div_ms * 1e-3),
        "frac_of_8TBps": DIV_BYTES_PER_COEFF * m / (div_ms * 1e-3) / HBM_BYTES_PER_S,
        "hbm_bound_ms": t_hbm, "fr_mul_bound_ms": t_mul,
        "bound": "fr_mul_issue" if t_mul > t_hbm else "hbm",
        "frac_of_bound": max(t_hbm, t_mul) / div_ms,
    }
    res["fold"] = {"polys": len(polys), "ms": kern["kzg_fold"],
                   "bytes_per_s": 32 * m * (len(polys) + 1) / (kern["kzg_fold"] * 1e-3)}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--cases", default="bls12377:%d,bn254:%d" % ((1 << 22) + 3, (1 << 20) + 3))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kzg_open_timing.json"))
    a = ap.parse_args()
    import gnark_mi355x as gm
    results = []
    with gm.Context(0) as ctx:
        ctx.profile(True)
        for case in a.cases.split(","):
            curve, m = case.split(":")
            r = run_case(gm, ctx, curve, int(m), a.reps, a.warmup)
            results.append(r)
            print(json.dumps(r), flush=True)
    doc = {"tool": "tools/kzg_open_timing.py", "timing": "device events on the context stream (profile scopes)",
           "not_measured": "host Horner, fold and division of the replaced opening (no Go toolchain)",
           "results": results}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(doc, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
