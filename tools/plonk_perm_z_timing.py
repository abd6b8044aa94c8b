#!/usr/bin/env python3
"""Times the PLONK permutation polynomial Z on resident wires, and the device
share of the stage with and without it (not part of bench.py).

  python tools/plonk_perm_z_timing.py [--reps 3] [--warmup 1] [--out profiles/plonk_perm_z_timing.json]
                                      [--cases bls12377:4194304,bn254:1048576]

Per case (BLS12-377 n = 2^22, BN254 n = 2^20), in one process, the legs
alternating after a warm-up:
  (a) perm_z_resident   gm_plonk_perm_z on resident inputs, both outputs written:
                        the device-event bracket of the whole call (profile scope
                        plonk_perm_z_call), its three kernels and the transform to
                        the canonical form beside it, and the host wall clock.
                        perm_z_and_commit adds gm_msm_prepared reading z_lagrange
                        where it lies: the new path of the stage.
  (b) host_z_path       what the device does for this stage without the call: Z
                        comes from the host, so gm_kzg_commit uploads it and runs
                        the MSM over the Lagrange SRS, and one gm_copy_to_device of
                        n elements brings the canonical Z the quotient needs.  The
                        host's own work on Z (iop.BuildRatioCopyConstraint, the
                        inverse FFT) is left out, so (b) is a lower bound on the
                        old stage.
The two n-sized kernels are set against two bounds:
  HBM      7 x 32 B per row (six reads, one write) at 8 TB/s; as written both
           kernels read the six inputs, 13 x 32 B per row
  Fr mul   the products per row as plonk_perm.hip is written at the 150 Gmul/s the
           radix-2^29 product reaches (field.hpp): 10 for num and den in either
           kernel, 2 for the chunk products, 2 for the run products, 3.5 for the
           scan over the runs (14 per run of 4) and 2 for Z: 29.5
No speed-up over gnark-crypto's CPU stage is claimed (no Go toolchain).
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
BYTES_PER_ROW = 7 * 32
BYTES_PER_ROW_AS_WRITTEN = 13 * 32
MULS_PER_ROW = 29.5
KERNELS = ("plonk_perm_chunk_prod", "plonk_perm_carry", "plonk_perm_write")


def _scopes(ctx):
    """{scope: (total ms, count)} since the last reset."""
    ctx.synchronize()
    st = ctx.profile_stats()
    ctx.profile_reset()
    return st


def _stats(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs)}


def run_case(gm, ctx, curve, n, reps, warmup):
    polys = {k: ctx.random_scalars(curve, n, 61 + i) for i, k in enumerate(gm.PLONK_PERM_POLYS)}
    small = ctx.random_scalars(curve, 2, 70).to_host()
    beta, gamma = small[:32], small[32:64]
    zl, zc = ctx.malloc(32 * n), ctx.malloc(32 * n)
    k = ctx.random_scalars(curve, n, 71)
    pts = ctx.batch_mul_base(curve, False, gm.generator(curve), k, n)
    srs = ctx.points_upload(curve, pts.to_host())
    pts.free()
    k.free()
    z_host = None
    digests = {}

    def leg_a():
        ctx.plonk_perm_z(curve, n, polys, beta, gamma, zl, zc)

    def leg_a_commit():
        digests["resident"] = ctx.msm_prepared(curve, zl, srs, n)[1]

    def leg_b():
        digests["host"] = ctx.kzg_commit(curve, srs, z_host)
        ctx.copy_to_device(z_host).free()

    rec = {"call_event_ms": [], "call_wall_ms": [], "commit_wall_ms": [], "new_path_wall_ms": [],
           "host_z_path_wall_ms": []}
    kern = []
    try:
        for it in range(warmup + reps):
            ctx.profile_reset()
            t0 = time.perf_counter()
            leg_a()
            t1 = time.perf_counter()
            st = _scopes(ctx)
            t2 = time.perf_counter()
            leg_a_commit()
            t3 = time.perf_counter()
            if z_host is None:
                z_host = np.frombuffer(zl.to_host(), np.uint8).copy()
            ctx.profile_reset()
            t4 = time.perf_counter()
            leg_b()
            t5 = time.perf_counter()
            ctx.profile_reset()
            if it >= warmup:
                rec["call_event_ms"].append(st["plonk_perm_z_call"][0])
                rec["call_wall_ms"].append((t1 - t0) * 1e3)
                rec["commit_wall_ms"].append((t3 - t2) * 1e3)
                rec["new_path_wall_ms"].append((t1 - t0 + t3 - t2) * 1e3)
                rec["host_z_path_wall_ms"].append((t5 - t4) * 1e3)
                kern.append({s: v[0] for s, v in st.items()})
        same = digests["resident"] == digests["host"]
    finally:
        for b in list(polys.values()) + [zl, zc, srs]:
            b.free()
    res = {"curve": curve, "n": n, "reps": reps, "warmup": warmup, "digests_equal": same}
    res["perm_z_resident"] = {"event_ms": _stats(rec["call_event_ms"]), "wall_ms": _stats(rec["call_wall_ms"])}
    res["perm_z_and_commit"] = {"wall_ms": _stats(rec["new_path_wall_ms"]),
                                "commit_wall_ms": _stats(rec["commit_wall_ms"])}
    res["host_z_path"] = {"wall_ms": _stats(rec["host_z_path_wall_ms"])}
    a, b = res["perm_z_and_commit"]["wall_ms"]["median"], res["host_z_path"]["wall_ms"]["median"]
    res["new_over_host_z_path"] = a / b
    res["new_path_is_shorter"] = a < b
    res["scope_ms_per_call"] = {s: statistics.median(c[s] for c in kern) for s in kern[0]}
    sc = res["scope_ms_per_call"]
    k_ms = sc["plonk_perm_chunk_prod"] + sc["plonk_perm_write"]
    t_hbm = BYTES_PER_ROW * n / HBM_BYTES_PER_S * 1e3
    t_hbm_w = BYTES_PER_ROW_AS_WRITTEN * n / HBM_BYTES_PER_S * 1e3
    t_mul = MULS_PER_ROW * n / FR_MUL_PER_S * 1e3
    res["kernels"] = {
        "ms_per_call": {s: sc[s] for s in KERNELS},
        "canonical_ms_per_call": sc.get("plonk_perm_canonical"),
        "row_kernels_ms": k_ms,
        "bytes_per_s_as_written": BYTES_PER_ROW_AS_WRITTEN * n / (k_ms * 1e-3),
        "fr_mul_per_s": MULS_PER_ROW * n / (k_ms * 1e-3),
        "hbm_bound_ms": t_hbm, "hbm_as_written_ms": t_hbm_w, "fr_mul_bound_ms": t_mul,
        "bound": "fr_mul_issue" if t_mul > t_hbm_w else "hbm",
        "frac_of_bound": max(t_hbm_w, t_mul) / k_ms,
    }
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--cases", default="bls12377:%d,bn254:%d" % (1 << 22, 1 << 20))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "plonk_perm_z_timing.json"))
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
    doc = {"tool": "tools/plonk_perm_z_timing.py",
           "timing": "leg (a): device events on the context stream (profile scopes) and host wall clock; "
                     "leg (b) and the commit: host wall clock of the synchronous calls",
           "not_measured": "the host's own construction of Z and its inverse FFT in the replaced stage "
                           "(no Go toolchain)",
           "results": results}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(doc, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
