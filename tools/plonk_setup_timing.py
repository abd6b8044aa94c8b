#!/usr/bin/env python3
"""Times the PLONK setup on the device (gm_kzg_srs_lagrange, gm_plonk_pk_setup)
against gm_plonk_pk_upload of the same key (not part of bench.py, not a test).

  python tools/plonk_setup_timing.py [--reps 3] [--warmup 1] [--out profiles/plonk_setup_timing.json]
                                     [--cases bls12377:4194304,bn254:1048576]

Per case (BLS12-377 n = 2^22, BN254 n = 2^20, nb_bsb = 0, two public inputs), in
one process, medians of `reps` runs with min-max after `warmup` runs:
  (a) lagrange   gm_kzg_srs_lagrange alone on resident points, by device events
                 (profiling scope kzg_srs_lagrange), with the count of group
                 operations it performed (from the twiddles' digits, counted here) and
                 its share of the VALU mad bound: operations x products per
                 operation x mads per product over 30.7 T mad/s
  (b) setup      gm_plonk_pk_setup whole, host wall clock: canonical SRS, selectors
                 and the permutation in; key, digests and Lagrange points out
  (c) upload     gm_plonk_pk_upload of the same key, with the Lagrange SRS (b)
                 returned and s1, s2, s3 from gm_plonk_sigma given from the host: the
                 path before, without the CPU work it presupposes; (b) - (c) is
                 what the derivation costs, not a speed-up
The canonical SRS is n + 3 random multiples of G (no tau is known), so
correctness is checked through the transform's own identity: for random Lagrange
values v the commit over the derived SRS equals the commit of their canonical
form (device inverse NTT) over the canonical SRS.  The keys of (b) and (c) must
report the same bytes.  Not measured: gnark-crypto's CPU ToLagrangeG1 (no Go
toolchain), so no ratio against it.
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
sys.path.insert(0, os.path.join(ROOT, "oracle"))

NB_PUBLIC = 2
MAD_PEAK = 30.7e12
# field products per complete XYZZ operation (curve.hpp) and v_mad_u64_u32 per product (2 N^2, N radix-2^29 limbs)
DBL_PRODUCTS, ADD_PRODUCTS = 9, 14
LIMBS = {"bn254": 9, "bls12377": 14}
SCALAR_BITS = 256    # the loop doubles once per bit of the 8-word twiddle


def _stats(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs), "spread": max(xs) - min(xs)}


def _host(ctx, curve, k, seed):
    b = ctx.random_scalars(curve, k, seed)
    try:
        return b.to_host()
    finally:
        b.free()


def group_ops(curve, n):
    """Doublings and additions of one gm_kzg_srs_lagrange, from its definition: stage
    s of log2 n has n/2 butterflies of two additions and, but for the 2^s with
    twiddle 1, a 256-step double-and-add by the non-adjacent form of w^(-j 2^s); the
    last pass multiplies n points by 1/n."""
    import pyref
    c = pyref.CURVES[curve]
    r, logn = c.r, n.bit_length() - 1
    winv = pow(pyref.domain_generator(c, n), -1, r)
    pops, t = [], 1
    for _ in range(n // 2):
        pops.append(bin((3 * t) ^ t).count("1"))   # non-zero digits of the non-adjacent form
        t = t * winv % r
    pops = np.array(pops, np.int64)
    muls = adds = 0
    for s in range(logn):
        muls += n // 2 - (1 << s)
        adds += n + (int(pops[::1 << s].sum()) - 1) * (1 << s)   # pops[0] = 1 is the skipped twiddle
    muls += n
    ninv = pow(n, -1, r)
    adds += n * bin((3 * ninv) ^ ninv).count("1")
    return {"scalar_multiplications": muls, "doublings": muls * SCALAR_BITS, "additions": adds}


def run_case(gm, ctx, curve, n, reps, warmup):
    pb = gm.point_bytes(curve, False)
    host = lambda seed, k=n: np.frombuffer(_host(ctx, curve, k, seed), np.uint8)
    sel = {k: host(201 + i) for i, k in enumerate(gm.PLONK_SETUP_POLYS)}
    perm = np.random.default_rng(7).permutation(3 * n).astype(np.int64)
    k = ctx.random_scalars(curve, n + 3, 231)
    can_dev = ctx.batch_mul_base(curve, False, gm.generator(curve), k, n + 3)
    k.free()
    can = can_dev.to_host()
    out = {"curve": curve, "n": n, "nb_public": NB_PUBLIC, "nb_bsb": 0, "reps": reps, "warmup": warmup}

    # (a) the transform alone
    lag_dev = ctx.malloc(pb * n)
    ev = []
    ctx.profile(True)
    for it in range(warmup + reps):
        ctx.profile_reset()
        ctx.kzg_srs_lagrange(curve, can_dev, n, lag_dev)
        ms, cnt = ctx.profile_stats()["kzg_srs_lagrange"]
        assert cnt == 1
        if it >= warmup:
            ev.append(ms)
    ctx.profile(False)
    ctx.profile_reset()
    ops = group_ops(curve, n)
    mads = (ops["doublings"] * DBL_PRODUCTS + ops["additions"] * ADD_PRODUCTS) * 2 * LIMBS[curve] ** 2
    med = statistics.median(ev)
    out["lagrange"] = {"event_ms": _stats(ev), "group_operations": ops,
                       "products_per_operation": {"doubling": DBL_PRODUCTS, "addition": ADD_PRODUCTS},
                       "mads_per_product": 2 * LIMBS[curve] ** 2, "mads": mads,
                       "share_of_mad_bound": mads / MAD_PEAK / (med * 1e-3)}
    # the identity sum_i v_i out[i] = sum_j iNTT(v)_j in[j]
    v = ctx.random_scalars(curve, n, 241)
    _, over_lagrange = ctx.msm(curve, v, lag_dev, n)
    ctx.ntt(curve, v, n, 1, 0, 0)       # inverse, DIF: bit-reversed coefficients
    ctx.reverse_scalars(curve, v, n)
    _, over_canonical = ctx.msm(curve, v, can_dev, n)
    out["lagrange"]["commit_identity_holds"] = over_lagrange == over_canonical
    lag_first = lag_dev.to_host()
    for b in (v, lag_dev, can_dev):
        b.free()

    # (b) the whole setup, (c) the upload of the same key
    s_dev = ctx.plonk_sigma(curve, n, perm)
    s_host = [np.frombuffer(b.to_host(), np.uint8) for b in s_dev]
    for b in s_dev:
        b.free()
    full = dict(sel, s1=s_host[0], s2=s_host[1], s3=s_host[2])
    rec = {"setup": [], "upload": []}
    sizes, lag = {}, None
    for it in range(warmup + reps):
        t0 = time.perf_counter()
        key, digests, lag = gm.PlonkProvingKey.setup(ctx, curve, n, NB_PUBLIC, sel, perm, [], [], can, lagrange=True)
        t1 = time.perf_counter()
        sizes["setup"] = key.resident_bytes()
        key.free()
        t2 = time.perf_counter()
        key = gm.PlonkProvingKey(ctx, curve, n, NB_PUBLIC, full, [], [], can, lag)
        t3 = time.perf_counter()
        sizes["upload"] = key.resident_bytes()
        key.free()
        if it >= warmup:
            rec["setup"].append((t1 - t0) * 1e3)
            rec["upload"].append((t3 - t2) * 1e3)
    out["setup_wall_ms"] = _stats(rec["setup"])
    out["upload_wall_ms"] = _stats(rec["upload"])
    out["derivation_ms"] = out["setup_wall_ms"]["median"] - out["upload_wall_ms"]["median"]
    out["key_bytes"] = sizes["setup"][0]
    out["keys_report_equal_bytes"] = sizes["setup"] == sizes["upload"]
    out["setup_lagrange_equals_the_call_alone"] = lag == lag_first
    out["host_bytes_in"] = {"setup": 32 * 5 * n + 8 * 3 * n + pb * (n + 3), "upload": 32 * 8 * n + pb * (2 * n + 3)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--cases", default="bls12377:%d,bn254:%d" % (1 << 22, 1 << 20))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "plonk_setup_timing.json"))
    a = ap.parse_args()
    if a.reps < 3:
        ap.error("medians of at least three runs")
    import gnark_mi355x as gm
    results = []
    with gm.Context(0) as ctx:
        for case in a.cases.split(","):
            curve, n = case.split(":")
            r = run_case(gm, ctx, curve, int(n), a.reps, a.warmup)
            results.append(r)
            print(json.dumps(r), flush=True)
            ctx.trim()
    doc = {"tool": "tools/plonk_setup_timing.py",
           "timing": "the transform by device events; setup and upload by the host wall clock of synchronous calls; "
                     "one process, the two key entries alternating after the warm-up",
           "not_measured": "gnark-crypto's CPU ToLagrangeG1 (no Go toolchain): no ratio against it is claimed",
           "results": results}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(doc, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
