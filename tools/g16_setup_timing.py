#!/usr/bin/env python3
"""Times the Groth16 setup on the device (not part of bench.py, not a test).

  python tools/g16_setup_timing.py [--reps 5] [--warmup 1] [--log2n 20] [--sweep 8,12,13,14,16]
                                   [--setup bn254:20,bls12377:20,bn254:22] [--oracle 20]
                                   [--out profiles/g16_setup_timing.json]

One process; medians of `reps` runs with min and max after `warmup` runs, every run
on fresh seeded inputs.

(a) gm_batch_mul_fixed against the double-and-add entry it stands beside
(gm_batch_mul_base) on the same scalars, per curve and group, n = 2^log2n:
  base      gm_batch_mul_base, host wall clock of the synchronous call
  fixed     gm_batch_mul_fixed at the model's window, host wall clock, and its
            ratio to base; the outputs of the last run are compared byte for byte
  sweep     gm_batch_mul_fixed at each forced window c: wall clock and, by device
            events (profiling scopes), the shares of the table build (its own
            normalisation included), the multiply kernel and the normalisation of
            the results
  G1 only:  the multiply kernel's time per mixed addition, n W additions counted
            (a digit is zero with probability 2^-c), beside the MSM accumulation
            kernel's 77 ps per addition

(b) gm_g16_setup and gm_g16_pk_setup of squaring_chain_fast(2^k - 1) (2^k
constraints, 2^k + 2 wires) per --setup case: host wall clock of each call
(gm_g16_setup without its gm_g16_setup_sizes pass, which sizes the buffers first),
and by device events the stages of gm_g16_setup: Lagrange values, transpose, column
sums, compaction, K / Z scalars, G1 points, G2 points, the copy to the host.  The
setup's arrays of the last run are compared with the key gm_g16_pk_setup made by
proving with both.  Beside it, for constraint counts up to 2^--oracle, one run of
the test oracle's g16_setup on 16 threads: the project's C++ port of Setup, not
gnark-crypto.
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

FR_BITS = {"bn254": 254, "bls12377": 253}
SCOPES = ("fixed_base_table", "fixed_base_mul", "fixed_base_normalise")
ACC_PS_PER_ADD = 77.0


def _stats(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs)}


def _wall(fn):
    t0 = time.perf_counter()
    out = fn()
    return (time.perf_counter() - t0) * 1e3, out


def windows(curve, c):
    return (FR_BITS[curve] + 1 + c - 1) // c


def run_case(gm, ctx, curve, g2, n, reps, warmup, sweep):
    base = gm.generator(curve, g2)
    out = ctx.malloc(gm.point_bytes(curve, g2) * n)
    seed = [1000]

    def fresh():
        seed[0] += 1
        return ctx.random_scalars(curve, n, seed[0])

    def timed(call):
        ms = []
        for it in range(warmup + reps):
            k = fresh()
            t, res = _wall(lambda: call(k))
            if res is not None and res is not out:
                res.free()
            k.free()
            if it >= warmup:
                ms.append(t)
        return ms

    rec = {"curve": curve, "group": "g2" if g2 else "g1", "n": n, "reps": reps, "warmup": warmup}
    rec["base_wall_ms"] = _stats(timed(lambda k: ctx.batch_mul_base(curve, g2, base, k, n)))
    ctx.set_fixed_base_window(0)
    rec["fixed_wall_ms"] = _stats(timed(lambda k: ctx.batch_mul_fixed(curve, g2, base, k, n, out=out)))
    rec["ratio_base_over_fixed"] = rec["base_wall_ms"]["median"] / rec["fixed_wall_ms"]["median"]
    k = fresh()
    ref = ctx.batch_mul_base(curve, g2, base, k, n)
    ctx.batch_mul_fixed(curve, g2, base, k, n, out=out)
    rec["outputs_equal"] = ref.to_host() == out.to_host()
    ref.free()
    k.free()

    rec["sweep"] = []
    for c in sweep:
        ctx.set_fixed_base_window(c)
        W = windows(curve, c)
        row = {"c": c, "W": W, "table_entries": W << (c - 1),
               "table_bytes": (W << (c - 1)) * gm.point_bytes(curve, g2)}
        row["wall_ms"] = _stats(timed(lambda k: ctx.batch_mul_fixed(curve, g2, base, k, n, out=out)))
        shares = {s: [] for s in SCOPES}
        ctx.profile(True)
        for it in range(warmup + reps):
            k = fresh()
            ctx.profile_reset()
            ctx.batch_mul_fixed(curve, g2, base, k, n, out=out)
            st = ctx.profile_stats()
            k.free()
            if it >= warmup:
                for s in SCOPES:
                    shares[s].append(st[s][0])
        ctx.profile(False)
        ctx.profile_reset()
        row["event_ms"] = {s: _stats(v) for s, v in shares.items()}
        if not g2:
            ps = row["event_ms"]["fixed_base_mul"]["median"] * 1e9 / (n * W)
            row["mul_ps_per_add"] = ps
            row["mul_ps_per_add_over_accumulation"] = ps / ACC_PS_PER_ADD
        rec["sweep"].append(row)
    ctx.set_fixed_base_window(0)
    best = min(rec["sweep"], key=lambda r: r["wall_ms"]["median"])
    rec["fastest_swept_c"] = best["c"]
    out.free()
    return rec


SETUP_SCOPES = ("g16_setup_lagrange", "g16_setup_transpose", "g16_setup_columns", "g16_setup_compact", "g16_setup_kz",
                "g16_setup_g1", "g16_setup_g2", "g16_setup_d2h")
ORACLE_THREADS = 16


def run_setup_case(gm, ctx, curve, logn, reps, warmup, oracle_max):
    import ctypes
    import pyref
    import r1cs as R
    c = pyref.CURVES[curve]
    k = (1 << logn) - 1
    r1, W, a, b, cc = R.squaring_chain_fast(k, curve)
    table = b"".join(pyref.encode_fr(c, v) for v in (0, 1, 2, c.r - 1, c.r - 2))
    ones = [np.ones(r1.nc, np.uint32)] * 3
    h = gm.R1CS(ctx, curve, r1.nc, r1.nb_wires, r1.rowptr, ones, r1.wires, table)
    L = gm.load_library()
    rng = np.random.default_rng(2024 + logn)

    def fresh_toxic():
        return b"".join(pyref.encode_fr(c, int.from_bytes(rng.bytes(31), "little") + 2) for _ in range(5))

    rec = {"curve": curve, "nb_constraints": r1.nc, "nb_wires": r1.nb_wires, "nb_public": r1.nb_public,
           "reps": reps, "warmup": warmup}
    wall, key_wall = [], []
    stages = {s: [] for s in SETUP_SCOPES}
    tox = None
    for it in range(warmup + reps):
        tox = fresh_toxic()
        ain, out, collect, _keep = h._setup_out(tox, r1.nb_public, None)
        t, rc = _wall(lambda: L.gm_g16_setup(ctx.handle, h.handle, ctypes.byref(ain), ctypes.byref(out)))
        assert rc == 0
        tk, key = _wall(lambda: gm.ProvingKey.setup(ctx, h, tox, r1.nb_public))
        key.free()
        if it >= warmup:
            wall.append(t)
            key_wall.append(tk)
    ctx.profile(True)
    for it in range(warmup + reps):
        tox = fresh_toxic()
        ain, out, collect, _keep = h._setup_out(tox, r1.nb_public, None)
        ctx.profile_reset()
        assert L.gm_g16_setup(ctx.handle, h.handle, ctypes.byref(ain), ctypes.byref(out)) == 0
        st = ctx.profile_stats()
        if it >= warmup:
            for s in SETUP_SCOPES:
                stages[s].append(st.get(s, (0.0, 0))[0])
    ctx.profile(False)
    ctx.profile_reset()
    rec["setup_wall_ms"] = _stats(wall)
    rec["pk_setup_wall_ms"] = _stats(key_wall)
    rec["stage_event_ms"] = {s: _stats(v) for s, v in stages.items()}
    # the two entries make the same key: one proof from each
    pk = collect()
    r_, s_ = pyref.encode_fr(c, 0x77777), pyref.encode_fr(c, 0x99999)
    k1 = gm.ProvingKey(ctx, curve, pk, r1.domain_size, r1.nb_wires, r1.nb_public)
    p1 = k1.prove_r1cs(h, W, r_, s_)
    k1.free()
    k2 = gm.ProvingKey.setup(ctx, h, tox, r1.nb_public)
    p2 = k2.prove_r1cs(h, W, r_, s_)
    k2.free()
    rec["both_keys_give_the_same_proof"] = p1 == p2
    if logn <= oracle_max:
        import oracle_lib
        t, want = _wall(lambda: oracle_lib.g16_setup(curve, r1, tox, ORACLE_THREADS))
        rec["oracle_cpp_port"] = {"threads": ORACLE_THREADS, "runs": 1, "wall_ms": t,
                                  "arrays_equal": all(bytes(pk[x]) == bytes(want[x]) for x in
                                                      ("g1_A", "g1_B", "g1_Z", "g1_K", "g2_B", "infA", "infB"))}
        rec["oracle_over_setup"] = t / rec["setup_wall_ms"]["median"]
    else:
        rec["oracle_cpp_port"] = "not run at this size"
    h.free()
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--log2n", type=int, default=20)
    ap.add_argument("--sweep", default="8,12,13,14,16")
    ap.add_argument("--setup", default="bn254:20,bls12377:20,bn254:22")
    ap.add_argument("--oracle", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "g16_setup_timing.json"))
    a = ap.parse_args()
    if a.reps < 5:
        ap.error("medians of at least five runs")
    import gnark_mi355x as gm
    sweep = [int(c) for c in a.sweep.split(",")]
    results = []
    with gm.Context(0) as ctx:
        for curve in ("bn254", "bls12377"):
            for g2 in (False, True):
                r = run_case(gm, ctx, curve, g2, 1 << a.log2n, a.reps, a.warmup, sweep)
                results.append(r)
                print(json.dumps(r), flush=True)
                ctx.trim()
        setups = []
        for case in [x for x in a.setup.split(",") if x]:
            curve, logn = case.split(":")
            r = run_setup_case(gm, ctx, curve, int(logn), a.reps, a.warmup, a.oracle)
            setups.append(r)
            print(json.dumps(r), flush=True)
            ctx.trim()
    doc = {"tool": "tools/g16_setup_timing.py",
           "timing": "host wall clock of synchronous calls (table build included in every fixed-base call); "
                     "shares by device events around each stage; one process, fresh seeded scalars per run",
           "accumulation_ps_per_add": ACC_PS_PER_ADD,
           "oracle": "oracle_cpp_port is the test oracle's g16_setup (oracle/, this project's C++ port of Setup), one "
                     "run on 16 threads; it is not gnark-crypto, which was not measured (no Go toolchain)",
           "results": results, "setup": setups}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(doc, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
