#!/usr/bin/env python3
"""Times the PLONK permutation derived on the device from resident wire tables
(gm_plonk_wires_permutation, gm_plonk_sigma_wires) against the path before it,
gm_plonk_sigma from a host permutation (not part of bench.py, not a test).

  python tools/plonk_wires_perm_timing.py [--reps 5] [--warmup 1] [--out profiles/plonk_wires_perm_timing.json]
                                          [--cases bls12377:4194304,bn254:1048576]

Per case and nb_wires in (n, n / 2), in one process, medians of `reps` runs with
min-max after `warmup` runs.  The tables are uniform random ids with the last
eighth of the rows padding (0, 0, 0), so that wire 0 has one long run.
  (1) permutation   gm_plonk_wires_permutation alone: the whole call and its stages
                    by device events (each pass's histogram, scan and scatter,
                    then the link), and the host wall clock of the call, with the
                    bytes a stage moves by this tool's own count (the passes carry
                    the key beside the position; the variant that re-gathered it
                    through the position is in profiles/plonk_wires_perm_keys_ab.json)
  (2) sigma_wires   gm_plonk_sigma_wires, host wall clock and device events
  (3) sigma_host    gm_plonk_sigma from the same permutation held on the host: the
                    range check of 3n entries, the 24 n byte pageable upload and
                    the kernel; the host construction of the permutation, which
                    that path presupposes, is excluded
  (4) numpy         for information only: the permutation built on the host by
                    numpy (a stable argsort), which is not gnark's buildPermutation
                    loop and not what a Go caller would run
The device permutation must equal (4) entry for entry, and (2) must equal (3) byte
for byte.
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

TILE, DIGITS, LINK_TILE = 2048, 256, 1024


def _stats(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs), "spread": max(xs) - min(xs)}


def perm_numpy(lro):
    order = np.argsort(lro, kind="stable")
    k = lro[order]
    head = np.r_[True, k[1:] != k[:-1]]
    tail = np.r_[head[1:], True]
    prev = np.r_[0, order[:-1]]
    rid = np.cumsum(head) - 1
    prev[head] = order[tail][rid[head]]
    perm = np.empty_like(order)
    perm[order] = prev
    return perm.astype(np.int64)


def stage_bytes(N, passes):
    """Bytes the stages ask for, counted from the kernels' definitions (4-byte
    positions and keys)."""
    cells = DIGITS * ((N + TILE - 1) // TILE)
    out = {}
    for p in range(passes):
        out["hist_%d" % p] = 4 * N + 4 * cells               # keys in, counts out
        out["scan_%d" % p] = 4 * cells * 4                   # the local scan and the add: each reads and writes the counts
        read = 4 * N if p == 0 else 8 * N                     # the first pass reads the tables; then position + key
        out["scatter_%d" % p] = read + 4 * cells + 8 * N      # offsets in, position + key out
    out["link"] = 8 * N + 8 * N + 8 * ((N + LINK_TILE - 1) // LINK_TILE)   # position + key in, int64 out
    return out


def measure_permutation(gm, ctx, w, want, reps, warmup):
    n = w.n
    out = ctx.malloc(24 * n)
    walls, events = [], {}
    try:
        ctx.profile(True)
        for it in range(warmup + reps):
            ctx.profile_reset()
            t0 = time.perf_counter()
            w.permutation(out)
            t1 = time.perf_counter()
            if it < warmup:
                continue
            walls.append((t1 - t0) * 1e3)
            for name, (ms, cnt) in ctx.profile_stats().items():
                if name.startswith("wires_perm_") or name == "plonk_wires_permutation":
                    assert cnt == 1, (name, cnt)
                    events.setdefault(name, []).append(ms)
        ctx.profile(False)
        ctx.profile_reset()
        equal = bool(np.array_equal(np.frombuffer(out.to_host(), np.int64), want))
    finally:
        out.free()
    passes = sum(1 for k in events if k.startswith("wires_perm_hist_"))
    moved = stage_bytes(3 * n, passes)
    stages = {}
    for name, xs in sorted(events.items()):
        key = name[len("wires_perm_"):] if name.startswith("wires_perm_") else "call"
        stages[key] = {"event_ms": _stats(xs)}
        if key in moved:
            stages[key]["bytes"] = moved[key]
            stages[key]["gb_per_s"] = moved[key] / (statistics.median(xs) * 1e-3) / 1e9
    return {"passes": passes, "wall_ms": _stats(walls), "stages": stages, "equals_numpy": equal,
            "workspace_bytes": 4 * 12 * n + 4 * DIGITS * ((3 * n + TILE - 1) // TILE)}


def run_case(gm, ctx, curve, n, nb_wires, reps, warmup):
    rng = np.random.default_rng(n + nb_wires)
    t = rng.integers(0, nb_wires, size=(3, n), dtype=np.uint32)
    t[:, n - n // 8:] = 0
    lro = t.reshape(-1)
    host = []
    for _ in range(3):
        t0 = time.perf_counter()
        want = perm_numpy(lro)
        host.append((time.perf_counter() - t0) * 1e3)
    out = {"curve": curve, "n": n, "nb_wires": nb_wires, "reps": reps, "warmup": warmup,
           "numpy_host_construction_ms": dict(_stats(host), note="a stable argsort in numpy, not gnark's loop")}
    w = gm.PlonkWires(ctx, n, nb_wires, *t)
    try:
        out["permutation"] = measure_permutation(gm, ctx, w, want, reps, warmup)
        rec = {"sigma_wires": [], "sigma_host": []}
        ev = []
        same = True
        for it in range(warmup + reps):
            ctx.profile(True)
            ctx.profile_reset()
            t0 = time.perf_counter()
            a = ctx.plonk_sigma_wires(curve, w)
            t1 = time.perf_counter()
            ms, cnt = ctx.profile_stats()["plonk_sigma_wires"]
            ctx.profile(False)
            ctx.profile_reset()
            t2 = time.perf_counter()
            b = ctx.plonk_sigma(curve, n, want)
            t3 = time.perf_counter()
            if it == 0:
                same = all(x.to_host() == y.to_host() for x, y in zip(a, b))
            for x in a + b:
                x.free()
            if it >= warmup:
                rec["sigma_wires"].append((t1 - t0) * 1e3)
                rec["sigma_host"].append((t3 - t2) * 1e3)
                ev.append(ms)
        out["sigma_wires"] = {"wall_ms": _stats(rec["sigma_wires"]), "event_ms": _stats(ev)}
        out["sigma_host"] = {"wall_ms": _stats(rec["sigma_host"]), "host_bytes_in": 24 * n,
                             "note": "range check, pageable upload and kernel; the permutation's construction excluded"}
        out["sigma_wires_equals_sigma_host"] = same
    finally:
        w.free()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--cases", default="bls12377:%d,bn254:%d" % (1 << 22, 1 << 20))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "plonk_wires_perm_timing.json"))
    a = ap.parse_args()
    if a.reps < 3:
        ap.error("medians of at least three runs")
    import gnark_mi355x as gm
    results = []
    with gm.Context(0) as ctx:
        for case in a.cases.split(","):
            curve, n = case.split(":")
            for nb_wires in (int(n), int(n) // 2):
                r = run_case(gm, ctx, curve, int(n), nb_wires, a.reps, a.warmup)
                results.append(r)
                print(json.dumps(r), flush=True)
                ctx.trim()
    doc = {"tool": "tools/plonk_wires_perm_timing.py",
           "timing": "stages by device events (profiling scopes), calls by the host wall clock of synchronous calls; "
                     "one process, the two sigma entries alternating after the warm-up",
           "not_measured": "gnark's buildPermutation on the CPU (no Go toolchain): no ratio against it is claimed",
           "results": results}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(doc, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
