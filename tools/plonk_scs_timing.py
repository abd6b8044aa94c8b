#!/usr/bin/env python3
"""Times the PLONK circuit resident on the device (gm_plonk_scs_*,
gm_plonk_pk_setup_scs) beside the path before it (not part of bench.py, not a
test).

  python tools/plonk_scs_timing.py [--reps 5] [--warmup 1] [--out profiles/plonk_scs_timing.json]
                                   [--cases bls12377:4194304,bn254:1048576]

Per case, in one process, medians of `reps` runs with min-max after `warmup`
runs, on a squaring-chain-like circuit (x_(k+1) = x_k^2 + c_k: l = r = x_k,
o = x_(k+1), qm = 1, qo = -1, qk = c_k from a CoeffTable of 1000 entries; two
public inputs; two BSB22 gates of 64 committed constraints each):
  (1) setup      gm_plonk_pk_setup_scs against gm_plonk_pk_setup_wires fed the same
                 selectors as dense vectors in pageable host memory and the same
                 tables uploaded beforehand; host wall clock, the two alternating.
                 The sibling is existing code: it is the yardstick.  Digests must
                 be equal.
  (2) kernels    the selector kernel (a coefficient column and a qcp column) and
                 the split kernel by device events, with the bytes they move by
                 this tool's own count (4 + 32 + 32 per row for a selector) and
                 the share of the 8 TB/s HBM figure
  (3) check      gm_plonk_scs_check: the whole entry by the host wall clock (with
                 the upload of the witness) and its kernel by device events
                 (without).  The witness is random, so every constraint fails:
                 the atomics' worst case.
  (4) bytes      host bytes crossing PCIe per setup, both ways, by the entries'
                 definitions
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

NB_PUBLIC, NB_BSB, NCOEFFS, COMMITTED = 2, 2, 1000, 64
HBM_BYTES_PER_S = 8e12


def _stats(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs), "spread": max(xs) - min(xs)}


def chain_records(n):
    """XA XB XC QL QR QO QM QC Commitment per constraint; wire k is x_k."""
    nc = n - NB_PUBLIC
    rng = np.random.default_rng(n)
    rec = np.zeros((nc, 9), np.uint32)
    k = np.arange(nc, dtype=np.uint32)
    rec[:, 0], rec[:, 1], rec[:, 2] = k, k, k + 1
    rec[:, 5], rec[:, 6] = 3, 1                      # qo = -1, qm = 1
    rec[:, 7] = rng.integers(5, NCOEFFS, size=nc)    # qk = c_k
    committed = [np.sort(rng.choice(nc, size=COMMITTED, replace=False)).astype(np.uint32) for _ in range(NB_BSB)]
    index = [int(nc // 3), int(2 * nc // 3)]
    for rows in committed:
        rec[rows, 8] = 1
    rec[index, 8] = 2
    return rec, committed, index


def events(ctx, name):
    ms, cnt = ctx.profile_stats()[name]
    assert cnt == 1, (name, cnt)
    return ms


def run_case(gm, ctx, curve, n, reps, warmup):
    nc, nb_wires = n - NB_PUBLIC, n
    pb = gm.point_bytes(curve, False)
    rec, committed, index = chain_records(n)
    co = ctx.random_scalars(curve, NCOEFFS, 11)
    coeffs = bytearray(co.to_host())
    co.free()
    k = ctx.random_scalars(curve, n + 3, 231)
    can_dev = ctx.batch_mul_base(curve, False, gm.generator(curve), k, n + 3)
    k.free()
    can = can_dev.to_host()
    can_dev.free()
    out = {"curve": curve, "n": n, "nb_public": NB_PUBLIC, "nb_constraints": nc, "nb_wires": nb_wires,
           "ncoeffs": NCOEFFS, "nb_bsb": NB_BSB, "reps": reps, "warmup": warmup}

    # (2) the split kernel: one upload per repetition
    split = []
    ctx.profile(True)
    circ = None
    for it in range(warmup + reps):
        if circ is not None:
            circ.free()
        ctx.profile_reset()
        circ = gm.PlonkCircuit(ctx, curve, n, NB_PUBLIC, nb_wires, rec, bytes(coeffs), committed, index)
        if it >= warmup:
            split.append(events(ctx, "plonk_scs_split"))
    moved = 36 * nc + 12 * n + 21 * nc
    out["split_kernel"] = {"event_ms": _stats(split), "bytes": moved,
                           "gb_per_s": moved / (statistics.median(split) * 1e-3) / 1e9,
                           "share_of_hbm": moved / (statistics.median(split) * 1e-3) / HBM_BYTES_PER_S}
    out["resident_bytes"] = circ.resident_bytes()
    # (2) the selector kernel
    buf = ctx.malloc(32 * n)
    for label, which in (("selector_qk", gm.SCS_QK), ("selector_qcp0", gm.SCS_QCP0)):
        ev = []
        for it in range(warmup + reps):
            ctx.profile_reset()
            circ.selector(which, buf)
            if it >= warmup:
                ev.append(events(ctx, "plonk_scs_selector"))
        moved = (4 + 32 + 32) * n if which == gm.SCS_QK else 32 * n
        out[label] = {"event_ms": _stats(ev), "bytes": moved, "gb_per_s": moved / (statistics.median(ev) * 1e-3) / 1e9,
                      "share_of_hbm": moved / (statistics.median(ev) * 1e-3) / HBM_BYTES_PER_S,
                      "bytes_note": "4 + 32 + 32 per row" if which == gm.SCS_QK else
                                    "32 per row written; the search reads a list of %d rows" % COMMITTED}
    # (3) the check
    w = ctx.random_scalars(curve, nb_wires, 13)
    wit = w.to_host()
    w.free()
    wall, ev, count = [], [], None
    for it in range(warmup + reps):
        ctx.profile_reset()
        t0 = time.perf_counter()
        count, first = circ.check(wit)
        t1 = time.perf_counter()
        if it >= warmup:
            wall.append((t1 - t0) * 1e3)
            ev.append(events(ctx, "plonk_scs_check"))
    ctx.profile(False)
    ctx.profile_reset()
    out["check"] = {"wall_ms_with_upload": _stats(wall), "kernel_event_ms": _stats(ev), "witness_bytes": 32 * nb_wires,
                    "unsatisfied": count, "first": first, "checked": int((rec[:, 8] == 0).sum())}

    # (1) setup: the dense selectors the sibling is fed, made once
    sel = {}
    for name, which in zip(gm.PLONK_SETUP_POLYS, range(5)):
        sel[name] = np.frombuffer(circ.selector(which, buf).to_host(), np.uint8).copy()
    qcp = [np.frombuffer(circ.selector(gm.SCS_QCP0 + j, buf).to_host(), np.uint8).copy() for j in range(NB_BSB)]
    buf.free()
    t = np.zeros((3, n), np.uint32)
    t[0, :NB_PUBLIC] = np.arange(NB_PUBLIC)
    t[:, NB_PUBLIC:] = rec[:, :3].T
    wires = gm.PlonkWires(ctx, n, nb_wires, *t)
    rows = [NB_PUBLIC + i for i in index]
    walls = {"scs": [], "wires": []}
    same = True
    for it in range(warmup + reps):
        t0 = time.perf_counter()
        key, d_scs, _ = gm.PlonkProvingKey.setup_from_circuit(circ, can, lagrange=True)
        t1 = time.perf_counter()
        sizes = key.resident_bytes()
        key.free()
        t2 = time.perf_counter()
        key, d_wires, _ = gm.PlonkProvingKey.setup_from_wires(ctx, curve, n, NB_PUBLIC, sel, wires, qcp, rows, can,
                                                              lagrange=True)
        t3 = time.perf_counter()
        assert key.resident_bytes() == sizes
        key.free()
        same = same and d_scs == d_wires
        if it >= warmup:
            walls["scs"].append((t1 - t0) * 1e3)
            walls["wires"].append((t3 - t2) * 1e3)
    wires.free()
    circ.free()
    a, b = _stats(walls["scs"]), _stats(walls["wires"])
    out["setup"] = {"scs_wall_ms": a, "wires_wall_ms": b, "digests_equal": same,
                    "scs_minus_wires_ms": a["median"] - b["median"],
                    "beyond_siblings_spread": abs(a["median"] - b["median"]) > b["spread"]}
    # (4) host bytes across PCIe per setup
    srs_in, back = pb * (n + 3) + pb * n, pb * (8 + NB_BSB) + pb * n
    out["pcie_bytes"] = {
        "wires": {"in_selectors": (5 + NB_BSB) * 32 * n, "in_tables_once": 12 * n, "in_srs": srs_in, "out": back},
        "scs": {"in_circuit_once": 36 * nc + 32 * NCOEFFS + 4 * COMMITTED * NB_BSB, "in_srs": srs_in, "out": back},
        "note": "in_srs: the canonical points for the key and the first n again for the EC-FFT, as both entries do",
    }
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--cases", default="bls12377:%d,bn254:%d" % (1 << 22, 1 << 20))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "plonk_scs_timing.json"))
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
    doc = {"tool": "tools/plonk_scs_timing.py",
           "timing": "kernels by device events (profiling scopes), calls by the host wall clock of synchronous "
                     "calls; one process, the two setup entries alternating after the warm-up",
           "results": results}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(doc, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
