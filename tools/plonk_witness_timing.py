#!/usr/bin/env python3
"""Times a PLONK session that starts from the witness (gm_plonk_wires_upload,
gm_plonk_session_round1_witness, gm_plonk_session_bsb22_sparse) against the same
session from host-gathered l, r, o (not part of bench.py, not a test).

  python tools/plonk_witness_timing.py [--reps 5] [--warmup 1] [--out profiles/plonk_witness_timing.json]
                                       [--cases bls12377:4194304,bn254:1048576]

Per case (BLS12-377 n = 2^22, BN254 n = 2^20, two public inputs, h_rand given)
and per nb_wires in (n, n / 2), in one process, the challenges fixed, the legs
alternating after a warm-up round, every time but (c) the host wall clock of
synchronous calls:
  (a) witness    begin, round1_witness, rounds 2 to 5 and free on a default key
                 (nb_bsb = 0), each timed: 32 nb_wires bytes cross PCIe in round 1
  (b) host_lro   the same with round1 from l, r, o gathered on the host by numpy
                 OUTSIDE the timed part (96 n bytes cross): the path before the wire
                 tables, without the serial gather gnark's solver pays for it, so
                 (b) - (a) is a lower bound on the gain
  (c) gather     gm_plonk_gather_lro alone on resident buffers, by device events
                 (profiling scope plonk_gather_lro_call), in repetitions of its own
  (d) bsb22      begin, bsb22, free on a second key with nb_bsb = 1 (no coset
                 cache: bsb22 does not read it): the dense call with the n-element
                 vector against the sparse call with its 64 + 2 nonzero rows (64
                 committed wires and the two blinding rows of prove.go:300-311)
Every output of legs (a) and (b) must be equal, and so must the two digests of (d).

Acceptance (written into the JSON, not enforced): at nb_wires = n, round 1 of (a) is
shorter than round 1 of (b) by more than the two min-max spreads together, and so is
the whole proof.  Not measured: the Go seam (no Go toolchain), and the host gather
that leg (b) does not pay.
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
COMMITTED = 64
ROUNDS = ("begin", "round1", "round2", "round3", "round4", "round5", "free")
BSB = ("begin", "bsb22", "free")


def _stats(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs), "spread": max(xs) - min(xs)}


def _host(ctx, curve, k, seed):
    b = ctx.random_scalars(curve, k, seed)
    try:
        return b.to_host()
    finally:
        b.free()


def _tables(n, nb_wires, seed):
    """Random rows in evaluateLROSmallDomain's convention: (i, 0, 0) for the public
    inputs, (0, 0, 0) padding at the end."""
    t = np.random.default_rng(seed).integers(0, nb_wires, size=(3, n), dtype=np.uint32)
    t[0, :NB_PUBLIC] = np.arange(NB_PUBLIC)
    t[1:, :NB_PUBLIC] = 0
    t[:, n - 3:] = 0
    return t


def run_case(gm, ctx, curve, n, reps, warmup):
    host = lambda seed, k=n: np.frombuffer(_host(ctx, curve, k, seed), np.uint8)
    fixed = {k: host(101 + i) for i, k in enumerate(gm.PLONK_PK_POLYS)}
    small = _host(ctx, curve, 16, 120)
    el = lambda i, k=1: small[32 * i:32 * (i + k)]
    blinds = {"bl": el(0, 2), "br": el(2, 2), "bo": el(4, 2), "bz": el(6, 3)}
    h_rand = el(9, 2)
    beta, gamma, alpha, zeta, fold = el(11), el(12), el(13), el(14), el(15)
    srs_host = []
    for seed, cnt in ((131, n + 3), (132, n)):
        k = ctx.random_scalars(curve, cnt, seed)
        pts = ctx.batch_mul_base(curve, False, gm.generator(curve), k, cnt)
        srs_host.append(pts.to_host())
        pts.free()
        k.free()
    key = gm.PlonkProvingKey(ctx, curve, n, NB_PUBLIC, fixed, [], [], srs_host[0], srs_host[1])
    key1 = gm.PlonkProvingKey(ctx, curve, n, NB_PUBLIC, fixed, [host(140)], [NB_PUBLIC + 1], srs_host[0],
                              srs_host[1], cache=False)
    got = {}

    def proof(name, round1):
        r = got[name] = {}
        t = [time.perf_counter()]
        s = key.session()
        t.append(time.perf_counter())
        try:
            r["lro"] = round1(s)
            t.append(time.perf_counter())
            r["z"] = s.round2(beta, gamma)
            t.append(time.perf_counter())
            r["h"] = s.round3(alpha)
            t.append(time.perf_counter())
            r["lin"], r["claimed"], r["z_shifted"], r["z_open"] = s.round4(zeta)
            t.append(time.perf_counter())
            r["batch"] = s.round5(fold)
            t.append(time.perf_counter())
        finally:
            s.free()
        t.append(time.perf_counter())
        return t

    def bsb(name, call):
        t = [time.perf_counter()]
        s = key1.session()
        t.append(time.perf_counter())
        try:
            got[name] = call(s)
            t.append(time.perf_counter())
        finally:
            s.free()
        t.append(time.perf_counter())
        return t

    # (d): 64 committed rows and the two blinding rows, unsorted, somewhere behind the public inputs
    rows = np.random.default_rng(7).choice(np.arange(NB_PUBLIC, n), COMMITTED + 2, replace=False).astype(np.uint32)
    vals = host(141, COMMITTED + 2)
    dense = np.zeros((n, 32), np.uint8)
    dense[rows] = vals.reshape(-1, 32)
    dense = dense.reshape(-1)

    out = {"curve": curve, "n": n, "nb_public": NB_PUBLIC, "reps": reps, "warmup": warmup,
           "key_bytes": key.resident_bytes()[0], "by_nb_wires": []}
    try:
        rec = {"dense": [], "sparse": []}
        for it in range(warmup + reps):
            marks = {"dense": bsb("dense", lambda s: s.bsb22(0, dense)),
                     "sparse": bsb("sparse", lambda s: s.bsb22_sparse(0, rows, vals))}
            if it >= warmup:
                for k, t in marks.items():
                    rec[k].append([(y - x) * 1e3 for x, y in zip(t, t[1:])])
        out["bsb22"] = {"nb_bsb": 1, "rows": COMMITTED + 2, "digests_equal": got["dense"] == got["sparse"],
                        "host_bytes": {"dense": 32 * n, "sparse": 36 * (COMMITTED + 2)}}
        for leg in rec:
            out["bsb22"][leg] = {"total_wall_ms": _stats([sum(p) for p in rec[leg]]),
                                 "parts_wall_ms": {nm: _stats([p[i] for p in rec[leg]]) for i, nm in enumerate(BSB)}}

        for nb_wires in (n, n // 2):
            t = _tables(n, nb_wires, 150 + nb_wires % 7)
            witness = host(160, nb_wires)
            W = witness.reshape(nb_wires, 32)
            lro = [np.ascontiguousarray(W[t[k]]).reshape(-1) for k in range(3)]  # leg (b)'s host gather, untimed
            public = witness[:32 * NB_PUBLIC]
            wires = gm.PlonkWires(ctx, n, nb_wires, *t)
            legs = {"witness": lambda s: s.round1_witness(wires, witness, blinds, h_rand=h_rand),
                    "host_lro": lambda s: s.round1(lro[0], lro[1], lro[2], public, blinds, h_rand=h_rand)}
            rec = {k: [] for k in legs}
            try:
                for it in range(warmup + reps):
                    marks = {k: proof(k, f) for k, f in legs.items()}
                    if it >= warmup:
                        for k, tt in marks.items():
                            rec[k].append([(y - x) * 1e3 for x, y in zip(tt, tt[1:])])
                # (c): the gather alone, by device events
                wit_dev = ctx.copy_to_device(witness)
                bufs = [ctx.malloc(32 * n) for _ in range(3)]
                ev = []
                ctx.profile(True)
                for it in range(warmup + reps):
                    ctx.profile_reset()
                    wires.gather(wit_dev, *bufs)
                    ms, cnt = ctx.profile_stats()["plonk_gather_lro_call"]
                    assert cnt == 1
                    if it >= warmup:
                        ev.append(ms)
                ctx.profile(False)
                ctx.profile_reset()
                gathered = all(bufs[k].to_host() == lro[k].tobytes() for k in range(3))
                for b in bufs + [wit_dev]:
                    b.free()
            finally:
                wires.free()
            res = {"nb_wires": nb_wires, "wires_bytes": 12 * n,
                   "round1_host_bytes": {"witness": 32 * nb_wires, "host_lro": 32 * (3 * n + NB_PUBLIC)},
                   "legs_equal": got["witness"] == got["host_lro"], "gather_equals_numpy": gathered,
                   "gather_event_ms": _stats(ev),
                   "gather_traffic_bytes": 12 * n + 96 * n + 96 * n}
            for leg in legs:
                res[leg] = {"total_wall_ms": _stats([sum(p) for p in rec[leg]]),
                            "parts_wall_ms": {nm: _stats([p[i] for p in rec[leg]]) for i, nm in enumerate(ROUNDS)}}
            ra, rb = (res[k]["parts_wall_ms"]["round1"] for k in ("witness", "host_lro"))
            ta, tb = (res[k]["total_wall_ms"] for k in ("witness", "host_lro"))
            res["gain_ms"] = {"round1": rb["median"] - ra["median"], "proof": tb["median"] - ta["median"]}
            res["acceptance"] = {
                "round1_shorter_by_more_than_the_spreads": rb["median"] - ra["median"] > ra["spread"] + rb["spread"],
                "proof_shorter_by_more_than_the_spreads": tb["median"] - ta["median"] > ta["spread"] + tb["spread"],
            }
            out["by_nb_wires"].append(res)
    finally:
        key.free()
        key1.free()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--cases", default="bls12377:%d,bn254:%d" % (1 << 22, 1 << 20))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "plonk_witness_timing.json"))
    a = ap.parse_args()
    import gnark_mi355x as gm
    results = []
    with gm.Context(0) as ctx:
        for case in a.cases.split(","):
            curve, n = case.split(":")
            r = run_case(gm, ctx, curve, int(n), a.reps, a.warmup)
            results.append(r)
            print(json.dumps(r), flush=True)
            ctx.trim()
    doc = {"tool": "tools/plonk_witness_timing.py",
           "timing": "host wall clock of synchronous calls, the gather by device events; one process, fixed "
                     "challenges, legs alternating after the warm-up",
           "not_measured": "the Go seam (no Go toolchain); the host-side gather of l, r, o that the host_lro leg "
                           "does not pay (its inputs are gathered outside the timed part)",
           "results": results}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(doc, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
