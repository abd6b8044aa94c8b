#!/usr/bin/env python3
"""Times a whole PLONK proof on a resident key (gm_plonk_session_*), with and
without the key's coset cache, against what a caller can do with the stage calls
alone (not part of bench.py).

  python tools/plonk_session_timing.py [--reps 3] [--warmup 1] [--out profiles/plonk_session_timing.json]
                                       [--cases bls12377:4194304,bn254:1048576]

Per case (BLS12-377 n = 2^22, BN254 n = 2^20, nb_bsb = 0, two public inputs,
h_rand given), in one process, the challenges fixed, the legs alternating after a
warm-up round, every time the host wall clock of synchronous calls:
  (a)  session        gm_plonk_session_begin, rounds 1 to 5 and gm_plonk_session_free on a
                      default key (coset cache), each timed; the total spans all seven, as
                      leg (b)'s spans its uploads and its frees.  From the second session
                      on a key, begin takes the buffer the session before left with it
  (a') session_nocache  the same on a GM_PLONK_PK_NO_COSET_CACHE key
  (b)  stage_calls    the same host inputs through the calls that exist without the
                      session: three gm_copy_to_device of l, r, o and one of the
                      completed Qk, gm_ntt + gm_reverse_scalars of copies of them for
                      the canonical forms, gm_msm_prepared over the Lagrange SRS for the
                      wires and Z, gm_plonk_perm_z, gm_plonk_quotient, gm_msm_prepared of
                      the three h shards, gm_plonk_linearize, gm_msm_prepared of lin,
                      gm_kzg_open, gm_kzg_eval and gm_kzg_batch_open, and the frees.  The
                      fixed polynomials and both SRSs are resident beforehand in the
                      forms the stages take, Qk is completed on the host outside the
                      timed part, and the blinding's and h_rand's share of the digests
                      (host scalar multiplications in either leg's world) is left out:
                      (b) is a lower bound on what such a caller pays.
Outputs that do not depend on the parts (b) leaves out must be equal between the
legs: the h digests' sum identity is not checked here (tests/test_plonk_session_gpu.py
does); the claimed values, z~(w zeta), the digest of lin and both opening proofs are.

The quotient alone is then measured by device events in repetitions of their own with
profiling on (scopes plonk_session_quotient_cached, plonk_session_quotient and, in leg
(b), plonk_quotient_call): "quotient_event_ms".

Acceptance (written into the JSON, not enforced): (a) is not slower than (b) by more
than (b)'s min-max spread; round 3 of (a) is shorter than round 3 of (a') by more than
the two spreads together.  Not measured: nb_bsb > 0 at these sizes, and the Go seam
(no Go toolchain).
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
ROUNDS = ("begin", "round1", "round2", "round3", "round4", "round5", "free")
B_PARTS = ("upload_lro_qk", "canonical_forms", "commit_lro", "perm_z", "commit_z", "quotient", "commit_h",
           "linearize", "commit_lin", "open_z", "eval_and_batch_open", "frees")


def _stats(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs), "spread": max(xs) - min(xs)}


def run_case(gm, ctx, curve, n, reps, warmup):
    import pyref
    c = pyref.CURVES[curve]
    m = n + 2
    host = lambda seed, k=n: np.frombuffer(_host(ctx, curve, k, seed), np.uint8)
    fixed = {k: host(101 + i) for i, k in enumerate(gm.PLONK_PK_POLYS)}
    wires = [host(111 + i) for i in range(3)]
    small = _host(ctx, curve, 18 + NB_PUBLIC, 120)
    el = lambda i, k=1: small[32 * i:32 * (i + k)]
    blinds = {"bl": el(0, 2), "br": el(2, 2), "bo": el(4, 2), "bz": el(6, 3)}
    h_rand, public = el(9, 2), el(18, NB_PUBLIC)
    beta, gamma, alpha, zeta, fold = el(11), el(12), el(13), el(14), el(15)
    wzeta = pyref.encode_fr(c, pyref.domain_generator(c, n) * pyref.decode_fr(c, zeta) % c.r)
    srs_host = []
    for seed, cnt in ((131, n + 3), (132, n)):
        k = ctx.random_scalars(curve, cnt, seed)
        pts = ctx.batch_mul_base(curve, False, gm.generator(curve), k, cnt)
        srs_host.append(pts.to_host())
        pts.free()
        k.free()
    keys = {name: gm.PlonkProvingKey(ctx, curve, n, NB_PUBLIC, fixed, [], [], srs_host[0], srs_host[1], cache=on)
            for name, on in (("session", True), ("session_nocache", False))}
    key_bytes = {name: k.resident_bytes() for name, k in keys.items()}

    # ---- leg (b)'s resident state: what a caller of the stage calls keeps per key
    srs_can, srs_lag = ctx.points_upload(curve, srs_host[0]), ctx.points_upload(curve, srs_host[1])

    def canonical_of(lag_buf):
        out = ctx.malloc(32 * n)
        out.copy_from(lag_buf, 32 * n)
        ctx.ntt(curve, out, n, True, False, False)
        ctx.reverse_scalars(curve, out, n)
        return out

    kept = {}
    for k in gm.PLONK_PK_POLYS:
        if k == "qk":
            continue
        lag = ctx.copy_to_device(fixed[k])
        kept[k] = canonical_of(lag)
        if k in ("s1", "s2", "s3"):
            kept[k + "_lag"] = lag
        else:
            lag.free()
    qk_done = fixed["qk"].copy()
    qk_done[:32 * NB_PUBLIC] = np.frombuffer(public, np.uint8)
    view = lambda b, off, elems: gm.DeviceBuffer(ctx, b.ptr + 32 * off, 32 * elems)
    got = {}

    def leg_session(name):
        r = got[name] = {}
        t = [time.perf_counter()]
        s = keys[name].session()
        t.append(time.perf_counter())
        try:
            r["lro"] = s.round1(wires[0], wires[1], wires[2], public, blinds, h_rand=h_rand)
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

    def leg_b():
        r = got["stage_calls"] = {}
        t = [time.perf_counter()]
        lag = [ctx.copy_to_device(w) for w in wires]
        qk_lag = ctx.copy_to_device(qk_done)
        t.append(time.perf_counter())
        can = [canonical_of(b) for b in lag]
        qk = canonical_of(qk_lag)
        t.append(time.perf_counter())
        r["lro_unblinded"] = [ctx.msm_prepared(curve, b, srs_lag, n)[1] for b in lag]
        t.append(time.perf_counter())
        zl, zc, h = ctx.malloc(32 * n), ctx.malloc(32 * n), ctx.malloc(32 * 4 * n)
        perm = {"l": lag[0], "r": lag[1], "o": lag[2], "s1": kept["s1_lag"], "s2": kept["s2_lag"],
                "s3": kept["s3_lag"]}
        ctx.plonk_perm_z(curve, n, perm, beta, gamma, zl, zc)
        t.append(time.perf_counter())
        r["z_unblinded"] = ctx.msm_prepared(curve, zl, srs_lag, n)[1]
        t.append(time.perf_counter())
        q = dict({k: kept[k] for k in gm.PLONK_PK_POLYS if k != "qk"}, qk=qk, l=can[0], r=can[1], o=can[2], z=zc)
        ctx.plonk_quotient(curve, n, q, [], [], blinds, alpha, beta, gamma, h)
        t.append(time.perf_counter())
        r["h_unedited"] = [ctx.msm_prepared(curve, view(h, m * s, m), srs_can, m)[1] for s in range(3)]
        t.append(time.perf_counter())
        lin = ctx.malloc(32 * (n + 3))
        out = {k: ctx.malloc(32 * (n + (3 if k == "z_blinded" else 2))) for k in gm.PLONK_LIN_BLINDED}
        ev = ctx.plonk_linearize(curve, n, q, [], [], blinds, h, alpha, beta, gamma, zeta, lin, h_rand=h_rand,
                                 blinded=out)
        t.append(time.perf_counter())
        r["lin"] = ctx.msm_prepared(curve, lin, srs_can, n + 3)[1]
        t.append(time.perf_counter())
        r["z_shifted"], r["z_open"] = ctx.kzg_open(curve, srs_can, out["z_blinded"], wzeta, n + 3)
        t.append(time.perf_counter())
        polys = [lin, out["l_blinded"], out["r_blinded"], out["o_blinded"], kept["s1"], kept["s2"]]
        lens = [n + 3, n + 2, n + 2, n + 2, n, n]
        r["claimed"] = ctx.kzg_eval(curve, polys[:1], zeta, lens[:1]) + ev[:5]
        r["batch"] = ctx.kzg_batch_open(curve, srs_can, polys, zeta, fold, lens)[1]
        t.append(time.perf_counter())
        for b in lag + can + [qk_lag, qk, zl, zc, h, lin] + list(out.values()):
            b.free()
        t.append(time.perf_counter())
        return t

    rec = {"session": [], "session_nocache": [], "stage_calls": []}
    try:
        for it in range(warmup + reps):
            marks = {"session": leg_session("session"), "stage_calls": leg_b(),
                     "session_nocache": leg_session("session_nocache")}
            if it >= warmup:
                for k, t in marks.items():
                    rec[k].append([(y - x) * 1e3 for x, y in zip(t, t[1:])])
        # the quotient alone, by device events, in repetitions of their own (profiling
        # records an event pair per kernel, so it stays out of the wall-clock legs)
        quot = {"session": [], "session_nocache": [], "stage_calls": []}
        scope = {"session": "plonk_session_quotient_cached", "session_nocache": "plonk_session_quotient",
                 "stage_calls": "plonk_quotient_call"}
        ctx.profile(True)
        for it in range(reps):
            for leg, fn in (("session", lambda: leg_session("session")), ("stage_calls", leg_b),
                            ("session_nocache", lambda: leg_session("session_nocache"))):
                ctx.profile_reset()
                fn()
                ctx.synchronize()
                ms, cnt = ctx.profile_stats()[scope[leg]]
                assert cnt == 1
                quot[leg].append(ms)
        ctx.profile(False)
        ctx.profile_reset()
        a, a2, b = got["session"], got["session_nocache"], got["stage_calls"]
        shared = ("lin", "claimed", "z_shifted", "z_open", "batch")
        same = {"cache_on_equals_cache_off": a == a2,
                "session_equals_stage_calls": {k: a[k] == b[k] for k in shared}}
    finally:
        for k in keys.values():
            k.free()
        for buf in list(kept.values()) + [srs_can, srs_lag]:
            buf.free()
    res = {"curve": curve, "n": n, "nb_bsb": 0, "nb_public": NB_PUBLIC, "reps": reps, "warmup": warmup,
           "legs_equal": same, "key_bytes": {k: {"resident": v[0], "coset_cache": v[1]} for k, v in key_bytes.items()}}
    for leg, names in (("session", ROUNDS), ("session_nocache", ROUNDS), ("stage_calls", B_PARTS)):
        res[leg] = {"total_wall_ms": _stats([sum(p) for p in rec[leg]]),
                    "parts_wall_ms": {nm: _stats([p[i] for p in rec[leg]]) for i, nm in enumerate(names)}}
    ta, tb = res["session"]["total_wall_ms"], res["stage_calls"]["total_wall_ms"]
    r3a = res["session"]["parts_wall_ms"]["round3"]
    r3n = res["session_nocache"]["parts_wall_ms"]["round3"]
    qb = res["stage_calls"]["parts_wall_ms"]
    res["quotient_event_ms"] = {leg: _stats(v) for leg, v in quot.items()}
    res["round3_vs_stage_quotient_ms"] = {"session": r3a["median"], "session_nocache": r3n["median"],
                                          "stage_quotient_plus_commit_h":
                                              qb["quotient"]["median"] + qb["commit_h"]["median"],
                                          "stage_quotient_alone": qb["quotient"]["median"]}
    res["acceptance"] = {
        "session_not_slower_than_stage_calls": ta["median"] <= tb["median"] + tb["spread"],
        "cached_round3_shorter_by_more_than_the_spreads":
            r3n["median"] - r3a["median"] > r3a["spread"] + r3n["spread"],
    }
    return res


def _host(ctx, curve, k, seed):
    b = ctx.random_scalars(curve, k, seed)
    try:
        return b.to_host()
    finally:
        b.free()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--cases", default="bls12377:%d,bn254:%d" % (1 << 22, 1 << 20))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "plonk_session_timing.json"))
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
    doc = {"tool": "tools/plonk_session_timing.py",
           "timing": "host wall clock of synchronous calls; one process, fixed challenges, legs alternating "
                     "after the warm-up",
           "not_measured": "nb_bsb > 0 at these sizes; the Go seam (no Go toolchain); the host's blinding and "
                           "h_rand scalar multiplications in leg (b)",
           "results": results}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(doc, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
