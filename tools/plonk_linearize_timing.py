#!/usr/bin/env python3
"""Times the PLONK linearized polynomial on resident buffers, and the device share
of the prover's last round with and without it (not part of bench.py).

  python tools/plonk_linearize_timing.py [--reps 3] [--warmup 1] [--out profiles/plonk_linearize_timing.json]
                                         [--cases bls12377:4194304,bn254:1048576]

Per case (BLS12-377 n = 2^22, BN254 n = 2^20, nb_bsb = 0), in one process, the
legs alternating after a warm-up:
  (a) resident_round   gm_plonk_linearize with all four blinded outputs (device-event
                       bracket of the whole call, profile scope plonk_linearize_call,
                       its kernels beside it, and the host wall clock), then
                       gm_msm_prepared of lin, gm_kzg_open of z_blinded at w zeta,
                       gm_kzg_eval and gm_kzg_batch_open over [lin, l~, r~, o~, s1, s2],
                       all on the buffers where they lie.
  (b) host_lin_round   what the device does for the round without the call, as the Go
                       hook issues it: the three h shards downloaded (gm_memcpy_d2h
                       into one touched buffer), gm_kzg_commit of a host linearized
                       polynomial (uploads it), gm_copy_to_device and gm_kzg_open of a
                       host Z~, six gm_copy_to_device, gm_kzg_eval, gm_kzg_batch_open
                       and the frees.  The host's own combination and evaluations are
                       left out, so (b) is a lower bound on the old stage.  Its parts
                       are timed by host wall clock as well.
The digest, the claimed values and both opening proofs of the two legs must be
equal.  The combination kernel is set against two bounds:
  HBM      (12 + nb_bsb) x 32 B per coefficient at 8 TB/s; as written the kernel
           moves (11 + nb_bsb) x 32 B (z, s3, qm, ql, qr, qo, qk, three h shards in,
           lin out)
  Fr mul   (9 + nb_bsb) products per coefficient at the 150 Gmul/s the radix-2^29
           product reaches (field.hpp)
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
sys.path.insert(0, os.path.join(ROOT, "oracle"))

HBM_BYTES_PER_S = 8e12
FR_MUL_PER_S = 150e9
STREAMS = 12
STREAMS_AS_WRITTEN = 11
MULS = 9
KERNELS = ("plonk_lin_combine", "plonk_lin_blind")


def _scopes(ctx):
    """{scope: (total ms, count)} since the last reset."""
    ctx.synchronize()
    st = ctx.profile_stats()
    ctx.profile_reset()
    return st


def _stats(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs)}


def run_case(gm, ctx, curve, n, reps, warmup):
    import pyref
    c = pyref.CURVES[curve]
    m = n + 2
    polys = {k: ctx.random_scalars(curve, n, 81 + i) for i, k in enumerate(gm.PLONK_POLYS)}
    h = ctx.random_scalars(curve, 4 * n, 95)
    small = ctx.random_scalars(curve, 14, 96).to_host()
    el = lambda i, k=1: small[32 * i:32 * (i + k)]
    blinds = {"bl": el(0, 2), "br": el(2, 2), "bo": el(4, 2), "bz": el(6, 3)}
    alpha, beta, gamma, zeta, fold = el(9), el(10), el(11), el(12), el(13)
    wzeta = pyref.encode_fr(c, pyref.domain_generator(c, n) * pyref.decode_fr(c, zeta) % c.r)
    lin = ctx.malloc(32 * (n + 3))
    out = {k: ctx.malloc(32 * (n + (3 if k == "z_blinded" else 2))) for k in gm.PLONK_LIN_BLINDED}
    k = ctx.random_scalars(curve, n + 3, 97)
    pts = ctx.batch_mul_base(curve, False, gm.generator(curve), k, n + 3)
    srs = ctx.points_upload(curve, pts.to_host())
    pts.free()
    k.free()
    lens = [n + 3, n + 2, n + 2, n + 2, n, n]
    host = {}
    got = {"a": {}, "b": {}}

    def resident():
        return [lin, out["l_blinded"], out["r_blinded"], out["o_blinded"], polys["s1"], polys["s2"]]

    def leg_a_lin():
        got["a"]["evals"] = ctx.plonk_linearize(curve, n, polys, [], [], blinds, h, alpha, beta, gamma, zeta, lin,
                                                blinded=out)

    def leg_a_rest():
        r = got["a"]
        t = [time.perf_counter()]
        r["digest"] = ctx.msm_prepared(curve, lin, srs, n + 3)[1]
        t.append(time.perf_counter())
        r["z_open"] = ctx.kzg_open(curve, srs, out["z_blinded"], wzeta, n + 3)
        t.append(time.perf_counter())
        r["values"] = ctx.kzg_eval(curve, resident(), zeta, lens)
        r["batch"] = ctx.kzg_batch_open(curve, srs, resident(), zeta, fold, lens)
        t.append(time.perf_counter())
        return t

    shard = np.ones(32 * m, np.uint8)  # touched: the downloads land in mapped pages
    L = gm.load_library()

    def leg_b():
        """Returns the wall-clock marks between its parts."""
        r = got["b"]
        t = [time.perf_counter()]
        for s in range(3):  # the host needs h1, h2, h3 to build the polynomial
            gm._check(L.gm_memcpy_d2h(ctx.handle, gm._p(shard), h.ptr + 32 * m * s, 32 * m))
        t.append(time.perf_counter())
        r["digest"] = ctx.kzg_commit(curve, srs, host["lin"])
        t.append(time.perf_counter())
        zb = ctx.copy_to_device(host["z_blinded"])
        r["z_open"] = ctx.kzg_open(curve, srs, zb, wzeta, n + 3)
        zb.free()
        t.append(time.perf_counter())
        up = [ctx.copy_to_device(host[k]) for k in ("lin", "l_blinded", "r_blinded", "o_blinded", "s1", "s2")]
        t.append(time.perf_counter())
        r["values"] = ctx.kzg_eval(curve, up, zeta, lens)
        r["batch"] = ctx.kzg_batch_open(curve, srs, up, zeta, fold, lens)
        t.append(time.perf_counter())
        for b in up:
            b.free()
        t.append(time.perf_counter())
        return t

    rec = {"call_event_ms": [], "call_wall_ms": [], "rest_wall_ms": [], "resident_round_wall_ms": [],
           "host_lin_round_wall_ms": []}
    kern, parts, aparts = [], [], []
    try:
        for it in range(warmup + reps):
            ctx.profile_reset()
            t0 = time.perf_counter()
            leg_a_lin()
            t1 = time.perf_counter()
            st = _scopes(ctx)
            t2 = time.perf_counter()
            amarks = leg_a_rest()
            t3 = time.perf_counter()
            if not host:
                grab = lambda b, elems: np.frombuffer(b.to_host(32 * elems), np.uint8).copy()
                host.update(lin=grab(lin, n + 3), s1=grab(polys["s1"], n), s2=grab(polys["s2"], n))
                host.update({k: grab(out[k], n + (3 if k == "z_blinded" else 2)) for k in gm.PLONK_LIN_BLINDED})
            ctx.profile_reset()
            marks = leg_b()
            t4, t5 = marks[0], marks[-1]
            ctx.profile_reset()
            if it >= warmup:
                rec["call_event_ms"].append(st["plonk_linearize_call"][0])
                rec["call_wall_ms"].append((t1 - t0) * 1e3)
                rec["rest_wall_ms"].append((t3 - t2) * 1e3)
                rec["resident_round_wall_ms"].append((t1 - t0 + t3 - t2) * 1e3)
                rec["host_lin_round_wall_ms"].append((t5 - t4) * 1e3)
                parts.append([(y - x) * 1e3 for x, y in zip(marks, marks[1:])])
                aparts.append([(y - x) * 1e3 for x, y in zip(amarks, amarks[1:])])
                kern.append({s: v[0] for s, v in st.items()})
        a, b = got["a"], got["b"]
        same = {"digest": a["digest"] == b["digest"], "z_opening": a["z_open"] == b["z_open"],
                "claimed_values": a["values"] == b["values"], "batch_opening": a["batch"] == b["batch"],
                "z_claimed_is_evals_5": a["z_open"][0] == a["evals"][5],
                "claimed_are_evals": a["values"][1:] == a["evals"][:5]}
    finally:
        for buf in list(polys.values()) + list(out.values()) + [h, lin, srs]:
            buf.free()
    res = {"curve": curve, "n": n, "nb_bsb": 0, "reps": reps, "warmup": warmup, "legs_equal": same}
    res["linearize_resident"] = {"event_ms": _stats(rec["call_event_ms"]), "wall_ms": _stats(rec["call_wall_ms"])}
    res["resident_round"] = {"wall_ms": _stats(rec["resident_round_wall_ms"]),
                             "commit_and_openings_wall_ms": _stats(rec["rest_wall_ms"]),
                             "parts_wall_ms": {name: statistics.median(p[i] for p in aparts) for i, name in enumerate(
                                 ("commit_of_resident_lin", "open_resident_z", "eval_and_batch_open"))}}
    res["host_lin_round"] = {"wall_ms": _stats(rec["host_lin_round_wall_ms"]),
                             "parts_wall_ms": {name: statistics.median(p[i] for p in parts) for i, name in enumerate(
                                 ("h_shards_d2h", "commit_of_host_lin", "upload_and_open_z", "six_uploads",
                                  "eval_and_batch_open", "six_frees"))}}
    ra, rb = res["resident_round"]["wall_ms"]["median"], res["host_lin_round"]["wall_ms"]["median"]
    res["resident_over_host_lin_round"] = ra / rb
    res["resident_round_is_shorter"] = ra < rb
    res["scope_ms_per_call"] = {s: statistics.median(c[s] for c in kern) for s in kern[0]}
    sc = res["scope_ms_per_call"]
    k_ms = sc["plonk_lin_combine"]
    t_hbm = STREAMS * 32 * n / HBM_BYTES_PER_S * 1e3
    t_hbm_w = STREAMS_AS_WRITTEN * 32 * n / HBM_BYTES_PER_S * 1e3
    t_mul = MULS * n / FR_MUL_PER_S * 1e3
    res["kernels"] = {
        "ms_per_call": {s: sc[s] for s in KERNELS},
        "evaluations_ms_per_call": sc.get("kzg_chunk_eval", 0) + sc.get("kzg_chunk_carry", 0),
        "combine_bytes_per_s_as_written": STREAMS_AS_WRITTEN * 32 * n / (k_ms * 1e-3),
        "combine_fr_mul_per_s": MULS * n / (k_ms * 1e-3),
        "blind_bytes_per_s": 8 * 32 * n / (sc["plonk_lin_blind"] * 1e-3),
        "hbm_bound_ms": t_hbm, "hbm_as_written_ms": t_hbm_w, "fr_mul_bound_ms": t_mul,
        "bound": "fr_mul_issue" if t_mul > t_hbm else "hbm",
        "frac_of_bound": max(t_hbm, t_mul) / k_ms,
    }
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--cases", default="bls12377:%d,bn254:%d" % (1 << 22, 1 << 20))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "plonk_linearize_timing.json"))
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
    doc = {"tool": "tools/plonk_linearize_timing.py",
           "timing": "leg (a): device events on the context stream (profile scopes) and host wall clock; "
                     "leg (b), the commit and the openings: host wall clock of the synchronous calls",
           "not_measured": "the host's own evaluations and combination in the replaced stage, and the Go "
                           "seam's linearize method (no Go toolchain)",
           "results": results}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(doc, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
