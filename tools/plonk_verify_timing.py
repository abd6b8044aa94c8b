#!/usr/bin/env python3
"""Times batched PLONK and KZG verification beside gm_g16_verify_batch, in one
process (not part of bench.py, not a test).

  python tools/plonk_verify_timing.py [--reps 5] [--warmup 1] [--logm 14] [--out profiles/plonk_verify_timing.json]

Medians of `reps` runs with min and max after `warmup` runs (ms); kernel times are
HIP events around the launches (gm_profile_*).  Per curve:
  plonk    gm_plonk_verify_batch at m = 2^logm and m = 1 with nb_public in {1, 16}
           and nb_bsb in {0, 1}: wall clock, and the kernel time of the scalars
           kernel, the ladders and the assemble
  g16      gm_g16_verify_batch with sixteen public inputs at the same m, its
           ladders and assemble beside them
  kzg      gm_kzg_verify_batch and gm_kzg_verify_folded at m = 2^(logm + 2)
The entries take host arrays, so wall clock includes their upload; the kernel
times do not.  Keys and proofs are subgroup points (tiled multiples of the
generator) with random scalars, 256 distinct proofs tiled to m; each proof's first
claimed value is set to the model's constLin (tests/plonk_verify_model.py), so no
proof stops at the algebraic check and every ladder runs; the pairing equation
then fails (status 2) after the full work.
`counts` states the doublings and additions per proof from the kernels' loops
(256-step ladders, a mixed addition per set bit, a full addition per term in the
assemble), `mads` their multiply-adds (a product 2 N^2, a squaring N^2 + N (N + 1) / 2,
N limbs; a doubling is 6 products and 3 squarings, a mixed addition 8 and 2, a full
addition 12 and 2) and `mad_bound` that over the ladders' time at 30.7 T mad/s
(DESIGN.md section 3).  No CPU verifier is timed.
"""
import argparse
import json
import os
import random
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for sub_ in ("gnark-icicle_amd", "oracle", "tests", "tools"):
    sys.path.insert(0, os.path.join(ROOT, sub_))
import pyref  # noqa: E402
import pairing_constants as pcn  # noqa: E402
import plonk_verify_model as pvm  # noqa: E402
import points_check_timing as pct  # noqa: E402

CURVES = ("bn254", "bls12377", "bls12381")
MAD_RATE = 30.7e12
DISTINCT = 256


def ladder_counts(c, terms):
    """Per proof: doublings, mixed additions (expected: half the scalar's bits), full additions."""
    steps = 32 * 8
    return {"ladders": terms, "doublings": terms * steps, "mixed_additions": terms * c.r.bit_length() // 2,
            "full_additions": terms}


def mads(curve, cnt):
    n = pcn.n29(pcn.derive(curve)["c"])
    mul, sqr = 2 * n * n, n * n + n * (n + 1) // 2
    return (cnt["doublings"] * (6 * mul + 3 * sqr) + cnt["mixed_additions"] * (8 * mul + 2 * sqr)
            + cnt["full_additions"] * (12 * mul + 2 * sqr))


def tile(b, reps):
    return np.tile(np.frombuffer(b, np.uint8), reps)


def plonk_inputs(curve, n, nbp, nb, m):
    """(vk dict, the five arrays) with DISTINCT different proofs tiled to m."""
    c = pyref.CURVES[curve]
    rng = random.Random(0x71 + nbp + 100 * nb)
    rows = [nbp + 1 + 2 * j for j in range(nb)]
    vk = types.SimpleNamespace(n=n, nb_public=nbp, rows=rows)
    d = min(m, DISTINCT)
    rnd = lambda k: [rng.randrange(c.r) for _ in range(k)]
    vals, pubs, hashed, chal = [], [], [], []
    for _ in range(d):
        v, p, h, ch = rnd(7 + nb), rnd(nbp), rnd(nb), rnd(6)
        v[0] = pvm.scalars(c, vk, v, p, h, ch)[2]
        vals += v
        pubs += p
        hashed += h
        chal += ch
    pb = pct.points(curve, False, 1, 1).size
    key = pct.points(curve, False, 9 + nb, 61).reshape(9 + nb, pb)
    names = pvm.KEY_POINTS + ("kzg_g1",)
    vkd = {k: key[i].tobytes() for i, k in enumerate(names)}
    vkd.update(n=n, nb_public=nbp, qcp=pct.points(curve, False, nb, 62).tobytes() if nb else b"", commitment_row=rows,
               kzg_g2_0=pct.points(curve, True, 1, 63).tobytes(), kzg_g2_1=pct.points(curve, True, 1, 64).tobytes())
    reps = m // d
    points = np.tile(pct.points(curve, False, d * (9 + nb), 65), reps)
    return vkd, (points, tile(pvm.enc(c, vals), reps), tile(pvm.enc(c, pubs), reps) if nbp else b"",
                 tile(pvm.enc(c, hashed), reps) if nb else b"", tile(pvm.enc(c, chal), reps))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--logm", type=int, default=14)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "plonk_verify_timing.json"))
    a = ap.parse_args()
    import gnark_mi355x as gm
    big = 1 << a.logm
    res = {"reps": a.reps, "warmup": a.warmup, "unit": "ms", "m": big, "mad_rate": MAD_RATE, "curves": {}}
    pv_kern = ["points_check_g1", "plonk_verify_scalars", "plonk_verify_terms", "plonk_verify_assemble", "pairing_miller",
               "pairing_reduce", "pairing_final_exp"]
    with gm.Context(0) as ctx:
        for curve in CURVES:
            c = pyref.CURVES[curve]
            out = {}
            for nbp in (1, 16):
                for nb in (0, 1):
                    for m in (big, 1):
                        vkd, arrays = plonk_inputs(curve, 1 << 20, nbp, nb, m)
                        vk = gm.PlonkVk(ctx, curve, vkd)
                        try:
                            def run():
                                st, ok = vk.verify_batch(*arrays)
                                assert ok == 0 and set(st.tolist()) == {gm.PLONK_VERIFY_MISMATCH}, set(st.tolist())
                            e = {"wall": pct._timed(run, a.reps, a.warmup)}
                            if m == big:
                                e["kernels"] = pct._kernel_ms(ctx, run, a.reps, pv_kern)
                                for k in ("scalars", "terms", "assemble"):
                                    e[k] = pct._kernel_ms(ctx, run, a.reps, ["plonk_verify_" + k])
                                cnt = ladder_counts(c, 18 + 2 * nb)
                                e["counts"] = dict(cnt, mads=mads(curve, cnt), miller_lanes=2, final_exponentiations=1)
                                t = (e["terms"]["median"] + e["assemble"]["median"]) * 1e-3
                                e["mad_bound"] = round(mads(curve, cnt) * m / MAD_RATE / t, 3)
                            out["plonk_m%d_public%d_bsb%d" % (m, nbp, nb)] = e
                        finally:
                            vk.free()
            # Groth16 beside it: sixteen public inputs, the same m, the same process
            rng = random.Random(7)
            g16 = gm.VerifyingKey(ctx, curve, dict(alpha_g1=pct.points(curve, False, 1, 41), beta_g2=pct.points(curve, True, 1, 42),
                                                    gamma_g2=pct.points(curve, True, 1, 43), delta_g2=pct.points(curve, True, 1, 44),
                                                    k_g1=pct.points(curve, False, 17, 45)))
            try:
                g1, g2 = pct.points(curve, False, 2 * big, 51).reshape(big, 2, -1), pct.points(curve, True, big, 52).reshape(big, -1)
                proofs = np.concatenate([g1[:, 0], g2, g1[:, 1]], axis=1).reshape(-1)
                pub = tile(pvm.enc(c, [rng.randrange(c.r) for _ in range(DISTINCT * 16)]), big // DISTINCT)

                def run16():
                    st, ok = g16.verify_batch(proofs, pub)
                    assert ok == 0
                cnt = ladder_counts(c, 16)
                e = {"wall": pct._timed(run16, a.reps, a.warmup),
                     "terms": pct._kernel_ms(ctx, run16, a.reps, ["g16_verify_ksum_terms"]),
                     "assemble": pct._kernel_ms(ctx, run16, a.reps, ["g16_verify_ksum_assemble"]),
                     "counts": dict(cnt, mads=mads(curve, cnt), miller_lanes=4, final_exponentiations=1)}
                out["g16_m%d_inputs16" % big] = e
            finally:
                g16.free()
            # KZG: 2^(logm + 2) openings, per opening and folded
            mk = 4 * big
            kk = gm.KzgVk(ctx, curve, pct.points(curve, False, 1, 71), pct.points(curve, True, 1, 72), pct.points(curve, True, 1, 73))
            try:
                dig, prf = pct.points(curve, False, mk, 74), pct.points(curve, False, mk, 75)
                fr = lambda seed: tile(pvm.enc(c, pyref.random_scalars(c, DISTINCT, seed)), mk // DISTINCT)
                z, y, lam = fr(76), fr(77), fr(78)

                def runk():
                    st, ok = kk.verify_batch(dig, prf, z, y)
                    assert ok == 0

                def runf():
                    assert kk.verify_folded(dig, prf, z, y, lam) == gm.KZG_VERIFY_MISMATCH
                out["kzg_m%d" % mk] = {"wall": pct._timed(runk, a.reps, a.warmup),
                                       "terms": pct._kernel_ms(ctx, runk, a.reps, ["kzg_verify_terms"]),
                                       "kernels": pct._kernel_ms(ctx, runk, a.reps, ["points_check_g1", "kzg_verify_terms", "kzg_verify_assemble", "pairing_miller", "pairing_reduce", "pairing_final_exp"])}
                out["kzg_folded_m%d" % mk] = {"wall": pct._timed(runf, a.reps, a.warmup),
                                              "terms": pct._kernel_ms(ctx, runf, a.reps, ["kzg_verify_terms"])}
            finally:
                kk.free()
            res["curves"][curve] = out
            print(curve, json.dumps(out), flush=True)
            ctx.trim()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
