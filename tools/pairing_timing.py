#!/usr/bin/env python3
"""Times the device pairing beside its nearest sibling, in one process (not part
of bench.py, not a test).

  python tools/pairing_timing.py [--reps 5] [--warmup 1] [--logn 16] [--out profiles/pairing_timing.json]

Medians of `reps` runs with min and max after `warmup` runs (ms); kernel times are
HIP events around the launches (gm_profile_*).  Per curve:
  pairs     gm_pairing_check_device over 2^logn pairs as products of four: the
            Miller loop (2^logn lanes), the reduce launch and the final
            exponentiation (2^(logn - 2) lanes each); and over products of one pair,
            which puts 2^logn lanes into the final exponentiation
  sibling   gm_points_check on 2^logn G2 points, the ladder of Fp2 doublings
  verify    gm_g16_verify_batch at m = 1 and m = 2^(logn - 2) (four Miller lanes per
            proof) with one and with sixteen public inputs: wall clock, the kernels
            summed, and the share of kSum (ladders and sums) in the kernels
`mads` counts each kernel's multiply-adds per lane from its formulas (a product
2 N^2, a squaring N^2 + N (N + 1) / 2, N limbs), `mad_bound` is that over the
time at 30.7 T mad/s, as for the point check.
Points are subgroup points (tiled multiples of the generators), so every lane
runs its whole loop; the proofs are such points too and are rejected (status 2)
after the full work.
"""
import argparse
import json
import os
import random
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for sub_ in ("gnark-icicle_amd", "oracle", "tests", "tools"):
    sys.path.insert(0, os.path.join(ROOT, sub_))
import pyref  # noqa: E402
import pairing_constants as pcn  # noqa: E402
import points_check_timing as pct  # noqa: E402

CURVES = ("bn254", "bls12377", "bls12381")
MAD_RATE = 30.7e12


def op_counts(name):
    """(Fp products, Fp squarings) per lane of the Miller loop, a reduce step of
    four values and the final exponentiation, from pairing_impl.hpp's formulas."""
    d = pcn.derive(name)
    c, u = d["c"], abs(d["u"])
    m2, s2, scale2 = 3, 2, 2
    mul6 = 6 * m2
    mul12, sqr12 = 3 * mul6, 2 * mul6
    line = 2 * mul6 + 3 * m2                      # two mul6_01 and a scaling (D) or a mul6_1 (M)
    dbl = 5 * s2 + 10 * m2 + 2 * scale2
    add = 2 * s2 + 11 * m2 + 2 * scale2
    loop = d["loop"]
    iters, adds = loop.bit_length() - 1, bin(loop).count("1") - 1
    miller = iters * (sqr12 + dbl + line) + adds * (add + line)
    if d["bn"]:
        miller += 2 * (add + line) + 3 * 2 * m2   # the two closing lines, psi three times
    cyc = 9 * s2
    exp_u = (u.bit_length() - 1) * cyc + (bin(u).count("1") - 1) * mul12
    frob = 5 * m2
    inv_sq, inv_mul = 8 * c.fp_limbs * 8, bin(c.p - 2).count("1")           # Fermat: a squaring per bit
    inv6 = 3 * s2 + 9 * m2 + 3 * m2 + 4                                       # and the Fp2 inverse's four products
    inv12 = 4 * mul6 + inv6
    easy = inv12 + 2 * mul12 + frob
    if d["bn"]:
        hard = 3 * exp_u + 7 * cyc + 12 * mul12 + 3 * frob
    else:
        hard = 5 * exp_u + cyc + 7 * mul12 + 2 * frob
    return {"miller": (miller, 0), "reduce4": (3 * mul12, 0), "final_exp": (easy + hard + inv_mul, inv_sq + 2)}


def mads(name, counts):
    n = pcn.n29(pcn.derive(name)["c"])
    return counts[0] * 2 * n * n + counts[1] * (n * n + n * (n + 1) // 2)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--logn", type=int, default=16)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pairing_timing.json"))
    a = ap.parse_args()
    import gnark_mi355x as gm
    n = 1 << a.logn
    res = {"reps": a.reps, "warmup": a.warmup, "unit": "ms", "pairs": n, "mad_rate": MAD_RATE, "curves": {}}
    with gm.Context(0) as ctx:
        for curve in CURVES:
            c = pyref.CURVES[curve]
            counts = op_counts(curve)
            out = {"fp_ops_per_lane": {k: {"products": v[0], "squarings": v[1], "mads": mads(curve, v)}
                                       for k, v in counts.items()}}
            h1, h2 = pct.points(curve, False, n, 31), pct.points(curve, True, n, 32)
            P1, P2 = ctx.copy_to_device(h1), ctx.copy_to_device(h2)
            try:
                for k in (4, 1):
                    run = lambda: ctx.pairing_check_device(curve, P1, P2, n // k, k)
                    key = "products_of_%d" % k
                    out[key] = {"wall": pct._timed(run, a.reps, a.warmup)}
                    for kern in ("pairing_miller", "pairing_reduce", "pairing_final_exp"):
                        out[key][kern] = pct._kernel_ms(ctx, run, a.reps, [kern])
                lanes = {"pairing_miller": ("products_of_4", n, "miller"), "pairing_reduce": ("products_of_4", n // 4, "reduce4"),
                         "pairing_final_exp": ("products_of_1", n, "final_exp")}
                out["mad_bound"] = {}
                for kern, (key, ln, cnt) in lanes.items():
                    t = out[key][kern]["median"] * 1e-3
                    out["mad_bound"][kern] = round(mads(curve, counts[cnt]) * ln / MAD_RATE / t, 3) if t else None
                chk = lambda: ctx.points_check(curve, P2, n, True)
                out["sibling_points_check_g2"] = pct._kernel_ms(ctx, chk, a.reps, ["points_check_g2"])
            finally:
                P1.free()
                P2.free()
            # verification: subgroup points as the key and the proofs
            rng = random.Random(7)
            for nb_in in (1, 16):
                vk = gm.VerifyingKey(ctx, curve, dict(alpha_g1=pct.points(curve, False, 1, 41), beta_g2=pct.points(curve, True, 1, 42),
                                                      gamma_g2=pct.points(curve, True, 1, 43), delta_g2=pct.points(curve, True, 1, 44),
                                                      k_g1=pct.points(curve, False, nb_in + 1, 45)))
                try:
                    for m in (1, n // 4):
                        g1, g2 = pct.points(curve, False, 2 * m, 51).reshape(m, 2, -1), pct.points(curve, True, m, 52).reshape(m, -1)
                        proofs = np.concatenate([g1[:, 0], g2, g1[:, 1]], axis=1).reshape(-1)
                        pub = b"".join(pyref.encode_fr(c, rng.randrange(c.r)) for _ in range(m * nb_in))
                        def run():
                            st, ok = vk.verify_batch(proofs, pub)
                            assert ok == 0 and set(st.tolist()) == {2}
                        kern = ["g16_verify_split", "points_check_g1", "points_check_g2", "g16_verify_ksum_terms",
                                "g16_verify_ksum_assemble", "pairing_miller", "pairing_reduce", "pairing_final_exp"]
                        e = {"wall": pct._timed(run, a.reps, a.warmup), "kernels": pct._kernel_ms(ctx, run, a.reps, kern),
                             "ksum": pct._kernel_ms(ctx, run, a.reps, kern[3:5])}
                        e["ksum_share_of_kernels"] = round(e["ksum"]["median"] / e["kernels"]["median"], 3)
                        out["verify_m%d_inputs%d" % (m, nb_in)] = e
                finally:
                    vk.free()
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
