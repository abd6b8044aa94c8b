#!/usr/bin/env python3
"""Times the point codec beside the point check, in one process (not part of
bench.py, not a test).

  python tools/points_decode_timing.py [--reps 5] [--warmup 1] [--size 22] [--key 20]
                                       [--out profiles/points_decode_timing.json]

Medians of `reps` runs with min and max after `warmup` runs (ms), kernel time by
HIP events around the launch (gm_profile_*).  Per curve and group, n = 2^--size
resident records:
  decode   gm_points_decode, compressed and raw, with the subgroup check and with
           GM_DECODE_NO_SUBGROUP_CHECK
  encode   gm_points_encode, compressed and raw
  check    gm_points_check over the same points, the sibling
  key      BN254 and BLS12-377: a synthetic key at 2^--key from a WriteTo-shaped
           and a WriteRawTo-shaped file through gm_g16_pk_upload_encoded, and
           from a WriteDump-shaped file through gm_g16_pk_upload_dump: host wall
           clock of the whole call (files in the page cache)
Points: those of tools/points_check_timing.py (4096 small multiples of the
generator with random signs, tiled; all in the subgroup).  The records are the
device encoder's, which the tests pin byte for byte.  On BLS12-377 the
Tonelli-Shanks trip count depends on the point: tiled points repeat the same
4096 counts.
"""
import argparse
import json
import os
import struct
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for sub_ in ("gnark-icicle_amd", "oracle", "tests", "tools"):
    sys.path.insert(0, os.path.join(ROOT, sub_))
from points_check_timing import CURVES, SIBLING_CURVES, _kernel_ms, _timed, points  # noqa: E402

WIDTHS = (("compressed", 0), ("raw", 1))


def kname(op, raw, g2):
    return "points_%s%s_%s" % (op, "_raw" if raw else "", "g2" if g2 else "g1")


def time_group(gm, ctx, curve, g2, n, reps):
    host = points(curve, g2, n, 23)
    out = {"point_bytes": int(host.size)}
    P = ctx.copy_points_to_device(curve, host, g2)
    try:
        def check():
            rep = ctx.points_check(curve, P, n, g2)
            assert rep["first_bad"] == n, rep
        check()
        out["check_kernel"] = _kernel_ms(ctx, check, reps, ["points_check_g2" if g2 else "points_check_g1"])
        for wname, width in WIDTHS:
            enc, bad = ctx.points_encode(curve, P, n, g2, width)
            assert bad == 0
            try:
                def encode():
                    e, b = ctx.points_encode(curve, P, n, g2, width)
                    e.free()
                out["encode_%s_kernel" % wname] = _kernel_ms(ctx, encode, reps, [kname("encode", width, g2)])
                for fname, flags in (("checked", 0), ("no_subgroup_check", gm.DECODE_NO_SUBGROUP_CHECK)):
                    def decode():
                        pts, rep = ctx.points_decode(curve, enc, n, g2, width, flags)
                        pts.free()
                        assert rep["first_bad"] == n and rep["infinities"] == 0, rep
                    decode()
                    out["decode_%s_%s_kernel" % (wname, fname)] = _kernel_ms(ctx, decode, reps,
                                                                             [kname("decode", width, g2)])
            finally:
                enc.free()
    finally:
        P.free()
    return out


def time_key(gm, ctx, curve, logn, reps, warmup, tmp):
    n = 1 << logn
    nb_wires, nb_public = n + 2, 2
    g1 = lambda cnt, seed: points(curve, False, cnt, seed)
    pk = {"g1_alpha": g1(1, 1), "g1_beta": g1(1, 2), "g1_delta": g1(1, 3), "g1_A": g1(nb_wires, 4),
          "g1_B": g1(nb_wires, 5), "g1_Z": g1(n - 1, 6), "g1_K": g1(nb_wires - nb_public, 7),
          "g2_beta": points(curve, True, 1, 8), "g2_delta": points(curve, True, 1, 9),
          "g2_B": points(curve, True, nb_wires, 10),
          "infA": np.zeros(nb_wires, np.uint8), "infB": np.zeros(nb_wires, np.uint8)}
    order = (("g1_alpha", False, False), ("g1_beta", False, False), ("g1_delta", False, False), ("g1_A", False, True),
             ("g1_B", False, True), ("g1_Z", False, True), ("g1_K", False, True), ("g2_beta", True, False),
             ("g2_delta", True, False), ("g2_B", True, True))
    counts = (nb_wires, nb_wires, nb_wires - nb_public)
    meta = dict(infA=pk["infA"], infB=pk["infB"], k_wires=None, counts=counts)
    out = {}
    for wname, width in WIDTHS:
        path = os.path.join(tmp, "%s_%s.bin" % (curve, wname))
        with open(path, "wb") as f:
            for key, g2, is_slice in order:
                cnt = pk[key].size // gm.point_bytes(curve, g2)
                P = ctx.copy_points_to_device(curve, pk[key], g2)
                enc, bad = ctx.points_encode(curve, P, cnt, g2, width)
                assert bad == 0
                if is_slice:
                    f.write(struct.pack(">I", cnt))
                f.write(enc.to_host(cnt * gm.record_bytes(curve, g2, width)))
                P.free()
                enc.free()
        out["file_bytes_%s" % wname] = os.path.getsize(path)

        def load():
            k, end, rep, _ = gm.ProvingKey.from_encoded(ctx, curve, path, 0, meta, n, nb_wires, nb_public, width)
            k.free()
            assert end == os.path.getsize(path) and rep["first_bad_member"] is None
        out["upload_encoded_%s_wall" % wname] = _timed(load, reps, warmup)
        os.unlink(path)
    path = os.path.join(tmp, "%s.dump" % curve)
    gm.write_dump_slices(path, curve, pk)
    out["file_bytes_dump"] = os.path.getsize(path)
    dmeta = dict(meta, **{k: pk[k] for k in ("g1_alpha", "g1_beta", "g1_delta", "g2_beta", "g2_delta")})

    def dump():
        k, end = gm.ProvingKey.from_dump(ctx, curve, path, 0, dmeta, n, nb_wires, nb_public)
        k.free()
    out["upload_dump_wall"] = _timed(dump, reps, warmup)
    os.unlink(path)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--size", type=int, default=22)
    ap.add_argument("--key", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "points_decode_timing.json"))
    a = ap.parse_args()
    import gnark_mi355x as gm
    res = {"reps": a.reps, "warmup": a.warmup, "unit": "ms", "lib_bytes": os.path.getsize(gm.LIB_PATH),
           "groups": {}, "key": {}}
    with gm.Context(0) as ctx, tempfile.TemporaryDirectory() as tmp:
        for curve in CURVES:
            for g2 in (False, True):
                key = "%s_%s_2p%d" % (curve, "g2" if g2 else "g1", a.size)
                res["groups"][key] = time_group(gm, ctx, curve, g2, 1 << a.size, a.reps)
                print(key, json.dumps(res["groups"][key]), flush=True)
            ctx.trim()
        if a.key:
            for curve in SIBLING_CURVES:
                k = "%s_2p%d" % (curve, a.key)
                res["key"][k] = time_key(gm, ctx, curve, a.key, a.reps, a.warmup, tmp)
                print("key", k, json.dumps(res["key"][k]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
