/* Test-only entry points: element-wise device primitives of the field / curve
 * layer, used by the parity tests (tests/test_field_gpu.py) to pin each
 * arithmetic primitive against the oracle.  Built into
 * libgnark_mi355x_testhooks.so (csrc/testhooks.hip), which links against
 * libgnark_mi355x.so; the product library does not contain them.  Not on the
 * proving path, and nothing in the reference's FFI corresponds to them. */
#ifndef GNARK_MI355X_TESTHOOKS_H
#define GNARK_MI355X_TESTHOOKS_H

#include "gnark_mi355x.h"

#ifdef __cplusplus
extern "C" {
#endif

/* kind: 0 = Fr, 1 = Fp, 2 = Fp2; op: 0 mul, 1 add, 2 sub, 3 neg, 4 inv, 5 sqr.
 * Point op (affine in/out): 0 mixed add, 1 double, 2 XYZZ add, 3 [1000003]P. */
int gm_test_field_op(gm_ctx* ctx, int curve, int kind, int op, const void* a_dev,
                     const void* b_dev, void* out_dev, size_t n);
int gm_test_point_op(gm_ctx* ctx, int curve, int g2, int op, const void* a_dev,
                     const void* b_dev, void* out_dev, size_t n);

/* fe_sqrt (csrc/field_sqrt.hpp) on its own: n elements in gnark form at a_dev,
 * kind 1 = Fp, 2 = Fp2 ({A0, A1}).  root_dev receives n elements in gnark form,
 * exists_dev n bytes: 1 and a square root where the element is a square, else 0
 * (the element at root_dev is then unspecified). */
int gm_test_fe_sqrt(gm_ctx* ctx, int curve, int kind, const void* a_dev, size_t n, void* root_dev,
                    uint8_t* exists_dev);

/* The pairing's layers on their own (csrc/pairing_impl.hpp).  An Fp12 element is
 * twelve Fp in gnark Montgomery form in gnark-crypto's E12 memory order
 * (C0.B0.A0, C0.B0.A1, C0.B1.A0, ... C1.B2.A1); a_dev, b_dev and out_dev hold n of
 * them, 16-byte aligned, except:
 *   LINE_MUL  b_dev holds the line as an Fp12 element of which only the line's
 *             three slots are read (w^0, w^1, w^3 on the D-twists; w^0, w^2, w^3
 *             on BLS12-381): out = a times that sparse element;
 *   MILLER    a_dev holds n gnark G1 points, b_dev n gnark G2 points (on the
 *             curve and in the subgroup, or (0, 0)): out = the Miller values.
 * INV sends 0 to 0.  CYC_SQR and EXP_U (a^|u|) are defined on elements of the
 * cyclotomic subgroup only.  FINAL_EXP: out = a^(s (p^12 - 1) / r), s as in
 * DESIGN.md section 3.11.  b_dev is read by MUL, LINE_MUL and MILLER only. */
enum {
  GM_TPAIR_MUL = 0, GM_TPAIR_SQR, GM_TPAIR_INV, GM_TPAIR_CONJ, GM_TPAIR_FROB1, GM_TPAIR_FROB2, GM_TPAIR_CYC_SQR,
  GM_TPAIR_LINE_MUL, GM_TPAIR_EXP_U, GM_TPAIR_MILLER, GM_TPAIR_FINAL_EXP, GM_TPAIR_OPS
};
int gm_test_pairing_op(gm_ctx* ctx, int curve, int op, const void* a_dev, const void* b_dev, size_t n,
                       void* out_dev);

/* Raw-limb hooks for the lazily reduced layer (field.hpp "Lazily reduced
 * arithmetic", curve.hpp, pair_fp2.hpp).  Elements cross the boundary as the
 * internal radix-2^29 limbs: N little-endian u32 per element (N = 9, or 14 for
 * BLS12-377 Fp), loaded and stored as they are -- no form conversion, no
 * reduction -- so the caller picks the representative v + j p going in and sees
 * every limb coming out.
 *
 * Field hook: kind 0 = Fr, 1 = Fp.  op = family * 100 + K, K the function's
 * template constant (0 where it has none); chain = 0, 1, 2 is the product's
 * CHAIN level (ignored by functions without one).  Scalar families take the
 * operand arrays a..d with N limbs per element and write N limbs per element;
 * the Fp2 families (GM_TRAW_FE2_MUL and up) take and write 2 N limbs per
 * element, component a0 then a1.  Unused operands may be NULL (read as 0).  A
 * (family, K, chain) the library does not instantiate for that field, or that
 * the limb-count guard of the function excludes, is GM_ERR_INVALID. */
#define GM_TRAW_MUL_LZ 0       /* fe_mul<P, false, CH>(a, b) */
#define GM_TRAW_SQR_LZ 1       /* fe_sqr<P, false, CH>(a) */
#define GM_TRAW_MUL 2          /* fe_mul<P, true, CH>(a, b) */
#define GM_TRAW_MUL2 3         /* fe_mul2_redc_u<P, CH>(a, b, c, d) */
#define GM_TRAW_MUL2_NEGK 4    /* fe_mul2_redc_u<P, CH>(a, b, fe_negk_cf<K>(c), d) */
#define GM_TRAW_ADD_LZ 5       /* fe_add_lz(a, b) */
#define GM_TRAW_SUB_LZ 6       /* fe_sub_lz<K>(a, b) */
#define GM_TRAW_SUB2X_LZ 7     /* fe_sub2x_lz<K>(a, b, c) */
#define GM_TRAW_SUB_CF_MUL 8   /* fe_mul<P, false, CH>(fe_sub_cf<K>(a, b), c) */
#define GM_TRAW_CNEG_SUB 9     /* fe_sub_lz<K>(fe_cneg2p_cf(a, d[0] & 1), b) */
#define GM_TRAW_PMINUS 10      /* fe_pminus(a) */
#define GM_TRAW_REDUCE_K 11    /* fe_reduce_k<K>(a) */
#define GM_TRAW_CANON 12       /* fe_canon<K>(a) */
#define GM_TRAW_TO2P 13        /* fe_to2p<K>(a) */
#define GM_TRAW_IS_ZERO 14     /* fe_is_zero_lz<K>(a): limb 0 = 0 or 1, the rest 0 */
#define GM_TRAW_TIMES5 15      /* fe_times5_lz(a) */
#define GM_TRAW_FE2_MUL 16     /* one lane: fe2_mul_lz(a, b) */
#define GM_TRAW_FE2_SQR 17     /* one lane: fe2_sqr_lz<K>(a) */
#define GM_TRAW_PF2_MUL 18     /* lane pair: pf2_mul<P, BETA, CH>(a, b) */
#define GM_TRAW_PF2_SQR 19     /* lane pair: pf2_sqr<P, BETA, K, CH>(a) */
#define GM_TRAW_PF2_MUL_SUB 20 /* lane pair: pf2_mul_sub(a, b, c, d) = a b - c d */
#define GM_TRAW_MUL4_REDC 21   /* fe_mul4_redc(a0, a1, b0, b1, c0, c1, d0, d1), result in a0's place */
int gm_test_field_raw_op(gm_ctx* ctx, int curve, int kind, int op, int chain, const void* a_dev, const void* b_dev,
                         const void* c_dev, const void* d_dev, void* out_dev, size_t n);

/* Point hook: acc_in / acc_out are raw XYZZ accumulators, 4 N limbs (x, y, zz,
 * zzz), 8 N for G2 in the XYZZ<Fe2> word order (x.a0, x.a1, y.a0, ...).  other
 * is a gnark-layout affine point (the _AFF ops) or a second raw XYZZ;
 * flags[i] & 1 is the digit sign (the point is subtracted).  chain: G1 mixed
 * add 0 or 2, lane-pair mixed add 0 or 1, else 0. */
#define GM_TRAW_G1_ADD_AFF 0   /* xyzz_add_aff_lz<P, CH>(acc, other, sign) */
#define GM_TRAW_G1_ADD 1       /* xyzz_add_lz(acc, other) */
#define GM_TRAW_G1_CANON 2     /* xyzz_canon_raw(acc) */
#define GM_TRAW_G2_ADD_AFF 3   /* one lane: xyzz_add_aff_lz(acc, sign ? -other : other) */
#define GM_TRAW_G2P_ADD_AFF 4  /* lane pair: pxyzz_add_aff<P, BETA, CH>(acc, other, sign) */
#define GM_TRAW_G2P_DBL_AFF 5  /* lane pair: pxyzz_dbl_aff(other) */
#define GM_TRAW_G2P_ADD 6      /* lane pair: pxyzz_add(acc, other) */
#define GM_TRAW_G2P_DBL 7      /* lane pair: pxyzz_dbl(acc) */
int gm_test_point_raw_op(gm_ctx* ctx, int curve, int g2, int op, int chain, const void* acc_in_dev,
                         const void* other_dev, const void* flags_dev, void* acc_out_dev, size_t n);

/* Replays the level shape of the reference benchmark circuit (a chain of
 * squarings: level j finishes constraint j and solves wire nb_inputs + j)
 * through gm_g16_stage_put_indexed: mode 0 one put per level and vector, mode 1
 * the Go level hook's gathering (a put every flush_at ids); abc = 0 stages the
 * wires only.  Reports the host time per level. */
int gm_test_stage_replay_chain(gm_g16_stage* st, const void* wires, size_t nb_inputs, const void* a,
                               const void* b, const void* c, size_t nb_constraints, int mode, int abc,
                               size_t flush_at, double* ns_per_level);

/* Builds the sort plan of n scalars without sorted keys (a G1-only plan) and
 * hands it to the G2 launch, which must refuse it: returns that launch's code
 * (GM_ERR_INVALID expected; gm_last_error names the missing keys).  points_dev
 * holds n G2 points; nothing reads them when the launch refuses. */
int gm_test_msm_g2_keyless_plan(gm_ctx* ctx, int curve, const void* scalars_dev, const void* points_dev, size_t n);

/* The device-wide u32 scans (csrc/scan.hpp) on their own, arrays of u32 on the
 * device.  op 0: the exclusive sum scan of in_dev[0, n) into out_dev[0, n], the
 * total in out_dev[n]; out_dev may be in_dev; the workspace comes from the arena
 * and is filled with 0xFF bytes first.  op 1: in_dev[0, n) is copied to out_dev
 * and becomes its exclusive running maximum (from 0) in place, by one block. */
int gm_test_scan(gm_ctx* ctx, int op, const void* in_dev, size_t n, void* out_dev);

/* Host-only report of the geometry an MSM of n scalars derives from its sizes:
 * the functions the driver itself calls (msm.hpp msm_plan_geom, msm_seg_geom,
 * msm_tree_geom), with no context and no device.  c_override is the window as
 * gm_set_msm_window takes it (0: the cost model); for the precomputed layout it
 * is the window of the prepared set of n points (0: the shared-bucket cost
 * model, as gm_precompute_layout reports it).  GM_ERR_INVALID with
 * gm_last_error where the plan would refuse the MSM. */
#define GM_TGEOM_PLAIN 0    /* gnark-layout points, GLV split off */
#define GM_TGEOM_GLV 1      /* gnark-layout points, GLV split on */
#define GM_TGEOM_PRECOMP 2  /* precomputed set, one shared bucket set */
#define GM_TGEOM_DEFAULT 3  /* gnark-layout points, GLV by the size rule */
#define GM_TGEOM_MAX_LEVELS 24
typedef struct gm_test_msm_geom {
  /* plan */
  uint32_t c, W;            /* window bits, windows */
  uint32_t wn, narrow;      /* first narrow (c - 1 bit) window; W - wn */
  uint32_t Wred, nb, total; /* windows reduced separately; buckets per window; Wred * nb */
  uint32_t glv, shared;     /* the layout taken (GM_TGEOM_DEFAULT resolves glv) */
  uint32_t bits;            /* scalar bits the digits cover */
  uint32_t F, G, NC, NS, compact; /* the sort's bins and entry width */
  uint32_t piece_len;       /* G1 piece length by the size rule */
  /* launch and reduction */
  uint32_t L, nseg;         /* level-1 segment length and segments per window */
  uint32_t levels, lg[GM_TGEOM_MAX_LEVELS]; /* LDS tree levels, log2 of each group */
  uint32_t Q;               /* points per exported node */
  uint32_t xyzz_bytes;      /* bytes of one bucket of this group */
  uint64_t n, M, npts;      /* (virtual) points, entry bound, addressable points */
  uint64_t bucket_bytes, node_bytes, offset_bytes; /* what the launch and the plan allocate for them */
} gm_test_msm_geom;
int gm_test_msm_geometry(int curve, int g2, size_t n, int c_override, int layout, gm_test_msm_geom* out);

/* The scalars kernel of gm_plonk_verify_batch alone (the proofs' points are not
 * read): per proof the 18 + 2 nb_bsb scalars in the order of the ladders
 *   G, Ql, Qr, Qm, Qo, S3, S1, S2, Qcp_j; L, R, O, Z, H0, H1, H2, Hb, Hz, Bsb_j; u
 * to scalars_out, PI(zeta) and constLin to aux_out (2 per proof), all Montgomery
 * fr.Elements, and to class_out the proof's class without the points:
 * GM_PLONK_VERIFY_OK, _BAD_INPUT or _ALGEBRAIC.  One chunk: m is small. */
int gm_test_plonk_verify_scalars(gm_ctx* ctx, const gm_plonk_vk* vk, const gm_plonk_proofs_host* proofs, size_t m,
                                 void* scalars_out, void* aux_out, uint8_t* class_out);
/* gm_plonk_verify_batch with per_chunk whole proofs per chunk instead of the
 * computed count. */
int gm_test_plonk_verify_chunked(gm_ctx* ctx, const gm_plonk_vk* vk, const gm_plonk_proofs_host* proofs, size_t m,
                                 size_t per_chunk, uint8_t* status_out, size_t* nb_ok);
/* The KZG entries with per_chunk whole openings per chunk: fold == 0 is
 * gm_kzg_verify_batch, fold != 0 is gm_kzg_verify_folded, which writes one status
 * byte and sets *nb_ok to 0 or 1. */
int gm_test_kzg_verify_chunked(gm_ctx* ctx, const gm_kzg_vk* vk, const gm_kzg_openings_host* openings, size_t m,
                               size_t per_chunk, int fold, uint8_t* status_out, size_t* nb_ok);

#ifdef __cplusplus
}
#endif

#endif
