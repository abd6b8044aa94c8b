/*
 * gnark_mi355x.h -- C-ABI of the MI355X (gfx950) MSM + NTT backend for gnark's
 * Groth16 prover.  Drop-in replacement for the device layer that
 * backend/groth16/bn254/icicle/icicle.go binds through
 * github.com/ingonyama-zk/iciclegnark v0.1.0 (go.mod:15; not vendored -- the
 * signatures below are the ones its call sites in icicle.go imply).
 *
 * Conventions
 *  - Plain C, no torch / HIP types in signatures.  Device buffers are opaque
 *    `void*` device pointers owned by the caller and released with gm_free
 *    (iciclegnark's unsafe.Pointer + FreeDevicePointer model).
 *  - Host pointers are only read/written during the call and never retained
 *    (cgo rule).  Every entry point selects its context's device itself.
 *  - Memory layout is gnark-crypto's, byte for byte: fr.Element / fp.Element =
 *    little-endian u64 limbs in Montgomery form; G1Affine {X,Y}; G2Affine
 *    {X.A0,X.A1,Y.A0,Y.A1}; G1Jac/G2Jac {X,Y,Z}; infinity affine = all zero.
 *  - Every function returns GM_OK (0) or a negative gm_status; the message of
 *    the last failure on the calling thread is available from gm_last_error().
 *  - Calls on one context are serialised; use one context per thread/GPU for
 *    concurrency.  Multi-GPU: either one process drives every GPU through one
 *    gm_multi handle: gm_g16_pk_upload_multi / gm_g16_prove_multi, or one process per
 *    GPU holds a key shard (gm_g16_pk_upload_shard / gm_g16_prove_partial).
 */
#ifndef GNARK_MI355X_H
#define GNARK_MI355X_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
  GM_OK = 0,
  GM_ERR_INVALID = -1,     /* bad argument / unsupported size */
  GM_ERR_DEVICE = -2,      /* HIP runtime error */
  GM_ERR_OOM = -3,         /* device allocation failed */
  GM_ERR_UNSUPPORTED = -4, /* curve/group combination not built */
} gm_status;

/* Curve ids.  BN254 and BLS12-377 are served by every entry that takes a curve.
 * BLS12-381 (Fp 381 bits = 6 x u64, Fr 255 bits = 4 x u64, G1 96 B, G2 192 B) is
 * served by the host group helpers, the point uploads, every MSM entry, the NTT /
 * poly-ops / computeH calls, the KZG commit / open calls, the Groth16 key
 * upload and prover (gm_g16_pk_upload[_ex], gm_g16_prove[_device], gm_g16_finish,
 * gm_g16_partial_bytes) and the point validation of what those uploads take
 * (gm_points_check, gm_points_check_host, gm_g16_pk_check; gm_g16_pk_check_dump
 * stands with the dump loader below) and the point codec (gm_points_decode,
 * gm_points_decode_host, gm_points_encode).  Every other entry that takes a curve --
 * the PLONK calls
 * and gm_kzg_srs_lagrange, gm_r1cs_upload and what needs it (gm_g16_prove_r1cs,
 * gm_g16_setup*, gm_g16_pk_setup), gm_batch_mul_fixed / gm_batch_mul_base, the
 * key dump / cache loaders, gm_g16_pk_upload_shard / _multi, gm_g16_prove_partial,
 * the staged-input calls and gm_icicle_* -- answers GM_ERR_UNSUPPORTED for it,
 * before any allocation, upload or launch, with a message that names the curve
 * and the entry.  Any other id is GM_ERR_INVALID, "unknown curve id". */
typedef enum { GM_BN254 = 0, GM_BLS12_377 = 1, GM_BLS12_381 = 2 } gm_curve;

typedef struct gm_ctx gm_ctx;

/* ---- context ---------------------------------------------------------- */
const char* gm_last_error(void);
int gm_version(void);
/* Number of visible HIP devices. */
int gm_device_count(int* count);
/* Creates a context on HIP device `device` with its own streams. */
int gm_init(int device, gm_ctx** out);
int gm_destroy(gm_ctx* ctx);
int gm_synchronize(gm_ctx* ctx);
/* Releases the device memory a context keeps for reuse between calls: the
 * workspace arenas, the a / b / c input buffer of host-input proves (3 n Fr,
 * 1.5 GB at 2^24), the pinned H2D ring, the cached NTT domain tables and the
 * staging buffers parked with keys by gm_g16_stage_free (3 n + nb_wires Fr plus
 * 64 MiB pinned and 64 MiB device per key) and the session buffers parked with
 * PLONK keys by gm_plonk_session_free.  All
 * are re-created on demand by the next call that needs them.  Refused
 * (GM_ERR_INVALID) while gm_msm_async MSMs are pending.  Call it before
 * uploading a key whose GM_PK_PRECOMPUTE_AUTO decision should see that memory
 * as free. */
int gm_trim(gm_ctx* ctx);
/* Per-kernel timing with HIP events on the context stream (bench/profiling). */
int gm_profile_enable(gm_ctx* ctx, int on);
int gm_profile_reset(gm_ctx* ctx);
/* Fetches accumulated time (ms) and launch count for kernel `name`. */
int gm_profile_get(gm_ctx* ctx, const char* name, double* total_ms, uint64_t* count);
/* Writes "name total_ms count\n" lines into buf (truncated to cap). */
int gm_profile_dump(gm_ctx* ctx, char* buf, size_t cap);
/* Test/tuning knob: force the MSM window size c (0 = automatic). */
int gm_set_msm_window(gm_ctx* ctx, int c);
/* GLV split (k = k1 + k2 lambda over P_i and phi(P_i), BN254 and BLS12-377) of
 * MSMs over gnark-layout points: mode 1 on, 0 off, -1 default (on up to 2^21
 * points unless GM_MSM_GLV=0; G2 also unless GM_MSM_GLV_G2=0).  Tuning / A-B
 * knob; results are identical either way. */
int gm_set_msm_glv(gm_ctx* ctx, int mode);
/* Test/tuning knob: G1 MSMs accumulate pieces of at most t entries of one
 * bucket each (1..128; 0 = the built-in size rule).  Results are identical for
 * every t. */
int gm_set_msm_piece_len(gm_ctx* ctx, int t);

/* ---- memory (iciclegnark CopyToDevice / CopyPointsToDevice /
 *      CopyG2PointsToDevice / FreeDevicePointer; icicle.go:44,47,65,90,95,
 *      109,114,125,245,269,352,356,416-418,478-480,492,505-507) ---------- */
int gm_malloc(gm_ctx* ctx, size_t bytes, void** dev_out);
int gm_free(gm_ctx* ctx, void* dev);
int gm_copy_to_device(gm_ctx* ctx, const void* host, size_t bytes, void** dev_out);
int gm_memcpy_h2d(gm_ctx* ctx, void* dev, const void* host, size_t bytes);
int gm_memcpy_d2h(gm_ctx* ctx, void* host, const void* dev, size_t bytes);
int gm_memcpy_d2d(gm_ctx* ctx, void* dst_dev, const void* src_dev, size_t bytes);
/* Uploads n gnark affine points of (curve, g2) -> device buffer. */
int gm_copy_points_to_device(gm_ctx* ctx, int curve, int g2, const void* host_points, size_t n,
                             void** dev_out);

/* ---- MSM (iciclegnark MsmOnDevice icicle.go:302,315,332,355 and
 *      MsmG2OnDevice icicle.go:382; CPU twin G1Jac/G2Jac.MultiExp
 *      prove.go:204,217,237,247,293) ------------------------------------
 * out = sum_i int(scalars[i]) * points[i], scalars = n Montgomery fr.Element,
 * points = n gnark affine points ((0,0) = infinity is allowed), both resident
 * on the device.  out_jac receives gnark's G1Jac (3 x fp) / G2Jac (3 x E2)
 * layout; out_affine (optional, may be NULL) receives the affine form. */
int gm_msm(gm_ctx* ctx, int curve, int g2, const void* scalars_dev, const void* points_dev,
           size_t n, void* out_jac, void* out_affine);
/* Pipelined MSM: gm_msm_async queues the device work of gm_msm (same
 * arguments) and returns at once; gm_msm_wait finishes it (host tail: checks
 * and the Horner combination) and frees the handle.  The host tail of one MSM
 * thus overlaps the device work of the next one issued before it.  At most three
 * MSMs may be in flight per context; wait in issue order.  Each in-flight MSM
 * runs on a stream of its own (GM_MSM_SLOT_STREAMS=0: the context stream), at
 * the highest stream priority (a hardware-queue pool of their own, so they do
 * not share a queue with the context's other streams; GM_MSM_SLOT_PRIO=0: normal
 * priority), so one MSM's reduction overlaps the next one's conversion and sort.
 * The MSM starts after the work already queued on the context stream (its
 * inputs).  gm_msm_async and gm_msm_wait queue nothing on the context stream;
 * the next call that does waits there for the pending MSMs' input reads first.
 * (The library also raises GPU_MAX_HW_QUEUES to 8 at load time when the
 * variable is unset.)  Synchronous calls
 * (gm_msm, gm_msm_prepared, gm_ntt, ...) may be made on the same context while
 * async MSMs are pending: each pending MSM keeps its own scratch arena and its
 * own pinned readback buffer until its gm_msm_wait, and work queued on the
 * context after gm_msm_async returns starts only once that MSM has read its
 * scalars and points, so such a call may overwrite them in place.
 * gm_destroy with MSMs pending waits for their device work and releases their
 * resources; each pending handle stays allocated, and its gm_msm_wait returns
 * GM_ERR_INVALID ("context was destroyed") and frees it. */
typedef struct gm_msm_pending gm_msm_pending;
int gm_msm_async(gm_ctx* ctx, int curve, int g2, const void* scalars_dev, const void* points_dev, size_t n,
                 gm_msm_pending** out);
int gm_msm_wait(gm_msm_pending* pending, void* out_jacobian, void* out_affine);
/* gm_msm with the scalars in host memory (copied on the context stream). */
int gm_msm_host_scalars(gm_ctx* ctx, int curve, int g2, const void* scalars_host,
                        const void* points_dev, size_t n, void* out_jac, void* out_affine);

/* Device-resident point sets (a proving key's arrays, a KZG SRS): upload n gnark
 * affine points once, converted to the MSM's internal layout (same byte size),
 * and run MSMs over any prefix of them without per-call conversion.  Free with
 * gm_free.  (setupDevicePointers, icicle.go:90-125, keeps pk points resident.) */
int gm_points_upload(gm_ctx* ctx, int curve, int g2, const void* host_points, size_t n,
                     void** prepared_out);
int gm_msm_prepared(gm_ctx* ctx, int curve, int g2, const void* scalars_dev, const void* prepared,
                    size_t n, void* out_jac, void* out_affine);

/* Fixed-base precomputation (ICICLE's MSM precompute_factor idea, re-derived):
 * besides the n points, W-1 copies [2^(c w)] P_i (w = 1..W-1) are stored, so
 * every window's digits share one bucket set and the bucket reduction runs
 * once instead of W times (and c can grow).  window = c in [2, 24], or 0 =
 * automatic from n.  Memory: W x the plain prepared size.  The copy count W =
 * ceil((r_bits + 1) / c) is reported by gm_precompute_layout.  An MSM over
 * any prefix n <= prepared_n of the set passes the SAME prepared_n and window
 * used at upload. */
int gm_precompute_layout(int curve, size_t prepared_n, int window, int* c_out, int* copies_out);
int gm_points_upload_precomputed(gm_ctx* ctx, int curve, int g2, const void* host_points, size_t n,
                                 int window, void** prepared_out);
int gm_msm_precomputed(gm_ctx* ctx, int curve, int g2, const void* scalars_dev, const void* prepared,
                       size_t prepared_n, int window, size_t n, void* out_jac, void* out_affine);

/* ---- KZG commitment (PLONK; backend/plonk/bls12-377/prove.go:312,460,718,
 *      1158-1168 call gnark-crypto kzg.Commit) ---------------------------------
 * digest = sum_i coeffs[i] * srs[i] over the first n points of a prepared SRS
 * (pk.Kzg.G1 or pk.KzgLagrange.G1, setup.go:81-82), coeffs = n Montgomery
 * fr.Elements in host memory.  GM_ERR_INVALID if n > srs_len (kzg.ErrInvalidPolynomialSize). */
int gm_kzg_commit(gm_ctx* ctx, int curve, const void* srs_prepared, size_t srs_len,
                  const void* coeffs_host, size_t n, void* digest_affine);

/* ---- KZG openings (PLONK; prove.go:611 kzg.Open, :757 kzg.BatchOpenSinglePoint)
 * The polynomial work of an opening on polynomials resident on the device
 * (n Montgomery fr.Elements each, 16-byte aligned, e.g. from gm_copy_to_device):
 * evaluation at z, the fold sum_i gamma^i f_i, and the division by X - z
 * (gnark-crypto's dividePolyByXminusA).  Fr results are canonical, so values and
 * quotient coefficients are gnark-crypto's bytes.  z, gamma and the returned
 * values are single Montgomery fr.Elements in host memory.  polys_dev is a host
 * array of k device pointers, lens their lengths in elements; k is not capped.
 * GM_ERR_INVALID for k == 0 or m == 0.
 *
 * A batch opening takes two calls because the Fiat-Shamir gamma depends on the
 * claimed values: upload the polynomials once, gm_kzg_eval, derive gamma on the
 * host, gm_kzg_batch_open on the same buffers.
 *
 *  - gm_kzg_eval: values_host[i] = f_i(z), k elements (a length of 0 gives 0).
 *  - gm_poly_div_linear: q_dev[0..m-2] = (f - f(z)) / (X - z), *value_host = f(z).
 *    m >= 1; m == 1 writes nothing to q_dev.  q_dev must not overlap f_dev
 *    (GM_ERR_INVALID if it does); f_dev is left unchanged.
 *  - gm_poly_fold: out_dev[0..max(lens)-1] = sum_i gamma^i f_i; a polynomial
 *    contributes nothing at and past its own length.
 *  - gm_kzg_open: *claimed_host = f(z) and h_affine = the commitment of the
 *    quotient over the first m - 1 points of a prepared SRS (gm_points_upload);
 *    the quotient never leaves the device.  GM_ERR_INVALID if m > srs_len
 *    (kzg.ErrInvalidPolynomialSize).  A constant polynomial (m == 1) gives the
 *    identity (0, 0).
 *  - gm_kzg_batch_open: the same for F = sum_i gamma^i f_i, m = max(lens);
 *    *folded_value_host (may be NULL) = F(z) = sum_i gamma^i f_i(z). */
int gm_kzg_eval(gm_ctx* ctx, int curve, const void* const* polys_dev, const size_t* lens, size_t k,
                const void* z_host, void* values_host);
int gm_poly_div_linear(gm_ctx* ctx, int curve, const void* f_dev, size_t m, const void* z_host,
                       void* q_dev, void* value_host);
int gm_poly_fold(gm_ctx* ctx, int curve, const void* const* polys_dev, const size_t* lens, size_t k,
                 const void* gamma_host, void* out_dev);
int gm_kzg_open(gm_ctx* ctx, int curve, const void* srs_prepared, size_t srs_len, const void* f_dev, size_t m,
                const void* z_host, void* claimed_host, void* h_affine);
int gm_kzg_batch_open(gm_ctx* ctx, int curve, const void* srs_prepared, size_t srs_len,
                      const void* const* polys_dev, const size_t* lens, size_t k, const void* z_host,
                      const void* gamma_host, void* folded_value_host, void* h_affine);

/* ---- PLONK quotient (backend/plonk/bls12-377/prove.go:771-1034 computeNumerator,
 *      :1178-1231 divideByZH) ----------------------------------------------------
 * The quotient stage on polynomials resident on the device: h_dev receives h, the
 * inputs stay where they are and are left unchanged.
 *
 * Every device polynomial is n Montgomery fr.Elements in the canonical basis,
 * regular (natural) layout, 16-byte aligned.  l, r, o, z are NOT blinded: the
 * blinding polynomials come as host coefficients (bl, br, bo: 2 elements, degree
 * 1; bz: 3 elements, degree 2).  qcp / pi2 are host arrays of nb_bsb device
 * pointers (the BSB22 commitment gates; nb_bsb may be 0, the tables then are not
 * read).  alpha, beta, gamma are single host elements.  h_dev holds 4n elements
 * and must overlap no input.
 *
 * With g = FrMultiplicativeGen, w1 the generator of the 4n domain, w0 = w1^4,
 * Z_H = X^n - 1, L~ = L + Z_H bl (R~, O~, Z~ likewise), L1 = Z_H / (n (X - 1)):
 *   T = Ql L~ + Qr R~ + Qm L~ R~ + Qo O~ + Qk + sum_i Qcp_i PI2_i
 *     + alpha [ (L~ + beta S1 + gamma)(R~ + beta S2 + gamma)(O~ + beta S3 + gamma) Z~(w0 X)
 *             - (L~ + beta X + gamma)(R~ + beta g X + gamma)(O~ + beta g^2 X + gamma) Z~ ]
 *     + alpha^2 (Z~ - 1) L1
 * and h is the polynomial of degree < 4n with h(x) = T(x) / Z_H(x) at the 4n
 * points x = g w1^k: for a satisfying witness the quotient (degree <= 3n + 5),
 * for any other input still well defined.  h_dev is in canonical, regular order;
 * the prover's h1, h2, h3 are h[0:n+2], h[n+2:2n+4], h[2n+4:3n+6] and can go into
 * gm_msm_prepared where they lie.  Every element is fully reduced, so the bytes
 * are gnark's.  StatisticalZK's randomised h coefficients are the caller's.
 *
 * GM_ERR_INVALID: NULL context (checked before any device call), NULL struct or
 * required pointer, n not a power of two or n < 8 (the reference's 8n domain for
 * tiny circuits is not built), nb_bsb > 0 with a NULL table or entry, a
 * misaligned pointer, h_dev overlapping an input.  Scratch ((13 + 2 nb_bsb) n
 * elements) comes from the context's workspace; gm_trim releases it. */
typedef struct {
  size_t n;                        /* domain0 size: a power of two, >= 8 */
  const void *ql, *qr, *qm, *qo, *qk, *s1, *s2, *s3;  /* device, n Fr each */
  const void *l, *r, *o, *z;       /* device, n Fr each, NOT blinded */
  size_t nb_bsb;                   /* BSB22 gates, may be 0 */
  const void* const* qcp;          /* host array of nb_bsb device pointers */
  const void* const* pi2;          /* host array of nb_bsb device pointers */
  const void *bl, *br, *bo;        /* host, 2 Fr each (blinding, degree 1) */
  const void *bz;                  /* host, 3 Fr (degree 2) */
  const void *alpha, *beta, *gamma;/* host, 1 Fr each */
} gm_plonk_quotient_in;
int gm_plonk_quotient(gm_ctx* ctx, int curve, const gm_plonk_quotient_in* in, void* h_dev);

/* ---- PLONK permutation polynomial Z (backend/plonk/bls12-377/prove.go:565-597
 *      buildRatioCopyConstraint, gnark-crypto iop.BuildRatioCopyConstraint) --------
 * The copy-constraint accumulator on polynomials resident on the device.  Every
 * device input is n Montgomery fr.Elements, 16-byte aligned, and is left unchanged:
 *  - l, r, o: Lagrange basis, regular order (element i is the value at w^i);
 *  - s1, s2, s3: Lagrange basis, regular order, s_k[i] = id[sigma(k n + i)] (gnark's
 *    trace.S1..S3 at setup), with the identity support id[k n + i] = g^k w^i,
 *    g = FrMultiplicativeGen (5 for BN254, 22 for BLS12-377), w the generator of
 *    fft.NewDomain(n).
 * beta and gamma are single host elements.  For i in [0, n - 1):
 *   num_i = (l[i] + beta w^i + gamma)(r[i] + beta g w^i + gamma)(o[i] + beta g^2 w^i + gamma)
 *   den_i = (l[i] + beta s1[i] + gamma)(r[i] + beta s2[i] + gamma)(o[i] + beta s3[i] + gamma)
 *   N_i = prod_{j<=i} num_j,   D_i = prod_{j<=i} den_j
 *   Z[0] = 1,   Z[i+1] = N_i inv0(D_i),   inv0(0) = 0, otherwise the field inverse
 * (BuildRatioCopyConstraint followed by fr.BatchInvert, which leaves zero entries
 * zero): from the first zero denominator on every later Z value is 0, the values
 * before it are unaffected.  Row n - 1 does not enter the product.
 *
 * z_lagrange_dev receives Z as n elements, Lagrange regular: it can go into
 * gm_msm_prepared over the Lagrange SRS where it lies.  z_canonical_dev, if not
 * NULL, receives the same polynomial in the canonical basis, regular order, NOT
 * blinded: the z member of gm_plonk_quotient_in.  Every stored element is fully
 * reduced, so the bytes are gnark's.  The outputs must overlap no input and must
 * not overlap each other.
 *
 * GM_ERR_INVALID: NULL context or NULL struct (both checked before any device
 * call), a NULL required pointer, n not a power of two or n < 8, a misaligned
 * pointer, an overlap.  Scratch (four elements per chunk of 512 rows) comes from
 * the context's workspace; gm_trim releases it. */
typedef struct {
  size_t n;                    /* power of two, >= 8 (as gm_plonk_quotient) */
  const void *l, *r, *o;       /* device, Lagrange regular */
  const void *s1, *s2, *s3;    /* device, Lagrange regular */
  const void *beta, *gamma;    /* host, 1 Fr each */
} gm_plonk_perm_in;
int gm_plonk_perm_z(gm_ctx* ctx, int curve, const gm_plonk_perm_in* in,
                    void* z_lagrange_dev, void* z_canonical_dev /* may be NULL */);

/* ---- PLONK linearized polynomial (backend/plonk/bls12-377/prove.go:656-724
 *      computeLinearizedPolynomial, :1233-1368 innerComputeLinearizedPoly) --------
 * The last polynomial stage of the prover on buffers resident on the device: the
 * evaluations at zeta, the linearized polynomial r(X) and, where asked for, the
 * blinded wires and Z~, so that the commit of r(X) (gm_msm_prepared), the opening
 * of Z~ at w zeta (gm_kzg_open) and the batch opening at zeta (gm_kzg_eval,
 * gm_kzg_batch_open) run where the data lie.
 *
 * The first twenty members of the input are gm_plonk_quotient_in's (same
 * conventions: canonical basis, regular order, n Montgomery fr.Elements each,
 * 16-byte aligned, l, r, o, z NOT blinded, qk the completed Qk); h is
 * gm_plonk_quotient's h_dev (4n elements, of which h[0 .. 3(n + 2)) are read);
 * h_rand, if not NULL, holds the two StatisticalZK randomizers of the quotient
 * shards (prove.go:619-654).  Every input is left unchanged.
 *
 * With g = FrMultiplicativeGen, w the generator of fft.NewDomain(n), m = n + 2,
 * Z_H(zeta) = zeta^n - 1 and P~ = P + (X^n - 1) b (as coefficients
 * getBlindedCoefficients, prove.go:1103-1111: P~[i] = P[i] - b[i] for i < len(b),
 * P~[n + i] = b[i]), evals receives, in this order,
 *   l~(zeta), r~(zeta), o~(zeta), s1(zeta), s2(zeta), z~(w zeta), qcp_j(zeta) (j < nb_bsb)
 * (the blinded ones as evaluateBlinded, :1073-1100), and with
 *   rl  = l~(zeta) r~(zeta)
 *   c1  = alpha (l~(zeta) + beta s1(zeta) + gamma)(r~(zeta) + beta s2(zeta) + gamma) beta z~(w zeta)
 *   c2  = -alpha (l~(zeta) + beta zeta + gamma)(r~(zeta) + beta g zeta + gamma)(o~(zeta) + beta g^2 zeta + gamma)
 *   a2L = alpha^2 (zeta^n - 1) inv0(zeta - 1) / n      (inv0(0) = 0: 0 at zeta = 1)
 *   zm  = zeta^m,   zh = zeta^n - 1
 * lin receives, for i in [0, n + 3), every polynomial contributing 0 at and past
 * its own length,
 *   lin[i] = (c2 + a2L) z~[i]
 *          + c1 s3[i] + rl qm[i] + l~(zeta) ql[i] + r~(zeta) qr[i] + o~(zeta) qo[i] + qk[i]
 *          + sum_j qcp_j(zeta) pi2_j[i]                                  (all of these: i < n)
 *          - zh (h[i] + zm h[m + i] + zm^2 h[2m + i])                    (i < m)
 * and, with h_rand = (rho0, rho1), lin[0] gains zh (zm rho0 + zm^2 rho1) and
 * lin[m] gains -zh (rho0 + zm rho1).  This is innerComputeLinearizedPoly's return
 * value byte for byte: every stored element is fully reduced.  l_blinded,
 * r_blinded, o_blinded (n + 2 elements) and z_blinded (n + 3), each of which may
 * be NULL, receive the blinded coefficient lists.
 *
 * GM_ERR_INVALID: NULL context, NULL in or NULL out (all checked before any
 * device call), a NULL required pointer, n not a power of two or n < 8,
 * nb_bsb > 0 with a NULL table or entry, a misaligned device pointer, an output
 * overlapping an input or another output.  nb_bsb is not capped.  Scratch (the
 * evaluations' chunk sums and nb_bsb table entries) comes from the context's
 * workspace; gm_trim releases it. */
typedef struct {
  size_t n;                                   /* domain0 size: power of two, >= 8 */
  const void *ql, *qr, *qm, *qo, *qk, *s1, *s2, *s3;  /* device, n Fr each (qk = completed Qk) */
  const void *l, *r, *o, *z;                  /* device, n Fr each, NOT blinded */
  size_t nb_bsb;                              /* may be 0; not capped */
  const void* const* qcp;                     /* host array of nb_bsb device pointers */
  const void* const* pi2;                     /* host array of nb_bsb device pointers */
  const void *bl, *br, *bo;                   /* host, 2 Fr each */
  const void *bz;                             /* host, 3 Fr */
  const void *h;                              /* device, 4n Fr: gm_plonk_quotient's h_dev */
  const void *h_rand;                         /* host, 2 Fr (StatisticalZK randomizers) or NULL */
  const void *alpha, *beta, *gamma, *zeta;    /* host, 1 Fr each */
} gm_plonk_linearize_in;

typedef struct {
  void *lin;                                  /* device, n + 3 Fr, required */
  void *l_blinded, *r_blinded, *o_blinded;    /* device, n + 2 Fr each, each may be NULL */
  void *z_blinded;                            /* device, n + 3 Fr, may be NULL */
  void *evals;                                /* host, 6 + nb_bsb Fr, required */
} gm_plonk_linearize_out;

int gm_plonk_linearize(gm_ctx* ctx, int curve, const gm_plonk_linearize_in* in,
                       const gm_plonk_linearize_out* out);

/* ---- PLONK proving key resident on the device (gnark plonk.ProvingKey,
 *      backend/plonk/bls12-377/setup.go; the PLONK twin of gm_g16_pk_upload) ---------
 * Uploaded once per circuit; any number of prover sessions run on it one after
 * another, and none of them writes to it.  Every host polynomial is n Montgomery
 * fr.Elements, Lagrange basis, regular order (element i is the value at w^i), as
 * gnark's trace holds them at setup: ql, qr, qm, qo, s1, s2, s3, the qcp_j, and qk
 * WITHOUT the public inputs and commitment values, which a session writes per
 * proof to rows [0, nb_public) and commitment_row[j] (prove.go:363-389; the rows
 * are already offset by nb_public).  srs_canonical is pk.Kzg.G1 (tau^i G,
 * srs_canonical_len >= n + 3 gnark G1Affine), srs_lagrange is pk.KzgLagrange.G1
 * (L_i(tau) G, n points).  No host pointer is kept after the call returns.
 *
 * The key keeps on the device: both SRSs in the MSM's layout (the form
 * gm_points_upload makes); every fixed polynomial in the canonical basis, s1, s2,
 * s3 and qk also as Lagrange values; and, unless GM_PLONK_PK_NO_COSET_CACHE is
 * set, the values of ql, qr, qm, qo, s1, s2, s3, L1 = (X^n - 1) / (n (X - 1)) and
 * every qcp_j on each of the four cosets g w1^i <w0> of the 4n domain (gm_plonk_quotient's
 * names), in the order and number form the quotient's own transforms produce:
 * 4 (8 + nb_bsb) n elements of 32 bytes (4.3 GB at n = 2^22, nb_bsb = 0).  A
 * session's quotient then transforms only qk, l, r, o, z and the pi2_j per coset
 * (5 + nb_bsb transforms instead of 13 + 2 nb_bsb); its results are the same
 * bytes with and without the cache.  Qk is never cached: it differs per proof.
 *
 * gm_plonk_pk_bytes reports the device bytes of the key, the cache included, and
 * the cache's share (0 without it); either pointer may be NULL.
 *
 * GM_ERR_INVALID: NULL context, struct or out (checked before any device call), a
 * NULL polynomial or SRS, n not a power of two or n < 8 (as gm_plonk_quotient),
 * srs_canonical_len < n + 3, nb_public > n, nb_bsb > 0 with a NULL table or
 * entry, nb_bsb > 1024, a commitment_row >= n, an unknown flag. */
typedef struct gm_plonk_pk gm_plonk_pk;
typedef struct {
  size_t n;                 /* domain0 size: power of two, >= 8 */
  size_t nb_public;         /* rows [0, nb_public) of Qk receive the public inputs */
  const void *ql, *qr, *qm, *qo, *qk, *s1, *s2, *s3;  /* host, n Fr each, Lagrange regular */
  size_t nb_bsb;
  const void* const* qcp;          /* host array of nb_bsb host pointers, n Fr each */
  const size_t* commitment_row;    /* nb_bsb rows of Qk that receive commitment_vals[j] */
  const void* srs_canonical;       /* gnark G1Affine */
  size_t srs_canonical_len;        /* >= n + 3 */
  const void* srs_lagrange;        /* gnark G1Affine, n points */
} gm_plonk_pk_host;
#define GM_PLONK_PK_NO_COSET_CACHE 1u
/* Round 4 of a session on this key builds the linearised polynomial from the key's
 * qk, as gnark's innerComputeLinearizedPoly does (prove.go:1301-1337 reads trace.Qk;
 * the completed Qk serves the quotient alone), so that lin, its claimed value and the
 * batch opening are the ones gnark's Verify and gm_plonk_verify_batch accept.  Without
 * the flag round 4 takes the completed Qk, the behaviour of this entry before the
 * flag existed: those proofs are refused by a gnark verifier (errAlgebraicRelation)
 * whenever a public input or a commitment value is non-zero, and are kept only so
 * that bytes recorded earlier stay reproducible.  One more inverse transform of n
 * elements per proof; the same flag is taken by every entry that makes a gm_plonk_pk.
 * Bit 2u is not assigned and stays refused as an unknown flag. */
#define GM_PLONK_PK_LIN_KEY_QK 4u
int gm_plonk_pk_upload(gm_ctx* ctx, int curve, const gm_plonk_pk_host* pk, unsigned flags, gm_plonk_pk** out);
int gm_plonk_pk_bytes(const gm_plonk_pk* pk, size_t* resident_bytes, size_t* coset_cache_bytes);
int gm_plonk_pk_free(gm_ctx* ctx, gm_plonk_pk* pk);

/* ---- PLONK prover session (backend/plonk/bls12-377/prove.go Prove: the five
 *      rounds on a resident key) ---------------------------------------------------
 * One session is one proof.  Its buffers live on the device from gm_plonk_session_begin
 * to gm_plonk_session_free; per proof only the solver's L, R, O and the public
 * inputs (or, with resident wire tables, the witness alone: see
 * gm_plonk_session_round1_witness below), the committed values, the blinding
 * scalars and the challenges go in, and digests, claimed values and opening
 * proofs come out.  The Fiat-Shamir transcript stays with the caller
 * (ChallengeHash and KZGFoldingHash are prover options): every challenge enters
 * as one Montgomery fr.Element in host memory, as with gm_kzg_batch_open.  Every
 * host vector is Montgomery fr.Elements; every digest is one gnark G1Affine.  The
 * outputs are the bytes prove.go produces for the same inputs.
 *
 *  - bsb22 (prove.go:292-327), once per j < nb_bsb before round 1: the committed-
 *    values polynomial j (n elements, Lagrange regular) is uploaded and kept in
 *    both bases; digest_affine = its commit over the Lagrange SRS (not blinded).
 *  - round 1 (:331-417, :458-468, :1114-1127): l, r, o (n elements each, Lagrange
 *    regular: solution.L / R / O) are uploaded and also taken to canonical form;
 *    Qk is completed (the key's qk with public_inputs on rows [0, nb_public) and
 *    commitment_vals[j] on commitment_row[j]); lro_affine receives the three
 *    commits of the blinded wires P~ = P + (X^n - 1) b: the commit of the values
 *    over the Lagrange SRS plus sum_k b_k (G_n+k - G_k) over the canonical one.
 *    bl, br, bo (2 elements: b_0 + b_1 X), bz (3) and h_rand (2, or NULL: no
 *    StatisticalZK) are copied for the later rounds.
 *  - round 2 (:565-597): Z as gm_plonk_perm_z defines it, from beta and gamma;
 *    z_affine = the commit of Z~ = Z + (X^n - 1) bz.
 *  - round 3 (:486-563, :619-654, :1154-1173): h as gm_plonk_quotient defines it,
 *    from alpha, read from the key's coset cache where the key has one.  With
 *    m = n + 2, h_affine receives the commits of h[0:m], h[m:2m], h[2m:3m] over
 *    the canonical SRS; with h_rand = (rho0, rho1) those of h1 || rho0, of h2
 *    with [0] -= rho0 followed by rho1, and of h3 with [0] -= rho1.
 *  - round 4 (:600-617, :656-724): the linearized polynomial as gm_plonk_linearize
 *    defines it, from zeta, over the completed Qk or, on a key made with
 *    GM_PLONK_PK_LIN_KEY_QK, over the key's qk as gnark does (see the flag: only
 *    those proofs pass gnark's Verify); lin_affine = its commit; claimed receives, in the
 *    order of polysToOpen (:736-744), lin(zeta), l~(zeta), r~(zeta), o~(zeta),
 *    s1(zeta), s2(zeta), qcp_j(zeta) (6 + nb_bsb elements): what the caller derives
 *    the folding challenge from; z_shifted_value = z~(w zeta) and
 *    z_shifted_h_affine = the proof of kzg.Open of Z~ at w zeta.
 *  - round 5 (:726-767): batch_h_affine = the proof of kzg.BatchOpenSinglePoint of
 *    [lin, l~, r~, o~, s1, s2, qcp_j] at zeta with the folding challenge kzg_gamma.
 *
 * The rounds are a state machine: GM_ERR_INVALID, with a message and the session
 * left as it was, for a round out of order, a bsb22 call after round 1 or with
 * j >= nb_bsb, round 1 before every bsb22 call, a NULL required pointer
 * (public_inputs may be NULL iff nb_public == 0; commitment_vals is NULL iff
 * nb_bsb == 0), a key of another context.  A NULL context, key, session, input
 * struct or out is refused before any device call.  Calls on the session's
 * context are serialised as for every entry; scratch comes from the context's
 * workspace (gm_trim releases it, also between rounds).  The session must be
 * freed before its key and its context.  gm_plonk_session_free leaves the
 * session's device buffer (about 18 + 2 nb_bsb polynomials of n elements) with
 * the key, and the next gm_plonk_session_begin on that key takes it: a prover
 * loop allocates once, not per proof, and no proof reads what an earlier one
 * wrote.  gm_trim, gm_destroy and gm_plonk_pk_free release that buffer;
 * gm_plonk_pk_bytes does not count it. */
typedef struct gm_plonk_session gm_plonk_session;
int gm_plonk_session_begin(gm_ctx* ctx, gm_plonk_pk* pk, gm_plonk_session** out);
int gm_plonk_session_bsb22(gm_plonk_session* s, size_t j, const void* committed_host, void* digest_affine);
typedef struct {
  const void *l, *r, *o;        /* host, n Fr each: solution.L / R / O, Lagrange regular */
  const void *public_inputs;    /* host, nb_public Fr */
  const void *commitment_vals;  /* host, nb_bsb Fr (NULL iff nb_bsb == 0) */
  const void *bl, *br, *bo;     /* host, 2 Fr each */
  const void *bz;               /* host, 3 Fr */
  const void *h_rand;           /* host, 2 Fr (StatisticalZK) or NULL */
} gm_plonk_round1_in;
int gm_plonk_session_round1(gm_plonk_session* s, const gm_plonk_round1_in* in, void* lro_affine /* 3 points */);
int gm_plonk_session_round2(gm_plonk_session* s, const void* beta, const void* gamma, void* z_affine);
int gm_plonk_session_round3(gm_plonk_session* s, const void* alpha, void* h_affine /* 3 points */);
int gm_plonk_session_round4(gm_plonk_session* s, const void* zeta, void* lin_affine,
                            void* claimed /* 6 + nb_bsb Fr */, void* z_shifted_value /* 1 Fr */,
                            void* z_shifted_h_affine);
int gm_plonk_session_round5(gm_plonk_session* s, const void* kzg_gamma, void* batch_h_affine);
int gm_plonk_session_free(gm_plonk_session* s);

/* ---- PLONK session from the witness: resident wire tables (gnark
 *      evaluateLROSmallDomain, constraint/bls12-377/system.go:173-217; the PLONK
 *      twin of gm_r1cs_upload) ---------------------------------------------------------
 * solution.L / R / O are a gather of the solver's values through three wire ids
 * per row that are fixed when the circuit is compiled:
 *   l[i] = values[xa[i]]   r[i] = values[xb[i]]   o[i] = values[xc[i]]
 * gm_plonk_wires_upload puts the three tables (n u32 each, 12 n bytes, reported
 * by gm_plonk_wires_bytes) on the device once per circuit.  The caller supplies
 * complete rows, the placeholder rows (i, 0, 0) of the public inputs and the
 * padding rows (0, 0, 0) included: the library gives no row a meaning.  The
 * tables belong to no curve and to no key: a gm_plonk_pk is never written, and
 * one table object serves any number of sessions on keys of the same n.  Every id
 * is checked < nb_wires on the host before the upload, and gm_last_error names
 * the first offending table and row; the per-proof kernel reads inside the
 * witness without a check of its own.  No host pointer is kept.  The object is
 * freed before its context; gm_destroy releases the tables a context still owns.
 * GM_ERR_INVALID: a NULL argument (checked before any device call), n not a
 * power of two or n < 8, nb_wires = 0 or nb_wires > 2^32 - 1, an id >= nb_wires,
 * gm_plonk_wires_free on another context than the upload's.
 *
 * gm_plonk_gather_lro is the stage call on resident buffers: l, r, o (n elements
 * each) from witness (nb_wires elements) in one launch.  Elements are 32-byte
 * words moved untouched, so the call takes no curve.  GM_ERR_INVALID: a NULL
 * argument, tables of another context, a pointer that is not 16-byte aligned, an
 * output that overlaps the witness or another output.
 *
 * gm_plonk_session_round1_witness takes round 1's place in the state machine,
 * with round 1's preconditions: the witness (nb_wires elements, the solver's
 * values, whose first nb_public are the public inputs) is uploaded once, l, r, o
 * are gathered from it on the device, Qk's public rows are taken from
 * witness[0, nb_public), and the rest is round 1's.  Its outputs, and those of
 * every later round, are the bytes gm_plonk_session_round1 produces from the
 * host-gathered l, r, o and public_inputs = witness[0, nb_public).  Refused
 * besides what round 1 refuses: w->n != the key's n, nb_wires < nb_public, tables
 * of another context, NULL w or in (before the session is read).
 *
 * gm_plonk_session_bsb22_sparse is gm_plonk_session_bsb22 for a committed-values
 * vector given by its nonzero rows (prove.go:300-311: len(Committed) + 2 rows out
 * of n): the vector is zero-filled on the device and values[i] written to row
 * rows[i] for i < count; digest and session state are the bytes the dense call
 * gives for the same vector.  Rows are already offset by nb_public, as
 * commitment_row is; each must be < n and they must be pairwise distinct (a
 * duplicate is refused, not resolved); count = 0 is allowed, count > n refused.
 *
 * With the two calls the per-proof host input of a session is the witness
 * (32 nb_wires bytes, against 96 n for l, r, o), count (row, value) pairs per
 * commitment, the blinding scalars and the challenges. */
typedef struct gm_plonk_wires gm_plonk_wires;
int gm_plonk_wires_upload(gm_ctx* ctx, size_t n, size_t nb_wires,
                          const uint32_t* xa, const uint32_t* xb, const uint32_t* xc, /* host, n each */
                          gm_plonk_wires** out);
int gm_plonk_wires_bytes(const gm_plonk_wires* w, size_t* resident_bytes);
int gm_plonk_wires_free(gm_ctx* ctx, gm_plonk_wires* w);
int gm_plonk_gather_lro(gm_ctx* ctx, const gm_plonk_wires* w, const void* witness /* device, nb_wires Fr */,
                        void* l, void* r, void* o /* device, n Fr each */);
typedef struct {
  const void *witness;          /* host, nb_wires Fr: the solver's values */
  const void *commitment_vals;  /* host, nb_bsb Fr (NULL iff nb_bsb == 0) */
  const void *bl, *br, *bo;     /* host, 2 Fr each */
  const void *bz;               /* host, 3 Fr */
  const void *h_rand;           /* host, 2 Fr or NULL */
} gm_plonk_round1_witness_in;
int gm_plonk_session_round1_witness(gm_plonk_session* s, const gm_plonk_wires* w,
                                    const gm_plonk_round1_witness_in* in, void* lro_affine /* 3 points */);
int gm_plonk_session_bsb22_sparse(gm_plonk_session* s, size_t j, const uint32_t* rows /* host */,
                                  const void* values /* host, count Fr */, size_t count, void* digest_affine);

/* ---- PLONK setup on the device (gnark plonk.Setup, backend/plonk/bls12-377/setup.go,
 *      and the kzg.ToLagrangeG1 its caller runs first, backend/plonk/plonk.go:113-117) --
 * gm_kzg_srs_lagrange is the Lagrange-form SRS: srs_dev holds n gnark G1Affine
 * points on the device, the first n of pk.Kzg.G1 ((0,0) = infinity is allowed), and
 * lagrange_dev receives n gnark G1Affine points in natural order,
 *   out[i] = (1/n) sum_j w^(-ij) in[j],   w the generator of fft.NewDomain(n):
 * for in[j] = [tau^j] G that is [L_i(tau)] G, ToLagrangeG1's result, byte for byte
 * (affine coordinates fully reduced, infinity as (0,0)).  lagrange_dev == srs_dev
 * (in place) is allowed; the input is otherwise left unchanged.  n is a power of
 * two, 2 <= n <= 2^min(two-adicity, 30).  Scratch (one XYZZ point per input, 144 n
 * bytes for BN254 and 224 n for BLS12-377, plus 32 n of twiddles) comes from the
 * context's workspace.  G1 only.  GM_ERR_INVALID: a NULL argument, an unknown
 * curve, n out of range, the two ranges overlapping without being equal.
 *
 * gm_plonk_sigma is computePermutationPolynomials (setup.go:330-374) on gnark's
 * trace.S as it lies in memory: perm_host holds 3n int64, and
 *   s_k[i] = g^(S / n) w^(S mod n),  S = perm_host[k n + i],  g = FrMultiplicativeGen,
 * n Montgomery fr.Elements each, fully reduced, Lagrange regular: what
 * gm_plonk_perm_in and gm_plonk_pk_host take.  Every entry is checked against
 * 0 <= S < 3n on the host before any device call and gm_last_error names the first
 * offender; that S is a permutation is not checked (gnark does not either).  n as
 * above.  GM_ERR_INVALID: a NULL argument, an unknown curve, n out of range, an
 * entry out of range.
 *
 * gm_plonk_pk_setup makes the resident key from what Setup holds: the selector
 * polynomials as gm_plonk_pk_host has them, trace.S and the canonical SRS.  It
 * derives the Lagrange SRS from the first n canonical points and s1, s2, s3 from
 * the permutation, and then does what gm_plonk_pk_upload does, with the same
 * flags: the key is the same object (same gm_plonk_pk_bytes, same session outputs,
 * same lifetime rules).  vk_digests (host, 8 + nb_bsb gnark G1Affine) receives
 * commitTrace's commitments (setup.go:217-251) over the derived Lagrange SRS in
 * the VerifyingKey's order S1 S2 S3 Ql Qr Qm Qo Qk (incomplete) Qcp_j;
 * srs_lagrange_out (host, n gnark G1Affine, or NULL) receives the derived points,
 * for pk.KzgLagrange.  No host pointer is kept.  GM_ERR_INVALID: everything
 * gm_plonk_pk_upload refuses, a NULL permutation or vk_digests, a permutation
 * entry outside [0, 3n).
 *
 * The three _wires calls take the permutation from resident wire tables instead of
 * a host array, so that trace.S (24 n bytes) never crosses PCIe.  gnark's
 * buildPermutation (setup.go:271-325) reads lro = xa | xb | xc, which is a
 * gm_plonk_wires object's tables as they lie (3n u32, every id < nb_wires), and
 * links every position p to the largest q < p with lro[q] == lro[p], or to the
 * largest such q overall when there is none below p.  On the device that is a
 * stable radix sort of the positions by wire id and a link inside every run; the
 * result equals gnark's entry for entry and is a permutation by construction.
 * Scratch (48 n bytes of positions and keys, about 1.5 n of counters; nothing
 * sized by nb_wires) comes from the context's workspace.  The tables are left
 * unchanged.
 *
 * gm_plonk_wires_permutation is the stage call: perm_dev (device, 3n int64)
 * receives trace.S in gnark's element type, to be copied to the host when a CPU
 * Prove needs pk.trace.S.  It takes no curve and returns with the stream drained.
 * GM_ERR_INVALID (before any launch): a NULL argument, tables of another context,
 * perm_dev not 8-byte aligned or overlapping the tables, n > 2^30 (positions are
 * 32-bit, 3 * 2^30 < 2^32).
 *
 * gm_plonk_sigma_wires gives the bytes gm_plonk_sigma gives for that permutation
 * without materialising it as int64.  Refused besides the above: what
 * gm_plonk_sigma refuses of the curve and of n.
 *
 * gm_plonk_pk_setup_wires is gm_plonk_pk_setup with the permutation taken from w:
 * same flags, same key object, same vk_digests order, same srs_lagrange_out.
 * in->permutation must be NULL (a host permutation beside the tables is refused,
 * so that the call has one meaning), and w->n must equal in->n.  The key does not
 * refer to the tables afterwards. */
int gm_kzg_srs_lagrange(gm_ctx* ctx, int curve, const void* srs_dev, size_t n, void* lagrange_dev);
int gm_plonk_sigma(gm_ctx* ctx, int curve, size_t n, const int64_t* perm_host /* 3n */,
                   void* s1_dev, void* s2_dev, void* s3_dev /* n Fr each, Lagrange regular */);
typedef struct {
  size_t n, nb_public;
  const void *ql, *qr, *qm, *qo, *qk;   /* host, n Fr, Lagrange regular (qk incomplete) */
  const int64_t* permutation;           /* host, 3n: trace.S */
  size_t nb_bsb;
  const void* const* qcp;               /* host array of nb_bsb host pointers, n Fr each */
  const size_t* commitment_row;
  const void* srs_canonical;            /* gnark G1Affine */
  size_t srs_canonical_len;             /* >= n + 3 */
} gm_plonk_setup_host;
int gm_plonk_pk_setup(gm_ctx* ctx, int curve, const gm_plonk_setup_host* in, unsigned flags,
                      gm_plonk_pk** out, void* vk_digests /* host, 8 + nb_bsb G1Affine */,
                      void* srs_lagrange_out /* host, n G1Affine, or NULL */);
int gm_plonk_wires_permutation(gm_ctx* ctx, const gm_plonk_wires* w, int64_t* perm_dev /* device, 3n */);
int gm_plonk_sigma_wires(gm_ctx* ctx, int curve, const gm_plonk_wires* w,
                         void* s1_dev, void* s2_dev, void* s3_dev /* n Fr each, Lagrange regular */);
int gm_plonk_pk_setup_wires(gm_ctx* ctx, int curve, const gm_plonk_setup_host* in, const gm_plonk_wires* w,
                            unsigned flags, gm_plonk_pk** out, void* vk_digests, void* srs_lagrange_out);

/* ---- PLONK circuit on the device (gnark NewTrace, backend/plonk/bls12-377/
 *      setup.go:153-213; the PLONK twin of gm_r1cs_upload and gm_g16_pk_setup) ---------
 * One resident object per compiled circuit, made from what gnark holds compactly:
 * its []SparseR1C records as they lie in memory (constraint/r1cs_sparse.go:143-147,
 * nine u32 = 36 bytes per constraint: XA XB XC QL QR QO QM QC Commitment), the
 * CoeffTable (Montgomery fr.Elements, ids 0 and 1 being zero and one) and the
 * PlonkCommitments (Committed and CommitmentIndex, both constraint indices).  The
 * records go up once and a kernel splits them into the wire tables of
 * evaluateLROSmallDomain (rows (i, 0, 0) for i < nb_public, the constraints from
 * row nb_public on, (0, 0, 0) padding up to n), five columns of coefficient ids,
 * one byte of Commitment per constraint, the coefficient table and the committed
 * rows.  gm_plonk_scs_bytes reports the allocation.  No host pointer is kept.  The
 * object is freed before its context; gm_destroy releases what a context still
 * owns.  Curve ids 0 and 1.
 *
 * Everything is checked on the host before the first device call and
 * gm_last_error names the first offender and its record.  GM_ERR_INVALID: a NULL
 * argument; n not a power of two, n < 8, n > 2^30 or n < nb_public +
 * nb_constraints; nb_wires = 0, nb_wires < nb_public or nb_wires > 2^32 - 1; a
 * wire id >= nb_wires; a coefficient id >= ncoeffs; Commitment > 2; ncoeffs < 2;
 * nb_bsb > 1024; a committed index or commitment index >= nb_constraints
 * (duplicate committed indices are allowed); gm_plonk_scs_free on another context
 * than the upload's.
 *
 * gm_plonk_scs_wires hands out the wire tables inside the object: every call
 * that takes a gm_plonk_wires accepts them (gm_plonk_gather_lro,
 * gm_plonk_session_round1_witness, gm_plonk_wires_permutation,
 * gm_plonk_sigma_wires, gm_plonk_pk_setup_wires), gm_plonk_wires_free refuses them
 * with GM_ERR_INVALID, and they are freed with the circuit.
 *
 * gm_plonk_scs_selector writes one of NewTrace's columns (n Fr, Lagrange regular)
 * to out_dev: for GM_SCS_QL .. GM_SCS_QK, -1 (QL) or 0 on the rows of the public
 * inputs, coeffs[id] on the constraint rows, 0 on the padding (QK incomplete, as
 * gm_plonk_pk_host takes it); for GM_SCS_QCP0 + j, 1 on the rows nb_public +
 * Committed[j][i] and 0 elsewhere.  One launch per column.  GM_ERR_INVALID: a
 * NULL argument, which >= GM_SCS_QCP0 + nb_bsb, a circuit of another context,
 * out_dev not 16-byte aligned or overlapping the object.
 *
 * gm_plonk_pk_setup_scs is gm_plonk_pk_setup_wires with nothing dense from the
 * host: the curve, n, nb_public, nb_bsb and the commitment rows (nb_public +
 * CommitmentIndex[j]) come from the object, the permutation from its tables, and
 * every selector is generated on the device where the _wires call copies a host
 * vector.  The key, vk_digests (S1 S2 S3 Ql Qr Qm Qo Qk Qcp_j), srs_lagrange_out,
 * the flags and the refusals are those of the _wires call given the same
 * selectors.  The key does not refer to the circuit afterwards.  With it Setup
 * needs the constraint system and the canonical SRS, and a session's
 * gm_plonk_session_round1_witness needs the witness.
 *
 * gm_plonk_scs_check evaluates ql l + qr r + qm l r + qo o + qk on every
 * constraint whose Commitment is NOT (gnark's solver skips the others,
 * constraint/blueprint_scs.go:56-60) for a witness of nb_wires Fr on the host:
 * nb_unsatisfied receives the number of constraints where it is not zero,
 * first_unsatisfied the smallest such constraint index (untouched if there is
 * none).  Public placeholder rows and padding rows are not evaluated.  Returns
 * with the stream drained.  GM_ERR_INVALID: a NULL argument, a circuit of another
 * context. */
typedef struct gm_plonk_scs gm_plonk_scs;
typedef struct {
  size_t n;                 /* domain0 size: power of two, >= 8, >= nb_public + nb_constraints */
  size_t nb_public, nb_constraints, nb_wires;
  const uint32_t* records;  /* host, nb_constraints records of 9 u32 */
  const void* coeffs;       /* host, ncoeffs fr.Element, Montgomery: the CoeffTable */
  size_t ncoeffs;
  size_t nb_bsb;
  const uint32_t* const* committed;   /* nb_bsb host arrays: PlonkCommitment.Committed */
  const size_t* committed_len;
  const size_t* commitment_index;     /* nb_bsb: PlonkCommitment.CommitmentIndex */
} gm_plonk_scs_host;
int gm_plonk_scs_upload(gm_ctx* ctx, int curve, const gm_plonk_scs_host* in, gm_plonk_scs** out);
int gm_plonk_scs_bytes(const gm_plonk_scs* scs, size_t* resident_bytes);
int gm_plonk_scs_free(gm_ctx* ctx, gm_plonk_scs* scs);
int gm_plonk_scs_wires(const gm_plonk_scs* scs, const gm_plonk_wires** out /* borrowed */);
enum { GM_SCS_QL, GM_SCS_QR, GM_SCS_QM, GM_SCS_QO, GM_SCS_QK, GM_SCS_QCP0 /* + j */ };
int gm_plonk_scs_selector(gm_ctx* ctx, const gm_plonk_scs* scs, unsigned which,
                          void* out_dev /* device, n Fr, Lagrange regular */);
int gm_plonk_pk_setup_scs(gm_ctx* ctx, const gm_plonk_scs* scs, const void* srs_canonical,
                          size_t srs_canonical_len, unsigned flags, gm_plonk_pk** out,
                          void* vk_digests /* host, 8 + nb_bsb G1Affine */,
                          void* srs_lagrange_out /* host, n G1Affine, or NULL */);
int gm_plonk_scs_check(gm_ctx* ctx, const gm_plonk_scs* scs, const void* witness_host /* nb_wires Fr */,
                       size_t* nb_unsatisfied, size_t* first_unsatisfied /* constraint index */);

/* ---- NTT (iciclegnark GenerateTwiddleFactors icicle.go:68,73;
 *      INttOnDevice :489,502; NttOnDevice :490; PolyOps :500;
 *      ReverseScalars :510; CPU twin fft.Domain.FFT/FFTInverse
 *      prove.go:372-378,396) ---------------------------------------------
 * In-place transform of n = 2^k Montgomery fr.Elements with gnark-crypto
 * fft.Domain semantics:
 *   inverse = 0: coefficients -> evaluations at w^i (g*w^i if coset)
 *   inverse = 1: evaluations -> coefficients, scaled by 1/n (and g^-i if coset)
 *   dit = 0 (DIF): natural-order input, bit-reversed output
 *   dit = 1 (DIT): bit-reversed input, natural-order output
 * w = the domain generator of fft.NewDomain(n), g = FrMultiplicativeGen
 * (5 for BN254, 22 for BLS12-377). */
int gm_ntt(gm_ctx* ctx, int curve, void* data_dev, size_t n, int inverse, int dit, int coset);
/* a[i] <- (a[i]*b[i] - c[i]) * den   (PolyOps, den = (g^n - 1)^-1 broadcast) */
int gm_poly_ops(gm_ctx* ctx, int curve, void* a_dev, const void* b_dev, const void* c_dev,
                size_t n, const void* den_host);
/* In-place bit-reversal permutation of n = 2^k Fr elements (ReverseScalars). */
int gm_reverse_scalars(gm_ctx* ctx, int curve, void* data_dev, size_t n);

/* ---- iciclegnark call-for-call binding (icicle.go:68-76,489-510) --------
 * Same buffer ownership and element order as iciclegnark v0.1.0, so a cgo shim
 * can bind INttOnDevice / NttOnDevice / PolyOps / GenerateTwiddleFactors name
 * for name and icicle.go's computeH (icicle.go:453-513) runs unchanged,
 * including its FreeDevicePointer calls:
 *  - gm_icicle_intt_on_device: natural-order evaluations at in_dev -> a NEW
 *    device buffer (*out_dev, free with gm_free) of natural-order coefficients
 *    (times g^-i / n on the coset); in_dev is left bit-reversed, as iciclegnark
 *    leaves it (INttOnDevice, icicle.go:489,502).
 *  - gm_icicle_ntt_on_device: natural-order coefficients at in_dev -> natural-
 *    order evaluations (on the coset g*w^i if coset) at out_dev (NttOnDevice,
 *    icicle.go:490); out_dev == in_dev is allowed.
 *  - gm_icicle_poly_ops: a[i] <- (a[i]*b[i] - c[i]) * den[i], den a device
 *    vector (PolyOps with pk.DenDevice, icicle.go:52-65,500).
 *  - gm_icicle_generate_twiddles: builds the context's cached domain of size n
 *    and returns a freeable device token for pk.DomainDevice.Twiddles(Inv)
 *    (GenerateTwiddleFactors, icicle.go:68,73).
 * ReverseScalars (icicle.go:510) is gm_reverse_scalars, MsmOnDevice /
 * MsmG2OnDevice are gm_msm, CopyToDevice / CopyPointsToDevice are
 * gm_copy_to_device / gm_copy_points_to_device, FreeDevicePointer is gm_free. */
int gm_icicle_generate_twiddles(gm_ctx* ctx, int curve, size_t n, int inverse, void** token_out);
int gm_icicle_intt_on_device(gm_ctx* ctx, int curve, void* in_dev, size_t n, int coset, void** out_dev);
int gm_icicle_ntt_on_device(gm_ctx* ctx, int curve, void* out_dev, const void* in_dev, size_t n, int coset);
int gm_icicle_poly_ops(gm_ctx* ctx, int curve, void* a_dev, const void* b_dev, const void* c_dev,
                       const void* den_dev, size_t n);

/* ---- Groth16 computeH (icicle.go:453-513; prove.go:356-399) -----------
 * a, b, c: `len` Montgomery fr.Elements each (the R1CS solution vectors),
 * device-resident, zero-padded in place to n = domain size (buffers must hold
 * n elements).  On return a_dev holds h in BIT-REVERSED coefficient order
 * (matching pk.G1.Z, setup.go:265-267); b_dev and c_dev are clobbered. */
int gm_groth16_compute_h(gm_ctx* ctx, int curve, void* a_dev, void* b_dev, void* c_dev,
                         size_t len, size_t n);

/* ---- Groth16 prover (icicle_bn254.Prove, icicle.go:133-422; CPU twin
 *      groth16_bn254.Prove prove.go:62-325, without the BSB22 commitment
 *      side path) ---------------------------------------------------------
 * A proving key whose point arrays live on the device (uploaded once, as
 * icicle's setupDevicePointers, icicle.go:31-130). */
typedef struct gm_g16_pk gm_g16_pk;
typedef struct {
  size_t domain_size;      /* n = pk.Domain.Cardinality */
  size_t nb_wires;         /* len(InfinityA) */
  size_t nb_public;        /* r1cs.GetNbPublicVariables() (incl. ONE wire) */
  size_t nbA, nbB, nbK;    /* len(pk.G1.A), len(pk.G1.B), len(pk.G1.K) */
  const void* g1_alpha;    /* G1Affine */
  const void* g1_beta;
  const void* g1_delta;
  const void* g1_A;        /* nbA points */
  const void* g1_B;        /* nbB points */
  const void* g1_Z;        /* n-1 points, bit-reversed (setup.go:265-267) */
  const void* g1_K;        /* nbK points */
  const void* g2_beta;     /* G2Affine */
  const void* g2_delta;
  const void* g2_B;        /* nbB points */
  const uint8_t* infA;     /* nb_wires flags (InfinityA) */
  const uint8_t* infB;     /* nb_wires flags (InfinityB) */
  /* nbK wire indices whose values multiply pk.G1.K: wireValues[nb_public:]
   * minus the private-committed and commitment wires (prove.go:243-245,
   * filterHeap :331-354).  NULL = no commitments: nb_public + i. */
  const uint32_t* k_wires;
} gm_g16_pk_host;

int gm_g16_pk_upload(gm_ctx* ctx, int curve, const gm_g16_pk_host* pk, gm_g16_pk** out);
/* flags: GM_PK_PRECOMPUTE keeps fixed-base window copies of every point array
 * on the device (gm_points_upload_precomputed; ~12x the point memory at 2^24,
 * ~77 GB for a BN254 2^24 key) -- fewer windows and one bucket reduction per
 * MSM.  gm_g16_pk_upload(...) == gm_g16_pk_upload_ex(..., 0, ...). */
#define GM_PK_PRECOMPUTE 1u
/* GM_PK_PRECOMPUTE_AUTO: precompute when the window copies fit the device --
 * the key's precomputed arrays plus the upload's transient buffers take at
 * most GM_PK_PRECOMPUTE_FRAC (default 0.6) of the free device memory at upload
 * time (hipMemGetInfo); otherwise a plain key.  On a 288 GB MI355X a BN254
 * 2^24 key (~77 GB precomputed) qualifies.  gm_g16_pk_precomputed() reports
 * the choice. */
#define GM_PK_PRECOMPUTE_AUTO 2u
int gm_g16_pk_precomputed(const gm_g16_pk* pk, int* out);
int gm_g16_pk_upload_ex(gm_ctx* ctx, int curve, const gm_g16_pk_host* pk, unsigned flags, gm_g16_pk** out);
int gm_g16_pk_free(gm_ctx* ctx, gm_g16_pk* pk);

/* Proves with solved vectors in host memory: wires (nb_wires Fr), a, b, c
 * (nb_constraints Fr each), r and s (one Fr each, Montgomery).  Outputs
 * proof.Ar (G1Affine), proof.Bs (G2Affine), proof.Krs (G1Affine).  The wires
 * are copied first; a, b, c are copied on a separate stream by a helper thread
 * while the A/B/K MSMs run (the icicle.go:204-412 scope, H2D included). */
int gm_g16_prove(gm_ctx* ctx, gm_g16_pk* pk, const void* wires, const void* a, const void* b,
                 const void* c, size_t nb_constraints, const void* r, const void* s,
                 void* ar_out, void* bs_out, void* krs_out);
/* Same with wires/a/b/c already resident on the device (a, b, c buffers hold
 * n elements and are clobbered). */
int gm_g16_prove_device(gm_ctx* ctx, gm_g16_pk* pk, const void* wires_dev, void* a_dev,
                        void* b_dev, void* c_dev, size_t nb_constraints, const void* r,
                        const void* s, void* ar_out, void* bs_out, void* krs_out);

/* ---- R1CS resident on the device: a proof from the wires alone ------------
 * gnark's solver produces solution.A/B/C as <L_i, w>, <R_i, w>, <O_i, w>
 * (constraint/bn254/solver.go:540-620); with the constraint system on the
 * device (uploaded once, like the key) only the wires cross PCIe per proof.
 * Per matrix m in {L, R, O}: rowptr[m] (nb_constraints + 1 entries, from 0),
 * cid[m] / vid[m] (rowptr[m][nb_constraints] terms: coefficient id into
 * `coeffs`, wire id, or GM_R1CS_CONST for a constant term -- constraint.Term,
 * constraint/term.go:31-40); coeffs = the CoeffTable (coeff.go:30-44,
 * ncoeffs fr.Element, Montgomery; ids 0 and 1 must be zero and one).  Ids are
 * validated at upload. */
#define GM_R1CS_CONST 0xFFFFFFFFu
typedef struct gm_r1cs gm_r1cs;
int gm_r1cs_upload(gm_ctx* ctx, int curve, size_t nb_constraints, size_t nb_wires, const uint32_t* const* rowptr,
                   const uint32_t* const* cid, const uint32_t* const* vid, const void* coeffs, size_t ncoeffs,
                   gm_r1cs** out);
int gm_r1cs_free(gm_ctx* ctx, gm_r1cs* r1cs);
/* a_dev, b_dev, c_dev (nb_constraints Fr each) from device-resident wires. */
int gm_r1cs_eval(gm_ctx* ctx, const gm_r1cs* r1cs, const void* wires_dev, void* a_dev, void* b_dev, void* c_dev);
/* gm_g16_prove with the wires as the only host input: wires copied, a / b / c
 * evaluated on the device ahead of computeH while the MSMs run.  The key must
 * be whole (not a shard) and match the constraint system. */
int gm_g16_prove_r1cs(gm_ctx* ctx, gm_g16_pk* pk, const gm_r1cs* r1cs, const void* wires, const void* r,
                      const void* s, void* ar_out, void* bs_out, void* krs_out);

/* ---- sharded Groth16 (BASELINE config 4: G1/G2 MSMs split across the GPUs of
 *      a node, one process per GPU) -------------------------
 * Rank `rank` of `world` uploads only its contiguous slice [lo, hi) of each
 * point array (lo/hi as gnark_mi355x.shard_range: the first n % world ranks
 * hold one extra point) of pk.G1.A (nbA), pk.G1.B and pk.G2.B (nbB), pk.G1.K
 * (nbK) and pk.G1.Z (n - 1).  In `pk` the counts nbA/nbB/nbK and the flags
 * infA/infB/k_wires describe the WHOLE key, while g1_A, g1_B, g1_K, g1_Z and
 * g2_B point at the first point of this rank's slice.  world = 1 is
 * gm_g16_pk_upload_ex. */
int gm_g16_pk_upload_shard(gm_ctx* ctx, int curve, const gm_g16_pk_host* pk, unsigned flags, int rank,
                           int world, gm_g16_pk** out);
/* Size of one partial: 4 G1Jac (sums over A, B, K, Z) + 1 G2Jac (B2). */
int gm_g16_partial_bytes(int curve, size_t* out);
/* computeH over the whole domain (every rank holds the solved a, b, c and the
 * wires), then the five MSMs over this rank's slices: writes the raw sums
 * [sum_A, sum_B, sum_K, sum_Z] (G1Jac) and sum_B2 (G2Jac), no blinding. */
int gm_g16_prove_partial(gm_ctx* ctx, gm_g16_pk* pk, const void* wires_dev, void* a_dev, void* b_dev,
                         void* c_dev, size_t nb_constraints, void* partial_out);
/* Host only: proof elements from the rank-summed partials (same layout) with
 * the blinding of icicle.go:295-391 (alpha, beta, [r]delta, [s]delta,
 * [-rs]delta, [s]Ar, [r]Bs1, [s]delta2, beta2 from `pk`). */
int gm_g16_finish(int curve, const gm_g16_pk_host* pk, const void* sums, const void* r, const void* s,
                  void* ar_out, void* bs_out, void* krs_out);

/* ---- single-process multi-device Groth16 (one gnark process drives every
 *      GPU of the node behind unchanged groth16.Prove call sites,
 *      backend/groth16/groth16.go:192-204) ---------------
 * gm_multi_init creates one context (own streams) per entry of device_ids
 * (entries may repeat: several contexts on one GPU rehearse the multi-GPU path).
 * gm_g16_pk_upload_multi shards every point array of the key across the
 * devices (device 0, which also runs computeH, takes a smaller share:
 * GM_MULTI_SHARE0, default 0.6 of the others'); each device keeps only the
 * compaction-map slices of its shard and later receives only the wires those
 * slices read.  gm_g16_prove_multi runs one host thread per device: wires
 * slices to every device, a / b / c to device 0 (computeH there, h slices sent
 * to the other devices by peer copies over xGMI), the five partial MSMs
 * everywhere, then host adds of the per-device sums and the finishing of
 * gm_g16_finish.  Output and inputs as gm_g16_prove. */
typedef struct gm_multi gm_multi;
typedef struct gm_g16_pk_multi gm_g16_pk_multi;
int gm_multi_init(const int* device_ids, int count, gm_multi** out);
int gm_multi_destroy(gm_multi* m);
int gm_multi_size(const gm_multi* m, int* count);
int gm_multi_context(gm_multi* m, int index, gm_ctx** out);
int gm_g16_pk_upload_multi(gm_multi* m, int curve, const gm_g16_pk_host* pk, unsigned flags,
                           gm_g16_pk_multi** out);
int gm_g16_pk_free_multi(gm_multi* m, gm_g16_pk_multi* pk);
int gm_g16_prove_multi(gm_multi* m, gm_g16_pk_multi* pk, const void* wires, const void* a, const void* b,
                       const void* c, size_t nb_constraints, const void* r, const void* s, void* ar_out,
                       void* bs_out, void* krs_out);

/* ---- proving-key I/O --------------------------------
 * gnark's ProvingKey.WriteDump (backend/groth16/bn254/marshal.go:389-456)
 * writes, after its header (unsafe marker, Domain, the raw-encoded alpha /
 * beta / delta, nbWires, NbInfinityA/B, InfinityA/B, nbCommitments), the five
 * point slices G1.A, G1.B, G1.Z, G1.K, G2.B with gnark-crypto's
 * utils/unsafe.WriteSlice: a little-endian uint64 element count followed by
 * the raw G1Affine / G2Affine memory -- this ABI's point layout.
 * gm_g16_pk_upload_dump reads those five slices from `fd` starting at byte
 * `offset` (where ReadDump, marshal.go:511, starts reading them) and streams
 * them into device buffers (pread into pinned buffers; H2D and conversion /
 * GM_PK_PRECOMPUTE precomputation per 64 MiB chunk, overlapped with the
 * reads).  `meta` carries the header fields as in gm_g16_pk_upload; its point
 * pointers are ignored and its nbA / nbB / nbK (and domain_size - 1 for G1.Z)
 * must equal the slice lengths in the file.  *end_offset receives the first
 * byte after G2.B (the commitment keys' slices, marshal.go:532-543, follow).
 * The _shard form reads only rank's slice of every array (as
 * gm_g16_pk_upload_shard).  The file position of fd is not used or moved. */
int gm_g16_pk_upload_dump(gm_ctx* ctx, int curve, const gm_g16_pk_host* meta, int fd, uint64_t offset,
                          unsigned flags, uint64_t* end_offset, gm_g16_pk** out);
int gm_g16_pk_upload_dump_shard(gm_ctx* ctx, int curve, const gm_g16_pk_host* meta, int fd, uint64_t offset,
                                unsigned flags, int rank, int world, uint64_t* end_offset, gm_g16_pk** out);
/* A device-resident key (shard) in its device layout, GM_PK_PRECOMPUTE window
 * copies included, written to `fd` at its current position; load_cache reads
 * one back with no conversion or precomputation (the persisted device form of
 * SURVEY.md §5's checkpoint row). */
int gm_g16_pk_save_cache(gm_ctx* ctx, const gm_g16_pk* pk, int fd);
int gm_g16_pk_load_cache(gm_ctx* ctx, int fd, gm_g16_pk** out);

/* ---- point validation: curve and subgroup checks on the device -----------
 * Every upload entry takes raw Montgomery limbs unchecked, as gnark's
 * UnsafeReadFrom / ReadDump do (backend/groth16/bn254/marshal.go:320-324,
 * :386-389, :458-460); ProvingKey.ReadFrom (:314-318) pays gnark-crypto's
 * IsInSubGroup per point on the CPU.  These entries class every point of a
 * gnark-layout array on the device, one lane per point.  The first class that
 * applies wins:
 *   GM_POINT_OK            the point passes; (0, 0), gnark's affine infinity, is OK
 *                          and is also counted in `infinities`
 *   GM_POINT_NOT_REDUCED   a coordinate (or an Fp2 component) is >= p as stored;
 *                          no arithmetic is done on it; (0, p) is this class
 *   GM_POINT_OFF_CURVE     y^2 != x^3 + b (G2: the twist's b')
 *   GM_POINT_OFF_SUBGROUP  on the curve and [r]P != infinity
 * for every input, by endomorphism equations equivalent to [r]P = infinity
 * (DESIGN.md section 3.9).  All entries return GM_OK when the check ran, whatever
 * it found: the report carries the verdict.  first_bad is the lowest failing
 * index (n if none) and first_class its class.  n = 0 gives a zero report.
 * GM_ERR_INVALID, before any launch: a NULL context, array (with n > 0) or
 * report, g2 outside {0, 1}, a device array that is not 16-byte aligned, a bad
 * fd, an unknown curve id.  Curve ids 0, 1 and 2, except gm_g16_pk_check_dump:
 * ids 0 and 1 (GM_ERR_UNSUPPORTED for 2, like gm_g16_pk_upload_dump). */
enum { GM_POINT_OK = 0, GM_POINT_NOT_REDUCED = 1, GM_POINT_OFF_CURVE = 2, GM_POINT_OFF_SUBGROUP = 3 };
typedef struct {
  uint64_t n, infinities, not_reduced, off_curve, off_subgroup, first_bad /* n if none */;
  uint32_t first_class;
} gm_points_report;
/* points_dev: n gnark affine points on the device (what gm_copy_points_to_device
 * leaves there).  status_dev: NULL, or n bytes on the device that receive each
 * point's class. */
int gm_points_check(gm_ctx* ctx, int curve, int g2, const void* points_dev, size_t n,
                    uint8_t* status_dev /* NULL or n bytes */, gm_points_report* out);
/* The same over host memory, streamed through the pinned chunk ring of the dump
 * loader: nothing stays on the device, so any n works. */
int gm_points_check_host(gm_ctx* ctx, int curve, int g2, const void* points_host, size_t n, gm_points_report* out);
/* Test knob: the chunk of gm_points_check_host, gm_g16_pk_check and
 * gm_g16_pk_check_dump in bytes (0 = the default, 16 MiB; at most 64 MiB, the dump
 * loader's; a chunk holds at least one point). */
int gm_set_points_check_chunk(gm_ctx* ctx, size_t bytes);
/* The ten members of a Groth16 proving key, in report order. */
enum {
  GM_G16_PK_G1_ALPHA = 0, GM_G16_PK_G1_BETA, GM_G16_PK_G1_DELTA, GM_G16_PK_G2_BETA, GM_G16_PK_G2_DELTA,
  GM_G16_PK_G1_A, GM_G16_PK_G1_B, GM_G16_PK_G1_Z, GM_G16_PK_G1_K, GM_G16_PK_G2_B, GM_G16_PK_MEMBERS
};
typedef struct {
  gm_points_report member[GM_G16_PK_MEMBERS];
  int32_t first_bad_member; /* the first member with a failing point, -1 if none */
} gm_g16_pk_report;
/* Checks the points a gm_g16_pk_upload of `pk` would take (counts as there:
 * nbA, nbB, domain_size - 1, nbK, nbB).  Creates no key. */
int gm_g16_pk_check(gm_ctx* ctx, int curve, const gm_g16_pk_host* pk, gm_g16_pk_report* out);
/* Checks the five slices of a WriteDump file the way gm_g16_pk_upload_dump reads
 * them: the same `offset`, the slice lengths checked against `meta`, the same
 * *end_offset (may be NULL).  The reports of the five single points stay zero
 * (the dump's header holds them; check them with gm_points_check_host).  The
 * file is only read; no key is created. */
int gm_g16_pk_check_dump(gm_ctx* ctx, int curve, const gm_g16_pk_host* meta, int fd, uint64_t offset,
                         gm_g16_pk_report* out, uint64_t* end_offset);

/* ---- point encodings: gnark-crypto's compressed and raw records on the device
 * What G1Affine / G2Affine.Bytes, RawBytes and the Encoder behind
 * ProvingKey.WriteTo / WriteRawTo (backend/groth16/bn254/marshal.go:239-311) and
 * kzg.SRS.WriteTo write, decoded and encoded one lane per record (DESIGN.md
 * section 3.10).  A coordinate is 8 * fp_limbs bytes, big-endian, canonical (not
 * Montgomery).  G1: X (GM_ENC_COMPRESSED) or X || Y (GM_ENC_RAW); G2: X.A1 || X.A0
 * or X.A1 || X.A0 || Y.A1 || Y.A0.  The flag is the top bits of the record's
 * first byte:
 *   BN254 (two bits)        00 raw; 10 / 11 compressed, y the smaller / larger of
 *                           {y, -y}; 01 compressed infinity; the raw infinity is
 *                           the all-zero record
 *   BLS12-377 / -381 (three bits; BLS12-381: the ZCash encoding)
 *                           000 raw; 010 raw infinity; 100 / 101 compressed, smaller /
 *                           larger; 110 compressed infinity; 001, 011, 111 invalid
 * "Larger": the canonical value is > (p - 1) / 2; in Fp2 the rule is applied to A1,
 * to A0 when A1 = 0.  An infinity record is zero outside its flag; the all-zero
 * raw record is read as the infinity on every curve.  One call takes one width:
 * a record whose flag belongs to the other width is refused.  The array passed
 * has no length prefix (the Encoder's big-endian u32 count is the caller's).
 *
 * Decoding classes each record, the first class that applies:
 *   GM_POINT_BAD_ENCODING  an invalid flag, a flag of the other width, an
 *                          infinity record with other bits set
 *   GM_POINT_NOT_REDUCED   a coordinate component >= p once the flag is cleared
 *   GM_POINT_NO_ROOT       compressed: x^3 + b has no square root
 *   GM_POINT_OFF_CURVE     raw: y^2 != x^3 + b
 *   GM_POINT_OFF_SUBGROUP  [r]P != infinity
 * GM_DECODE_NO_SUBGROUP_CHECK (gnark's NoSubgroupChecks) skips the last two.  A
 * compressed point with y = 0 is accepted under either flag.  A refused record
 * and an infinity are stored as (0, 0).  The entries return GM_OK when the
 * decode ran, whatever it found: the report carries the verdict (first_bad = n
 * if none).  n = 0 gives a zero report.  GM_ERR_INVALID before any launch: a
 * NULL argument, an unknown encoding or flag, g2 outside {0, 1}, a device
 * pointer that is not 16-byte aligned, overlapping input and output, an unknown
 * curve id.  Curve ids 0, 1 and 2. */
enum { GM_POINT_BAD_ENCODING = 4, GM_POINT_NO_ROOT = 5 };
#define GM_ENC_COMPRESSED 0
#define GM_ENC_RAW 1
/* a bit of its own beside GM_PK_PRECOMPUTE[_AUTO]: the key loader takes both */
#define GM_DECODE_NO_SUBGROUP_CHECK 0x100u
typedef struct {
  uint64_t n, infinities, not_reduced, off_curve, off_subgroup, bad_encoding, no_root, first_bad /* n if none */;
  uint32_t first_class;
} gm_points_decode_report;
/* enc_dev: n records on the device; points_dev receives n gnark affine points
 * (the layout gm_copy_points_to_device leaves there); status_dev: NULL, or n
 * bytes that receive each record's class. */
int gm_points_decode(gm_ctx* ctx, int curve, int g2, int encoding, unsigned flags, const void* enc_dev, size_t n,
                     void* points_dev, uint8_t* status_dev /* NULL or n bytes */, gm_points_decode_report* out);
/* The same over records in host memory, streamed through the pinned chunk ring of
 * the dump loader in the chunks gm_set_points_check_chunk sets (a chunk holds at
 * least one record), so any n works.  The points go to points_dev (device, n
 * points), to points_host (host, n points), or to both; at least one is given. */
int gm_points_decode_host(gm_ctx* ctx, int curve, int g2, int encoding, unsigned flags, const void* enc_host,
                          size_t n, void* points_dev /* or NULL */, void* points_host /* or NULL */,
                          gm_points_decode_report* out);
/* The reverse: n gnark affine points on the device to n records at enc_dev.
 * (0, 0) becomes the infinity record.  A point with a coordinate component >= p
 * is counted in *not_reduced and written as a zero record; nothing else is
 * checked. */
int gm_points_encode(gm_ctx* ctx, int curve, int g2, int encoding, const void* points_dev, size_t n, void* enc_dev,
                     uint64_t* not_reduced);
/* A Groth16 proving key from the stream ProvingKey.WriteTo (GM_ENC_COMPRESSED) or
 * WriteRawTo (GM_ENC_RAW) writes (backend/groth16/bn254/marshal.go:239-311), as
 * gm_g16_pk_upload_dump takes a WriteDump file.  `offset` is the byte after
 * Domain.WriteTo, where G1.Alpha begins.  The members are read in writeTo's
 * order: G1 alpha, beta, delta (single records), G1 A, B, Z, K (slices: a
 * big-endian u32 count, then the records), G2 beta, delta (single records), G2 B
 * (slice).  Slice lengths are checked against `meta` (nbA, nbB, domain_size - 1,
 * nbK, nbB), whose infA / infB / k_wires are used as gm_g16_pk_upload uses them;
 * its point pointers are ignored.  Every slice is streamed through the pinned
 * chunk ring (chunks as gm_set_points_check_chunk sets them), decoded on the
 * device and converted into the key's layout; no decoded array is kept.  The
 * five decoded single points go to singles_out on the host in gnark layout: three
 * G1 points, then two G2 points.  `flags` takes GM_DECODE_NO_SUBGROUP_CHECK and
 * GM_PK_PRECOMPUTE[_AUTO].  The report has one gm_points_decode_report per member
 * in the order of GM_G16_PK_G1_ALPHA... (the enum's order, not the file's).  All
 * four-byte slice lengths are read and compared first; then the members are
 * decoded in the file's order, and decoding stops at the first member with a
 * failing record: no key is created, *pk is NULL, the call returns
 * GM_ERR_INVALID, first_bad_member is that member, the first in the file's order
 * (a bad G1.A is named before a bad G2 beta), and its first_bad / first_class say
 * where; the members behind it in the file report n = 0.  The failing member
 * itself is decoded to its end before its report is read (one read per slice
 * keeps the copies and kernels overlapped), so an early bad record of a long
 * slice costs the whole slice.  A slice whose length differs from `meta`'s is
 * refused with first_bad_member naming it.  A file that ends early is refused the
 * same way: first_bad_member names the member whose bytes are missing, first_bad
 * is the first record of the chunk that could not be read (first_class stays
 * GM_POINT_OK), and gm_last_error names the member and the records.  *end_offset (may be NULL) is the first byte
 * after G2.B, where nbWires follows.  The file position of fd is not used or
 * moved.  Curve ids 0 and 1 (GM_ERR_UNSUPPORTED for 2, like gm_g16_pk_upload_dump). */
typedef struct {
  gm_points_decode_report member[GM_G16_PK_MEMBERS];
  int32_t first_bad_member; /* the first member with a failing record, -1 if none */
} gm_g16_pk_decode_report;
int gm_g16_pk_upload_encoded(gm_ctx* ctx, int curve, const gm_g16_pk_host* meta, int fd, uint64_t offset,
                             int encoding, unsigned flags, void* singles_out, gm_g16_pk_decode_report* report,
                             uint64_t* end_offset, gm_g16_pk** pk);

/* ---- pairing-product checks and batched Groth16 verification ---------------------
 * The optimal ate pairing of gnark-crypto on all three curve ids (DESIGN.md
 * section 3.11): one lane per pair runs the Miller loop, the Miller values of a
 * product are multiplied 16 per lane and launch, and one lane per product runs
 * the final exponentiation.  No entry returns a GT element.
 *
 * gm_pairing_check: n_products products of k pairs each,
 *   ok_out[j] = (prod_{i<k} e(g1[j k + i], g2[j k + i]) == 1)   (1 or 0).
 * The points are gnark affine points and are assumed on the curve and in the
 * subgroup (gm_points_check); a pair with either point at infinity, (0, 0),
 * contributes 1.  The host variant streams the arrays in chunks of whole
 * products and keeps no host pointer; the device variant takes device arrays
 * (16-byte aligned) and writes ok_out on the host.  The workspace of a call
 * grows with k (one Fp12 value per pair of a chunk).
 * GM_ERR_INVALID, before any launch: an unknown curve id ("unknown curve id"), a
 * NULL context or array, k == 0, a misaligned device array, n_products * k not
 * fitting the address space.  n_products == 0: GM_OK with nothing written. */
int gm_pairing_check(gm_ctx* ctx, int curve, const void* g1_host, const void* g2_host, size_t n_products, size_t k,
                     uint8_t* ok_out);
int gm_pairing_check_device(gm_ctx* ctx, int curve, const void* g1_dev, const void* g2_dev, size_t n_products,
                            size_t k, uint8_t* ok_out /* host */);

/* A Groth16 verifying key resident on the device.  The members are gnark affine
 * points in host memory: G1 alpha, G2 beta, gamma, delta, and the nb_k points of
 * G1.K (nb_k = public inputs + 1, the one wire included).  gm_g16_vk_upload runs
 * the point check on every member and refuses the key with GM_ERR_INVALID, naming
 * the member and the class, if one fails; it keeps -alpha, beta, -gamma, -delta
 * and K on the device and no host pointer.  A verifying key with BSB22 commitments
 * (CommitmentKeys, PublicAndCommitmentCommitted) has no field here: such keys are
 * not served.  Free the key before gm_destroy.  GM_ERR_INVALID: an unknown curve
 * id, a NULL argument or member, nb_k == 0. */
typedef struct gm_g16_vk gm_g16_vk;
typedef struct {
  const void *alpha_g1, *beta_g2, *gamma_g2, *delta_g2, *k_g1;
  size_t nb_k;
} gm_g16_vk_host;
int gm_g16_vk_upload(gm_ctx* ctx, int curve, const gm_g16_vk_host* vk, gm_g16_vk** out);
int gm_g16_vk_free(gm_ctx* ctx, gm_g16_vk* vk);
/* m proofs against one key in the same launches.  proofs_host: m records
 * {Ar G1Affine, Bs G2Affine, Krs G1Affine} (gnark's in-memory Proof without
 * commitments); publics_host: m x (nb_k - 1) fr.Elements in gnark Montgomery form
 * (may be NULL when nb_k == 1).  Per proof: Ar, Krs and Bs are classed by the point
 * check as proof.isValid does (backend/groth16/bn254/verify.go:67), kSum = K[0] +
 * sum_j x_j K[j + 1] is computed, and e(Ar, Bs) e(Krs, -delta) e(kSum, -gamma)
 * e(-alpha, beta) == 1 is checked: four Miller lanes and one final exponentiation.
 * status_out[i]: GM_G16_VERIFY_OK, _BAD_POINT (a proof point failed the point
 * check), _MISMATCH (the pairing equation fails) or _BAD_INPUT (a public input's
 * words are not below r); the first that applies in the order BAD_POINT,
 * BAD_INPUT, MISMATCH.  *nb_ok (may be NULL) counts the accepted proofs.  A bad
 * proof never fails the call.  The arrays are streamed in chunks of whole proofs;
 * no host pointer is kept.  GM_ERR_INVALID: a NULL context, key, array or
 * status_out, a key of another context.  m == 0: GM_OK with nothing written. */
enum { GM_G16_VERIFY_OK = 0, GM_G16_VERIFY_BAD_POINT = 1, GM_G16_VERIFY_MISMATCH = 2, GM_G16_VERIFY_BAD_INPUT = 3 };
int gm_g16_verify_batch(gm_ctx* ctx, const gm_g16_vk* vk, const void* proofs_host, const void* publics_host,
                        size_t m, uint8_t* status_out, size_t* nb_ok);

/* ---- KZG and PLONK verification, batched -----------------
 * What gnark's plonk.Verify computes after its transcript (backend/plonk/bn254/
 * verify.go:128-322, with gnark-crypto's kzg.FoldProof and
 * kzg.BatchVerifyMultiPoints), and kzg.Verify, on the pairing above.  The
 * Fiat-Shamir transcript and hash-to-field stay with the caller: challenges and
 * the hashed BSB22 commitments enter as Montgomery fr.Elements.  Every point is a
 * gnark G1Affine or G2Affine, every scalar a Montgomery fr.Element, all in host
 * memory; the arrays are streamed in chunks of whole openings or proofs and no
 * host pointer is kept.  The decisions are gnark's; no intermediate point is
 * returned.  A status byte is, first that applies,
 *   BAD_POINT   a point of the opening or proof failed the point check,
 *   BAD_INPUT   an Fr word string is not below r, or a multiplier that must not
 *               be zero is (u; lambda_i for i > 0: a zero drops an opening),
 *   ALGEBRAIC   PLONK only: constLin != ClaimedValues[0], gnark's errAlgebraicRelation,
 *   MISMATCH    the pairing equation fails,
 * else OK, with gm_g16_verify_batch's values.  A bad opening or proof never fails
 * the call.
 *
 * A KZG verifying key: G1 generator, G2[0], G2[1] = [tau] G2.  The upload runs the
 * point check on each and refuses the key with GM_ERR_INVALID, naming the member
 * and the class, if one fails; G, G2[0] and -G2[1] stay on the device.  Free the
 * key before gm_destroy.
 *
 * gm_kzg_verify_batch: m independent openings, opening i = digest C_i, proof H_i,
 * point z_i, claimed value y_i:  status_out[i] from
 *   e(C - [y] G + [z] H, G2[0]) e(H, -G2[1]) == 1
 * (two ladders, two Miller lanes and one final exponentiation per opening);
 * *nb_ok (may be NULL) counts the accepted ones.  openings->lambda is not read.
 * gm_kzg_verify_folded: kzg.BatchVerifyMultiPoints' folded form.  The caller
 * supplies m random lambda_i; lambda_0 is not read and taken as 1, as gnark-crypto
 * does.  One product of two pairs for the batch,
 *   e(sum lambda_i (C_i - [y_i] G + [z_i] H_i), G2[0]) e(sum lambda_i H_i, -G2[1]) == 1,
 * and one byte: status_out[0].  BAD_POINT or BAD_INPUT of any opening is the
 * batch's.
 * GM_ERR_INVALID: a NULL context, key, struct, array or status_out, a key of
 * another context, an unknown curve id.  m == 0: GM_OK with nothing written. */
enum { GM_KZG_VERIFY_OK = 0, GM_KZG_VERIFY_BAD_POINT = 1, GM_KZG_VERIFY_MISMATCH = 2, GM_KZG_VERIFY_BAD_INPUT = 3 };
typedef struct gm_kzg_vk gm_kzg_vk;
typedef struct {
  const void *g1, *g2_0, *g2_1;
} gm_kzg_vk_host;
typedef struct {
  const void* digests; /* m G1Affine */
  const void* proofs;  /* m G1Affine: OpeningProof.H */
  const void* points;  /* m Fr: z */
  const void* values;  /* m Fr: OpeningProof.ClaimedValue */
  const void* lambda;  /* m Fr, the folded form only */
} gm_kzg_openings_host;
int gm_kzg_vk_upload(gm_ctx* ctx, int curve, const gm_kzg_vk_host* vk, gm_kzg_vk** out);
int gm_kzg_vk_free(gm_ctx* ctx, gm_kzg_vk* vk);
int gm_kzg_verify_batch(gm_ctx* ctx, const gm_kzg_vk* vk, const gm_kzg_openings_host* openings, size_t m,
                        uint8_t* status_out, size_t* nb_ok);
int gm_kzg_verify_folded(gm_ctx* ctx, const gm_kzg_vk* vk, const gm_kzg_openings_host* openings, size_t m,
                         uint8_t* status_out /* one byte */);

/* A PLONK verifying key resident on the device: n (a power of two >= 8, the
 * proving key's), nb_public, the digests Ql, Qr, Qm, Qo, Qk, S1, S2, S3, nb_bsb
 * digests Qcp (one array) with commitment_row[j], the absolute rows as
 * gm_plonk_pk_host gives them (gnark's NbPublicVariables +
 * CommitmentConstraintIndexes[j]), and the three KZG members.  The upload runs
 * the point check on every point and refuses the key naming the member and the
 * class; it derives 1 / n, the generator w of the domain, the coset shift
 * (FrMultiplicativeGen) and w^row[j] once and keeps -G2[1].  Free the key before
 * gm_destroy.  GM_ERR_INVALID, with a message and nothing left allocated: a NULL
 * argument or member, an unknown curve id, n not a power of two or < 8 or beyond
 * the field's two-adicity, nb_public > n, nb_bsb > 1024, nb_bsb > 0 with a NULL
 * qcp or commitment_row, a commitment_row >= n. */
typedef struct gm_plonk_vk gm_plonk_vk;
typedef struct {
  size_t n, nb_public;
  const void *ql, *qr, *qm, *qo, *qk, *s1, *s2, *s3; /* one G1Affine each */
  size_t nb_bsb;
  const void* qcp;              /* nb_bsb G1Affine */
  const size_t* commitment_row; /* nb_bsb */
  const void *kzg_g1, *kzg_g2_0, *kzg_g2_1;
} gm_plonk_vk_host;
int gm_plonk_vk_upload(gm_ctx* ctx, int curve, const gm_plonk_vk_host* vk, gm_plonk_vk** out);
int gm_plonk_vk_free(gm_ctx* ctx, gm_plonk_vk* vk);
/* m proofs against one key in the same launches.  Per proof,
 *   points      9 + nb_bsb G1Affine: L, R, O, Z, H0, H1, H2, BatchedProof.H,
 *               ZShiftedOpening.H, Bsb22Commitments[j];
 *   values      7 + nb_bsb Fr: BatchedProof.ClaimedValues in polysToOpen order (lin,
 *               l, r, o, s1, s2, qcp_j), then ZShiftedOpening.ClaimedValue: the order
 *               gm_plonk_session_round4 returns them;
 *   publics     nb_public Fr (may be NULL when nb_public == 0);
 *   hashed_cmt  nb_bsb Fr, the caller's hash-to-field of each Bsb22 commitment (may
 *               be NULL when nb_bsb == 0);
 *   challenges  6 Fr: gamma, beta, alpha, zeta, v (FoldProof's folding challenge) and
 *               u (the random multiplier of the second opening in
 *               BatchVerifyMultiPoints; u = 0 is BAD_INPUT);
 * each array holding the m proofs' parts one after the other.  Per proof one lane
 * computes zeta^n, L1(zeta), PI(zeta) (the nb_public + nb_bsb + 1 denominators
 * inverted together, zeros left zero), constLin and the 18 + 2 nb_bsb scalars;
 * one lane per (proof, scalar) runs a double-and-add ladder; one lane per proof
 * adds the terms into A and B = Hb + [u] Hz, and e(A, G2[0]) e(B, -G2[1]) == 1 is
 * checked with two Miller lanes and one final exponentiation.  status_out[i] is
 * GM_PLONK_VERIFY_*; *nb_ok (may be NULL) counts the accepted proofs.  The
 * workspace of a call grows with nb_public (one Fr per proof of a chunk and
 * denominator).  GM_ERR_INVALID: a NULL context, key, struct, required array or
 * status_out, a key of another context.  m == 0: GM_OK with nothing written. */
enum {
  GM_PLONK_VERIFY_OK = 0,
  GM_PLONK_VERIFY_BAD_POINT = 1,
  GM_PLONK_VERIFY_MISMATCH = 2,
  GM_PLONK_VERIFY_BAD_INPUT = 3,
  GM_PLONK_VERIFY_ALGEBRAIC = 4
};
typedef struct {
  const void *points, *values, *publics, *hashed_cmt, *challenges;
} gm_plonk_proofs_host;
int gm_plonk_verify_batch(gm_ctx* ctx, const gm_plonk_vk* vk, const gm_plonk_proofs_host* proofs, size_t m,
                          uint8_t* status_out, size_t* nb_ok);

/* ---- staged prover inputs --------------------------
 * The R1CS solver (constraint/bn254/solver.go:426-532) makes a, b, c final
 * level by level.  Each level (or range) can be handed over as soon as it is
 * solved: every put copies its host data into a pinned ring before it returns
 * (no host pointer is kept) and queues the copy to the device on the
 * context's copy stream, so the H2D overlaps the rest of Solve.
 * gm_g16_stage_prove waits for the queued copies and proves from the
 * device-resident inputs (gm_g16_prove_device).  Every element of a, b, c
 * [0, nb_constraints) and of the wires [0, nb_wires) must have been put; the
 * prove consumes a, b, c (one proof per stage).  gm_g16_stage_free keeps the
 * stage's device vectors and pinned ring with the key (one spare per key,
 * released by gm_g16_pk_free), and the next gm_g16_stage_begin on the same
 * context reuses them: no allocation per proof (GM_G16_STAGE_REUSE=0: off).
 * Indexed puts are gathered as records (element id, vector, value) in the open
 * ring slot and queued when it holds 65,536 of them, when it is full, before a
 * range put and before the prove: a put of one element (a solver level that
 * solved one wire) costs its 40-byte record, not a copy and a launch. */
typedef struct gm_g16_stage gm_g16_stage;
#define GM_STAGE_A 0
#define GM_STAGE_B 1
#define GM_STAGE_C 2
#define GM_STAGE_WIRES 3
int gm_g16_stage_begin(gm_ctx* ctx, gm_g16_pk* pk, size_t nb_constraints, gm_g16_stage** out);
/* elements [lo, lo + count) of vector `which`; host_src points at element lo */
int gm_g16_stage_put_range(gm_g16_stage* st, int which, size_t lo, size_t count, const void* host_src);
/* elements idx[0..k) of vector `which` (one solver level), read from host_base[idx[j]] */
int gm_g16_stage_put_indexed(gm_g16_stage* st, int which, const void* host_base, const uint32_t* idx, size_t k);
int gm_g16_stage_prove(gm_g16_stage* st, const void* r, const void* s, void* ar_out, void* bs_out,
                       void* krs_out);
/* The wires-only staged proof of a resident constraint system: the wires were
 * put during Solve (GM_STAGE_WIRES, e.g. per solver level), a, b, c come from
 * the device R1CS (gm_r1cs_upload) -- nothing crosses PCIe after Solve.  The
 * stage's a / b / c need not be put (they receive the evaluation). */
int gm_g16_stage_prove_r1cs(gm_g16_stage* st, const gm_r1cs* r1cs, const void* r, const void* s, void* ar_out,
                            void* bs_out, void* krs_out);
int gm_g16_stage_free(gm_g16_stage* st);

/* ---- host-side group helpers (finishing adds of sharded MSMs) ---------- */
/* out = p + q, all gnark Jacobian (G1Jac or G2Jac). */
int gm_jac_add(int curve, int g2, const void* p, const void* q, void* out);
/* affine_out = p in affine form. */
int gm_jac_to_affine(int curve, int g2, const void* p, void* affine_out);

/* ---- Groth16 setup: fixed-base batch scalar multiplication ---------------------
 * gnark-crypto's curve.BatchScalarMultiplicationG1/G2, what Setup turns its
 * scalar vectors into points with (backend/groth16/bn254/setup.go:239-275, 318-330):
 *   out[i] = [k_i] base
 * The contract and the bytes are gm_batch_mul_base's: scalars_dev holds n
 * Montgomery fr.Elements, fully reduced, on the device; out_dev receives n gnark
 * affine points, fully reduced; infinity (k_i = 0, or base = (0,0)) is (0,0).
 * Exactly n points are written.
 *
 * A window table T[w][d-1] = [d 2^(c w)] base, 1 <= d <= 2^(c-1), over the
 * W = ceil((r bits + 1) / c) signed-digit windows of the scalar is built in the
 * context's workspace for the call; every scalar then costs W mixed additions
 * of gathered entries and no doubling, and the affine conversion shares one
 * inversion per block of lanes.  c comes from a cost model in n (n W additions
 * against W 2^(c-1) table entries), at most 16: the table is then 32 MiB for
 * BN254 G1 and 96 MiB for BLS12-377 G2.  gm_set_fixed_base_window forces c in
 * [2, 16] for tests and sweeps (0 = the model); the results do not depend on it.
 * GM_ERR_INVALID: a NULL argument, an unknown curve, c out of range,
 * n >= 2^32. */
int gm_set_fixed_base_window(gm_ctx* ctx, int c);
int gm_batch_mul_fixed(gm_ctx* ctx, int curve, int g2, const void* base_affine_host,
                       const void* scalars_dev, size_t n, void* out_dev);

/* ---- Groth16 setup: the scalar side and the key's points -------------------------
 * What gnark's Setup computes between sampling the toxic waste and returning the
 * keys (backend/groth16/bn254/setup.go:120-330, setupABC :364-445), from the
 * resident constraint system (gm_r1cs_upload):
 *   L_j(t) = w^j (t^n - 1) / (n (t - w^j)) for every constraint j (n = the domain:
 *       the next power of two >= nb_constraints),
 *   A_w = sum over the terms of L with wire w of coeff L_row(t); B_w over R, C_w over O,
 *   InfinityA / InfinityB = exact zero tests of A_w / B_w; A, B (G1) and B (G2)
 *       hold the non-zero ones in wire order,
 *   K_w = (beta A_w + alpha B_w + C_w) / delta for the key's wires, / gamma for the
 *       verifier's side: the public wires and the wires of gamma_wires (gnark's
 *       commitment wires and private committed wires, setup.go:164-195),
 *   Z_i = t^i (t^n - 1) / delta, bit-reversed, n - 1 of them,
 * and every vector multiplied into its group by gm_batch_mul_fixed's kernels.
 * The caller samples the toxic scalars (the library holds no random source) and
 * keeps what Setup does beyond this: the Pedersen keys, vk.e, the pairing
 * precomputation.
 *
 * gm_g16_setup_sizes runs the scalar side only and returns the counts the caller
 * sizes gm_g16_setup's host buffers with: nbA and nbB points (g1_A; g1_B and
 * g2_B), nbK (g1_K, k_wires); g1_Z holds n - 1 points, g1_K_gamma nb_public +
 * nb_gamma, infA / infB nb_wires bytes.  A NULL member of gm_g16_setup_out is
 * skipped.  GM_ERR_INVALID, judged on the host before any launch and named in
 * gm_last_error: a NULL argument; nb_public > nb_wires; gamma_wires not strictly
 * increasing inside [nb_public, nb_wires); delta = 0 or gamma = 0; t^n = 1 (the
 * formula divides by zero); an R1CS with a constant term (GM_R1CS_CONST), which
 * gnark's never has; more than 2^25 wires or constraints.
 * gm_set_g16_setup_column_cut: the column length above which a column's sum is
 * split over several blocks (0 = the default, 2^14); tests only. */
typedef struct {
  const void* toxic;                 /* host, 5 Fr Montgomery: t, alpha, beta, gamma, delta */
  size_t nb_public;
  const uint32_t* gamma_wires;       /* or NULL */
  size_t nb_gamma;
} gm_g16_setup_in;

typedef struct {
  /* host buffers sized by the caller from gm_g16_setup_sizes */
  void *g1_alpha, *g1_beta, *g1_delta;
  void *g1_A, *g1_B, *g1_Z, *g1_K;
  void* g1_K_gamma;                  /* public wires, then gamma_wires, in wire order */
  void *g2_beta, *g2_delta, *g2_gamma, *g2_B;
  uint8_t *infA, *infB;
  uint32_t* k_wires;                 /* nbK */
} gm_g16_setup_out;

int gm_set_g16_setup_column_cut(gm_ctx* ctx, int t);
int gm_g16_setup_sizes(gm_ctx* ctx, const gm_r1cs* r1cs, const gm_g16_setup_in* in,
                       size_t* nbA, size_t* nbB, size_t* nbK);
int gm_g16_setup(gm_ctx* ctx, const gm_r1cs* r1cs, const gm_g16_setup_in* in,
                 const gm_g16_setup_out* out);
/* The resident proving key from the same derivation: the derived device arrays go
 * through gm_g16_pk_upload_ex's own conversion (flags as there) without a trip
 * through host memory, so the key is the object that entry makes from the arrays
 * gm_g16_setup returns: same proofs, same gm_g16_pk_precomputed.  With host_copy
 * non-NULL its non-NULL members also receive the arrays, as gm_g16_setup's do.  No
 * host pointer is kept.  Refused as gm_g16_setup, and for unknown flags or fewer
 * than two constraints. */
int gm_g16_pk_setup(gm_ctx* ctx, const gm_r1cs* r1cs, const gm_g16_setup_in* in, unsigned flags,
                    gm_g16_pk** out, const gm_g16_setup_out* host_copy /* or NULL */);

/* ---- synthetic inputs (bench / tests; not on the hot path) ------------
 * out[i] = [k_i] base, k_i = Montgomery fr.Elements on the device, outputs
 * affine points on the device (curve.BatchScalarMultiplicationG1/G2). */
int gm_batch_mul_base(gm_ctx* ctx, int curve, int g2, const void* base_affine_host,
                      const void* scalars_dev, size_t n, void* points_out_dev);
/* Fills n Montgomery Fr elements uniform in [0, r) from a seed (device). */
int gm_random_scalars(gm_ctx* ctx, int curve, uint64_t seed, size_t n, void* scalars_dev);
/* Generator points of the curve in gnark affine layout (host). */
int gm_generator(int curve, int g2, void* affine_out);

/* Element-wise test hooks of the device field / curve layer live in a separate
 * test-only library (include/gnark_mi355x_testhooks.h,
 * libgnark_mi355x_testhooks.so); the product library does not export them. */

#ifdef __cplusplus
}
#endif
#endif /* GNARK_MI355X_H */
