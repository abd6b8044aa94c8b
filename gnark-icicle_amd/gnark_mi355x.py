"""Python binding of libgnark_mi355x.so (ctypes) -- host plumbing for tests and
bench.py.  The product is the C-ABI in include/gnark_mi355x.h; this module only
mirrors it, keeping iciclegnark's operation names
(backend/groth16/bn254/icicle/icicle.go call sites) so tests read like the
reference's own flow:

    CopyToDevice          -> copy_to_device            (icicle.go:44,47,65,245,269,352,478-480)
    CopyPointsToDevice    -> copy_points_to_device     (icicle.go:90,95,109,114)
    CopyG2PointsToDevice  -> copy_points_to_device(g2=True)  (icicle.go:125)
    GenerateTwiddleFactors-> generate_twiddle_factors  (icicle.go:68,73)
    INttOnDevice          -> intt_on_device            (icicle.go:489,502)
    NttOnDevice           -> ntt_on_device             (icicle.go:490)
    PolyOps               -> poly_ops                  (icicle.go:500)
    ReverseScalars        -> reverse_scalars           (icicle.go:510)
    MsmOnDevice           -> msm_on_device             (icicle.go:302,315,332,355)
    MsmG2OnDevice         -> msm_g2_on_device          (icicle.go:382)
    FreeDevicePointer     -> free_device_pointer       (icicle.go:356,416-418,492,505-507)
    icicle_bn254.Prove    -> ProvingKey.prove          (icicle.go:133-422)

There is NO fallback: if the shared library is missing or no GPU is visible the
calls raise.
"""
from __future__ import annotations

import ctypes
import os
import struct

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
# GNARK_MI355X_LIB: an alternative build of the same library (same-box A/B runs)
LIB_PATH = os.environ.get("GNARK_MI355X_LIB") or os.path.join(HERE, "libgnark_mi355x.so")

BN254, BLS12_377, BLS12_381 = 0, 1, 2
CURVES = {"bn254": BN254, "bls12377": BLS12_377, "bls12381": BLS12_381}
FP_BYTES = {BN254: 32, BLS12_377: 48, BLS12_381: 48}
FR_BYTES = 32

# exported symbols (include/gnark_mi355x.h) -- checked by tests/test_capi_symbols.py
SYMBOLS = [
    "gm_last_error", "gm_version", "gm_init", "gm_destroy", "gm_synchronize", "gm_trim",
    "gm_profile_enable", "gm_profile_reset", "gm_profile_get", "gm_profile_dump",
    "gm_set_msm_window", "gm_set_msm_glv", "gm_set_msm_piece_len", "gm_malloc", "gm_free", "gm_copy_to_device", "gm_memcpy_h2d",
    "gm_memcpy_d2h", "gm_memcpy_d2d", "gm_copy_points_to_device", "gm_msm", "gm_msm_host_scalars", "gm_points_upload", "gm_msm_prepared", "gm_precompute_layout", "gm_points_upload_precomputed",
    "gm_msm_precomputed", "gm_kzg_commit", "gm_kzg_eval", "gm_poly_div_linear", "gm_poly_fold", "gm_kzg_open",
    "gm_kzg_batch_open", "gm_plonk_quotient", "gm_plonk_perm_z", "gm_plonk_linearize", "gm_ntt",
    "gm_poly_ops", "gm_reverse_scalars", "gm_groth16_compute_h", "gm_g16_pk_upload", "gm_g16_pk_upload_ex", "gm_g16_pk_upload_shard",
    "gm_g16_partial_bytes", "gm_g16_prove_partial", "gm_g16_finish",
    "gm_g16_pk_free", "gm_g16_pk_precomputed", "gm_g16_prove", "gm_g16_prove_device", "gm_jac_add", "gm_jac_to_affine",
    "gm_batch_mul_base", "gm_random_scalars", "gm_generator", "gm_icicle_generate_twiddles", "gm_icicle_intt_on_device", "gm_icicle_ntt_on_device",
    "gm_icicle_poly_ops", "gm_device_count", "gm_multi_init", "gm_multi_destroy", "gm_multi_size",
    "gm_multi_context", "gm_g16_pk_upload_multi", "gm_g16_pk_free_multi", "gm_g16_prove_multi",
    "gm_g16_pk_upload_dump", "gm_g16_pk_upload_dump_shard", "gm_g16_pk_save_cache", "gm_g16_pk_load_cache",
    "gm_g16_stage_begin", "gm_g16_stage_put_range", "gm_g16_stage_put_indexed", "gm_g16_stage_prove",
    "gm_g16_stage_free", "gm_msm_async", "gm_msm_wait", "gm_r1cs_upload", "gm_r1cs_free", "gm_r1cs_eval",
    "gm_g16_prove_r1cs", "gm_g16_stage_prove_r1cs",
    "gm_plonk_pk_upload", "gm_plonk_pk_bytes", "gm_plonk_pk_free", "gm_plonk_session_begin",
    "gm_plonk_session_bsb22", "gm_plonk_session_round1", "gm_plonk_session_round2", "gm_plonk_session_round3",
    "gm_plonk_session_round4", "gm_plonk_session_round5", "gm_plonk_session_free",
    "gm_plonk_wires_upload", "gm_plonk_wires_bytes", "gm_plonk_wires_free", "gm_plonk_gather_lro",
    "gm_plonk_session_round1_witness", "gm_plonk_session_bsb22_sparse",
    "gm_kzg_srs_lagrange", "gm_plonk_sigma", "gm_plonk_pk_setup",
    "gm_plonk_wires_permutation", "gm_plonk_sigma_wires", "gm_plonk_pk_setup_wires",
    "gm_plonk_scs_upload", "gm_plonk_scs_bytes", "gm_plonk_scs_free", "gm_plonk_scs_wires",
    "gm_plonk_scs_selector", "gm_plonk_pk_setup_scs", "gm_plonk_scs_check",
    "gm_set_fixed_base_window", "gm_batch_mul_fixed",
    "gm_set_g16_setup_column_cut", "gm_g16_setup_sizes", "gm_g16_setup", "gm_g16_pk_setup",
    "gm_points_check", "gm_points_check_host", "gm_set_points_check_chunk", "gm_g16_pk_check",
    "gm_g16_pk_check_dump",
    "gm_points_decode", "gm_points_decode_host", "gm_points_encode", "gm_g16_pk_upload_encoded",
    "gm_pairing_check", "gm_pairing_check_device", "gm_g16_vk_upload", "gm_g16_vk_free", "gm_g16_verify_batch",
    "gm_kzg_vk_upload", "gm_kzg_vk_free", "gm_kzg_verify_batch", "gm_kzg_verify_folded", "gm_plonk_vk_upload",
    "gm_plonk_vk_free", "gm_plonk_verify_batch",
]
# test-only library (include/gnark_mi355x_testhooks.h, libgnark_mi355x_testhooks.so)
TEST_SYMBOLS = ["gm_test_field_op", "gm_test_point_op", "gm_test_stage_replay_chain",
                "gm_test_msm_g2_keyless_plan", "gm_test_field_raw_op", "gm_test_point_raw_op",
                "gm_test_msm_geometry", "gm_test_scan", "gm_test_fe_sqrt", "gm_test_pairing_op",
                "gm_test_plonk_verify_scalars", "gm_test_plonk_verify_chunked", "gm_test_kzg_verify_chunked"]
TESTHOOKS_PATH = os.path.join(os.path.dirname(LIB_PATH), "libgnark_mi355x_testhooks.so")


class GmError(RuntimeError):
    pass


PLONK_POLYS = ("ql", "qr", "qm", "qo", "qk", "s1", "s2", "s3", "l", "r", "o", "z")


class _PlonkQuotientIn(ctypes.Structure):
    """gm_plonk_quotient_in (include/gnark_mi355x.h)."""
    _fields_ = ([("n", ctypes.c_size_t)] + [(k, ctypes.c_void_p) for k in PLONK_POLYS]
                + [("nb_bsb", ctypes.c_size_t), ("qcp", ctypes.POINTER(ctypes.c_void_p)),
                   ("pi2", ctypes.POINTER(ctypes.c_void_p))]
                + [(k, ctypes.c_void_p) for k in ("bl", "br", "bo", "bz", "alpha", "beta", "gamma")])


PLONK_PERM_POLYS = ("l", "r", "o", "s1", "s2", "s3")
# geometry of the scan behind gm_plonk_perm_z (csrc/plonk_perm.hpp): rows per
# thread run, rows per chunk, chunks per tile of the carry scan
PLONK_PERM_E, PLONK_PERM_CHUNK, PLONK_PERM_CARRY_TILE = 4, 512, 64


class _PlonkPermIn(ctypes.Structure):
    """gm_plonk_perm_in (include/gnark_mi355x.h)."""
    _fields_ = ([("n", ctypes.c_size_t)] + [(k, ctypes.c_void_p) for k in PLONK_PERM_POLYS]
                + [("beta", ctypes.c_void_p), ("gamma", ctypes.c_void_p)])


# geometry of the combination pass behind gm_plonk_linearize (csrc/plonk_lin.hpp):
# coefficients per block; a lane owns one coefficient and the grid is not capped
PLONK_LIN_BLOCK = 256
PLONK_LIN_BLINDED = ("l_blinded", "r_blinded", "o_blinded", "z_blinded")


class _PlonkLinearizeIn(ctypes.Structure):
    """gm_plonk_linearize_in (include/gnark_mi355x.h)."""
    _fields_ = ([("n", ctypes.c_size_t)] + [(k, ctypes.c_void_p) for k in PLONK_POLYS]
                + [("nb_bsb", ctypes.c_size_t), ("qcp", ctypes.POINTER(ctypes.c_void_p)),
                   ("pi2", ctypes.POINTER(ctypes.c_void_p))]
                + [(k, ctypes.c_void_p) for k in ("bl", "br", "bo", "bz", "h", "h_rand", "alpha", "beta", "gamma",
                                                  "zeta")])


class _PlonkLinearizeOut(ctypes.Structure):
    """gm_plonk_linearize_out (include/gnark_mi355x.h)."""
    _fields_ = [(k, ctypes.c_void_p) for k in ("lin",) + PLONK_LIN_BLINDED + ("evals",)]


PLONK_PK_POLYS = ("ql", "qr", "qm", "qo", "qk", "s1", "s2", "s3")
PLONK_PK_NO_COSET_CACHE = 1
PLONK_PK_LIN_KEY_QK = 4


class _PlonkPkHost(ctypes.Structure):
    """gm_plonk_pk_host (include/gnark_mi355x.h)."""
    _fields_ = ([("n", ctypes.c_size_t), ("nb_public", ctypes.c_size_t)]
                + [(k, ctypes.c_void_p) for k in PLONK_PK_POLYS]
                + [("nb_bsb", ctypes.c_size_t), ("qcp", ctypes.POINTER(ctypes.c_void_p)),
                   ("commitment_row", ctypes.POINTER(ctypes.c_size_t)), ("srs_canonical", ctypes.c_void_p),
                   ("srs_canonical_len", ctypes.c_size_t), ("srs_lagrange", ctypes.c_void_p)])


PLONK_SETUP_POLYS = ("ql", "qr", "qm", "qo", "qk")


class _PlonkSetupHost(ctypes.Structure):
    """gm_plonk_setup_host (include/gnark_mi355x.h)."""
    _fields_ = ([("n", ctypes.c_size_t), ("nb_public", ctypes.c_size_t)]
                + [(k, ctypes.c_void_p) for k in PLONK_SETUP_POLYS]
                + [("permutation", ctypes.POINTER(ctypes.c_int64)),
                   ("nb_bsb", ctypes.c_size_t), ("qcp", ctypes.POINTER(ctypes.c_void_p)),
                   ("commitment_row", ctypes.POINTER(ctypes.c_size_t)), ("srs_canonical", ctypes.c_void_p),
                   ("srs_canonical_len", ctypes.c_size_t)])


class _PlonkScsHost(ctypes.Structure):
    """gm_plonk_scs_host (include/gnark_mi355x.h)."""
    _fields_ = [("n", ctypes.c_size_t), ("nb_public", ctypes.c_size_t), ("nb_constraints", ctypes.c_size_t),
                ("nb_wires", ctypes.c_size_t), ("records", ctypes.POINTER(ctypes.c_uint32)),
                ("coeffs", ctypes.c_void_p), ("ncoeffs", ctypes.c_size_t), ("nb_bsb", ctypes.c_size_t),
                ("committed", ctypes.POINTER(ctypes.POINTER(ctypes.c_uint32))),
                ("committed_len", ctypes.POINTER(ctypes.c_size_t)),
                ("commitment_index", ctypes.POINTER(ctypes.c_size_t))]


# columns of gm_plonk_scs_selector; SCS_QCP0 + j is qcp_j
SCS_QL, SCS_QR, SCS_QM, SCS_QO, SCS_QK, SCS_QCP0 = range(6)
SCS_RECORD_WORDS = 9  # XA XB XC QL QR QO QM QC Commitment


PLONK_ROUND1_FIELDS = ("l", "r", "o", "public_inputs", "commitment_vals", "bl", "br", "bo", "bz", "h_rand")


class _PlonkRound1In(ctypes.Structure):
    """gm_plonk_round1_in (include/gnark_mi355x.h)."""
    _fields_ = [(k, ctypes.c_void_p) for k in PLONK_ROUND1_FIELDS]


PLONK_ROUND1_WITNESS_FIELDS = ("witness", "commitment_vals", "bl", "br", "bo", "bz", "h_rand")


class _PlonkRound1WitnessIn(ctypes.Structure):
    """gm_plonk_round1_witness_in (include/gnark_mi355x.h)."""
    _fields_ = [(k, ctypes.c_void_p) for k in PLONK_ROUND1_WITNESS_FIELDS]


G16_SETUP_OUT_FIELDS = ("g1_alpha", "g1_beta", "g1_delta", "g1_A", "g1_B", "g1_Z", "g1_K", "g1_K_gamma",
                        "g2_beta", "g2_delta", "g2_gamma", "g2_B", "infA", "infB", "k_wires")


class _G16SetupIn(ctypes.Structure):
    """gm_g16_setup_in (include/gnark_mi355x.h)."""
    _fields_ = [("toxic", ctypes.c_void_p), ("nb_public", ctypes.c_size_t),
                ("gamma_wires", ctypes.POINTER(ctypes.c_uint32)), ("nb_gamma", ctypes.c_size_t)]


class _G16SetupOut(ctypes.Structure):
    """gm_g16_setup_out (include/gnark_mi355x.h)."""
    _fields_ = [(k, ctypes.c_void_p) for k in G16_SETUP_OUT_FIELDS]


# gm_test_msm_geometry layouts (include/gnark_mi355x_testhooks.h)
TGEOM_PLAIN, TGEOM_GLV, TGEOM_PRECOMP, TGEOM_DEFAULT = 0, 1, 2, 3
# point validation (gm_points_check*): the class of a point, the first that applies
POINT_OK, POINT_NOT_REDUCED, POINT_OFF_CURVE, POINT_OFF_SUBGROUP = 0, 1, 2, 3
# the members of a Groth16 key in gm_g16_pk_report order
G16_PK_MEMBERS = ("g1_alpha", "g1_beta", "g1_delta", "g2_beta", "g2_delta", "g1_A", "g1_B", "g1_Z", "g1_K", "g2_B")


class _PointsReport(ctypes.Structure):
    _fields_ = [(k, ctypes.c_uint64) for k in ("n", "infinities", "not_reduced", "off_curve", "off_subgroup",
                                               "first_bad")] + [("first_class", ctypes.c_uint32)]

    def as_dict(self) -> dict:
        return {k: int(getattr(self, k)) for k, _ in self._fields_}


# point encodings (gm_points_decode*, gm_points_encode): the two further classes of a
# record, the widths and the decode flag
POINT_BAD_ENCODING, POINT_NO_ROOT = 4, 5
ENC_COMPRESSED, ENC_RAW = 0, 1
DECODE_NO_SUBGROUP_CHECK = 0x100


class _PointsDecodeReport(ctypes.Structure):
    """gm_points_decode_report (include/gnark_mi355x.h)."""
    _fields_ = [(k, ctypes.c_uint64) for k in ("n", "infinities", "not_reduced", "off_curve", "off_subgroup",
                                               "bad_encoding", "no_root", "first_bad")] + [("first_class",
                                                                                            ctypes.c_uint32)]

    def as_dict(self) -> dict:
        return {k: int(getattr(self, k)) for k, _ in self._fields_}


class _G16PkDecodeReport(ctypes.Structure):
    """gm_g16_pk_decode_report (include/gnark_mi355x.h)."""
    _fields_ = [("member", _PointsDecodeReport * len(G16_PK_MEMBERS)), ("first_bad_member", ctypes.c_int32)]

    def as_dict(self) -> dict:
        out = {name: self.member[i].as_dict() for i, name in enumerate(G16_PK_MEMBERS)}
        out["first_bad_member"] = None if self.first_bad_member < 0 else G16_PK_MEMBERS[self.first_bad_member]
        return out


class _G16PkReport(ctypes.Structure):
    _fields_ = [("member", _PointsReport * len(G16_PK_MEMBERS)), ("first_bad_member", ctypes.c_int32)]

    def as_dict(self) -> dict:
        out = {name: self.member[i].as_dict() for i, name in enumerate(G16_PK_MEMBERS)}
        out["first_bad_member"] = None if self.first_bad_member < 0 else G16_PK_MEMBERS[self.first_bad_member]
        return out


TGEOM_MAX_LEVELS = 24
# lanes per block of gm_test_fe_sqrt's kernel (csrc/testhooks.hip fe_sqrt_t): element i
# runs in lane i % 64 of block i // 64, one wave per block
FE_SQRT_HOOK_BLOCK = 64


class _G16VkHost(ctypes.Structure):
    _fields_ = [("alpha_g1", ctypes.c_void_p), ("beta_g2", ctypes.c_void_p), ("gamma_g2", ctypes.c_void_p),
                ("delta_g2", ctypes.c_void_p), ("k_g1", ctypes.c_void_p), ("nb_k", ctypes.c_size_t)]


# gm_test_pairing_op ops; gm_g16_verify_batch status bytes
(TPAIR_MUL, TPAIR_SQR, TPAIR_INV, TPAIR_CONJ, TPAIR_FROB1, TPAIR_FROB2, TPAIR_CYC_SQR, TPAIR_LINE_MUL, TPAIR_EXP_U,
 TPAIR_MILLER, TPAIR_FINAL_EXP) = range(11)
G16_VERIFY_OK, G16_VERIFY_BAD_POINT, G16_VERIFY_MISMATCH, G16_VERIFY_BAD_INPUT = 0, 1, 2, 3
# gm_kzg_verify_batch / gm_plonk_verify_batch status bytes
KZG_VERIFY_OK, KZG_VERIFY_BAD_POINT, KZG_VERIFY_MISMATCH, KZG_VERIFY_BAD_INPUT = 0, 1, 2, 3
(PLONK_VERIFY_OK, PLONK_VERIFY_BAD_POINT, PLONK_VERIFY_MISMATCH, PLONK_VERIFY_BAD_INPUT,
 PLONK_VERIFY_ALGEBRAIC) = range(5)


class _KzgVkHost(ctypes.Structure):
    """gm_kzg_vk_host (include/gnark_mi355x.h)."""
    _fields_ = [(k, ctypes.c_void_p) for k in ("g1", "g2_0", "g2_1")]


class _KzgOpeningsHost(ctypes.Structure):
    """gm_kzg_openings_host."""
    _fields_ = [(k, ctypes.c_void_p) for k in ("digests", "proofs", "points", "values", "lambda_")]


class _PlonkVkHost(ctypes.Structure):
    """gm_plonk_vk_host."""
    _fields_ = ([("n", ctypes.c_size_t), ("nb_public", ctypes.c_size_t)]
                + [(k, ctypes.c_void_p) for k in ("ql", "qr", "qm", "qo", "qk", "s1", "s2", "s3")]
                + [("nb_bsb", ctypes.c_size_t), ("qcp", ctypes.c_void_p),
                   ("commitment_row", ctypes.POINTER(ctypes.c_size_t))]
                + [(k, ctypes.c_void_p) for k in ("kzg_g1", "kzg_g2_0", "kzg_g2_1")])


class _PlonkProofsHost(ctypes.Structure):
    """gm_plonk_proofs_host."""
    _fields_ = [(k, ctypes.c_void_p) for k in ("points", "values", "publics", "hashed_cmt", "challenges")]


class _MsmGeom(ctypes.Structure):
    """gm_test_msm_geom (include/gnark_mi355x_testhooks.h)."""
    _fields_ = ([(k, ctypes.c_uint32) for k in ("c", "W", "wn", "narrow", "Wred", "nb", "total", "glv", "shared",
                                                "bits", "F", "G", "NC", "NS", "compact", "piece_len", "L", "nseg",
                                                "levels")]
                + [("lg", ctypes.c_uint32 * TGEOM_MAX_LEVELS), ("Q", ctypes.c_uint32), ("xyzz_bytes", ctypes.c_uint32)]
                + [(k, ctypes.c_uint64) for k in ("n", "M", "npts", "bucket_bytes", "node_bytes", "offset_bytes")])


_lib = None
_testhooks = None


def load_testhooks(path: str = None):
    """The test-only element-wise hooks (parity tests of the field / curve layer);
    loads the product library first (the hooks link against it)."""
    global _testhooks
    if _testhooks is not None:
        return _testhooks
    load_library()
    path = path or TESTHOOKS_PATH
    if not os.path.exists(path):
        raise GmError(f"{path} not built -- run `make -C gnark-icicle_amd`")
    T = ctypes.CDLL(path)
    vp, sz, i = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int
    T.gm_test_field_op.argtypes = [vp, i, i, i, vp, vp, vp, sz]
    T.gm_test_point_op.argtypes = [vp, i, i, i, vp, vp, vp, sz]
    T.gm_test_stage_replay_chain.argtypes = [vp, vp, sz, vp, vp, vp, sz, i, i, sz, ctypes.POINTER(ctypes.c_double)]
    T.gm_test_msm_g2_keyless_plan.argtypes = [vp, i, vp, vp, sz]
    T.gm_test_field_raw_op.argtypes = [vp, i, i, i, i, vp, vp, vp, vp, vp, sz]
    T.gm_test_point_raw_op.argtypes = [vp, i, i, i, i, vp, vp, vp, vp, sz]
    T.gm_test_msm_geometry.argtypes = [i, i, sz, i, i, ctypes.POINTER(_MsmGeom)]
    T.gm_test_scan.argtypes = [vp, i, vp, sz, vp]
    T.gm_test_fe_sqrt.argtypes = [vp, i, i, vp, sz, vp, vp]
    T.gm_test_pairing_op.argtypes = [vp, i, i, vp, vp, sz, vp]
    T.gm_test_plonk_verify_scalars.argtypes = [vp, vp, ctypes.POINTER(_PlonkProofsHost), sz, vp, vp, vp]
    T.gm_test_plonk_verify_chunked.argtypes = [vp, vp, ctypes.POINTER(_PlonkProofsHost), sz, sz, vp,
                                               ctypes.POINTER(sz)]
    T.gm_test_kzg_verify_chunked.argtypes = [vp, vp, ctypes.POINTER(_KzgOpeningsHost), sz, sz, i, vp, ctypes.POINTER(sz)]
    _testhooks = T
    return T


def load_library(path: str = LIB_PATH):
    """Loads the C-ABI library (raises if it has not been built)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(path):
        raise GmError(f"{path} not built -- run `make -C gnark-icicle_amd` (or __graft_entry__.build())")
    L = ctypes.CDLL(path)
    vp, sz, i, u64 = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_uint64
    pvp = ctypes.POINTER(ctypes.c_void_p)
    L.gm_last_error.restype = ctypes.c_char_p
    L.gm_init.argtypes = [i, pvp]
    L.gm_destroy.argtypes = [vp]
    L.gm_synchronize.argtypes = [vp]
    L.gm_trim.argtypes = [vp]
    L.gm_profile_enable.argtypes = [vp, i]
    L.gm_profile_reset.argtypes = [vp]
    L.gm_profile_get.argtypes = [vp, ctypes.c_char_p, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(u64)]
    L.gm_profile_dump.argtypes = [vp, ctypes.c_char_p, sz]
    L.gm_set_msm_window.argtypes = [vp, i]
    L.gm_set_msm_glv.argtypes = [vp, i]
    L.gm_set_msm_piece_len.argtypes = [vp, i]
    L.gm_malloc.argtypes = [vp, sz, pvp]
    L.gm_free.argtypes = [vp, vp]
    L.gm_copy_to_device.argtypes = [vp, vp, sz, pvp]
    L.gm_memcpy_h2d.argtypes = [vp, vp, vp, sz]
    L.gm_memcpy_d2h.argtypes = [vp, vp, vp, sz]
    L.gm_memcpy_d2d.argtypes = [vp, vp, vp, sz]
    L.gm_copy_points_to_device.argtypes = [vp, i, i, vp, sz, pvp]
    L.gm_msm.argtypes = [vp, i, i, vp, vp, sz, vp, vp]
    L.gm_msm_host_scalars.argtypes = [vp, i, i, vp, vp, sz, vp, vp]
    L.gm_points_upload.argtypes = [vp, i, i, vp, sz, pvp]
    L.gm_msm_prepared.argtypes = [vp, i, i, vp, vp, sz, vp, vp]
    L.gm_precompute_layout.argtypes = [i, sz, i, ctypes.POINTER(i), ctypes.POINTER(i)]
    L.gm_points_upload_precomputed.argtypes = [vp, i, i, vp, sz, i, pvp]
    L.gm_msm_precomputed.argtypes = [vp, i, i, vp, vp, sz, i, sz, vp, vp]
    L.gm_kzg_commit.argtypes = [vp, i, vp, sz, vp, sz, vp]
    psz = ctypes.POINTER(sz)
    L.gm_kzg_eval.argtypes = [vp, i, pvp, psz, sz, vp, vp]
    L.gm_poly_div_linear.argtypes = [vp, i, vp, sz, vp, vp, vp]
    L.gm_poly_fold.argtypes = [vp, i, pvp, psz, sz, vp, vp]
    L.gm_kzg_open.argtypes = [vp, i, vp, sz, vp, sz, vp, vp, vp]
    L.gm_kzg_batch_open.argtypes = [vp, i, vp, sz, pvp, psz, sz, vp, vp, vp, vp]
    L.gm_plonk_quotient.argtypes = [vp, i, ctypes.POINTER(_PlonkQuotientIn), vp]
    L.gm_plonk_perm_z.argtypes = [vp, i, ctypes.POINTER(_PlonkPermIn), vp, vp]
    L.gm_plonk_linearize.argtypes = [vp, i, ctypes.POINTER(_PlonkLinearizeIn), ctypes.POINTER(_PlonkLinearizeOut)]
    L.gm_ntt.argtypes = [vp, i, vp, sz, i, i, i]
    L.gm_poly_ops.argtypes = [vp, i, vp, vp, vp, sz, vp]
    L.gm_reverse_scalars.argtypes = [vp, i, vp, sz]
    L.gm_groth16_compute_h.argtypes = [vp, i, vp, vp, vp, sz, sz]
    L.gm_g16_pk_upload.argtypes = [vp, i, vp, pvp]
    L.gm_g16_pk_upload_ex.argtypes = [vp, i, vp, ctypes.c_uint, pvp]
    L.gm_g16_pk_upload_shard.argtypes = [vp, i, vp, ctypes.c_uint, i, i, pvp]
    L.gm_g16_partial_bytes.argtypes = [i, ctypes.POINTER(sz)]
    L.gm_g16_prove_partial.argtypes = [vp, vp, vp, vp, vp, vp, sz, vp]
    L.gm_g16_finish.argtypes = [i, vp, vp, vp, vp, vp, vp, vp]
    L.gm_g16_pk_free.argtypes = [vp, vp]
    L.gm_g16_pk_precomputed.argtypes = [vp, ctypes.POINTER(ctypes.c_int)]
    L.gm_g16_prove.argtypes = [vp, vp, vp, vp, vp, vp, sz, vp, vp, vp, vp, vp]
    L.gm_g16_prove_device.argtypes = [vp, vp, vp, vp, vp, vp, sz, vp, vp, vp, vp, vp]
    L.gm_r1cs_upload.argtypes = [vp, i, sz, sz, vp, vp, vp, vp, sz, vp]
    L.gm_r1cs_free.argtypes = [vp, vp]
    L.gm_r1cs_eval.argtypes = [vp, vp, vp, vp, vp, vp]
    L.gm_g16_prove_r1cs.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp, vp]
    L.gm_jac_add.argtypes = [i, i, vp, vp, vp]
    L.gm_jac_to_affine.argtypes = [i, i, vp, vp]
    L.gm_batch_mul_base.argtypes = [vp, i, i, vp, vp, sz, vp]
    L.gm_random_scalars.argtypes = [vp, i, u64, sz, vp]
    L.gm_generator.argtypes = [i, i, vp]
    L.gm_icicle_generate_twiddles.argtypes = [vp, i, sz, i, pvp]
    L.gm_icicle_intt_on_device.argtypes = [vp, i, vp, sz, i, pvp]
    L.gm_icicle_ntt_on_device.argtypes = [vp, i, vp, vp, sz, i]
    L.gm_icicle_poly_ops.argtypes = [vp, i, vp, vp, vp, vp, sz]
    L.gm_device_count.argtypes = [ctypes.POINTER(i)]
    L.gm_multi_init.argtypes = [ctypes.POINTER(i), i, pvp]
    L.gm_multi_destroy.argtypes = [vp]
    L.gm_multi_size.argtypes = [vp, ctypes.POINTER(i)]
    L.gm_multi_context.argtypes = [vp, i, pvp]
    L.gm_g16_pk_upload_multi.argtypes = [vp, i, vp, ctypes.c_uint, pvp]
    L.gm_g16_pk_free_multi.argtypes = [vp, vp]
    L.gm_g16_prove_multi.argtypes = [vp, vp, vp, vp, vp, vp, sz, vp, vp, vp, vp, vp]
    L.gm_g16_pk_upload_dump.argtypes = [vp, i, vp, i, u64, ctypes.c_uint, ctypes.POINTER(u64), pvp]
    L.gm_g16_pk_upload_dump_shard.argtypes = [vp, i, vp, i, u64, ctypes.c_uint, i, i, ctypes.POINTER(u64), pvp]
    L.gm_g16_pk_save_cache.argtypes = [vp, vp, i]
    L.gm_g16_pk_load_cache.argtypes = [vp, i, pvp]
    L.gm_g16_stage_begin.argtypes = [vp, vp, sz, pvp]
    L.gm_g16_stage_put_range.argtypes = [vp, i, sz, sz, vp]
    L.gm_g16_stage_put_indexed.argtypes = [vp, i, vp, vp, sz]
    L.gm_g16_stage_prove.argtypes = [vp, vp, vp, vp, vp, vp]
    L.gm_g16_stage_free.argtypes = [vp]
    L.gm_g16_stage_prove_r1cs.argtypes = [vp, vp, vp, vp, vp, vp, vp]
    L.gm_msm_async.argtypes = [vp, i, i, vp, vp, sz, pvp]
    L.gm_msm_wait.argtypes = [vp, vp, vp]
    L.gm_plonk_pk_upload.argtypes = [vp, i, ctypes.POINTER(_PlonkPkHost), ctypes.c_uint, pvp]
    L.gm_plonk_pk_bytes.argtypes = [vp, psz, psz]
    L.gm_plonk_pk_free.argtypes = [vp, vp]
    L.gm_plonk_session_begin.argtypes = [vp, vp, pvp]
    L.gm_plonk_session_bsb22.argtypes = [vp, sz, vp, vp]
    L.gm_plonk_session_round1.argtypes = [vp, ctypes.POINTER(_PlonkRound1In), vp]
    L.gm_plonk_session_round2.argtypes = [vp, vp, vp, vp]
    L.gm_plonk_session_round3.argtypes = [vp, vp, vp]
    L.gm_plonk_session_round4.argtypes = [vp, vp, vp, vp, vp, vp]
    L.gm_plonk_session_round5.argtypes = [vp, vp, vp]
    L.gm_plonk_session_free.argtypes = [vp]
    L.gm_plonk_wires_upload.argtypes = [vp, sz, sz, vp, vp, vp, pvp]
    L.gm_plonk_wires_bytes.argtypes = [vp, psz]
    L.gm_plonk_wires_free.argtypes = [vp, vp]
    L.gm_plonk_gather_lro.argtypes = [vp, vp, vp, vp, vp, vp]
    L.gm_plonk_session_round1_witness.argtypes = [vp, vp, ctypes.POINTER(_PlonkRound1WitnessIn), vp]
    L.gm_plonk_session_bsb22_sparse.argtypes = [vp, sz, vp, vp, sz, vp]
    L.gm_kzg_srs_lagrange.argtypes = [vp, i, vp, sz, vp]
    L.gm_plonk_sigma.argtypes = [vp, i, sz, ctypes.POINTER(ctypes.c_int64), vp, vp, vp]
    L.gm_plonk_pk_setup.argtypes = [vp, i, ctypes.POINTER(_PlonkSetupHost), ctypes.c_uint, pvp, vp, vp]
    L.gm_plonk_wires_permutation.argtypes = [vp, vp, vp]
    L.gm_plonk_sigma_wires.argtypes = [vp, i, vp, vp, vp, vp]
    L.gm_plonk_pk_setup_wires.argtypes = [vp, i, ctypes.POINTER(_PlonkSetupHost), vp, ctypes.c_uint, pvp, vp, vp]
    L.gm_plonk_scs_upload.argtypes = [vp, i, ctypes.POINTER(_PlonkScsHost), pvp]
    L.gm_plonk_scs_bytes.argtypes = [vp, psz]
    L.gm_plonk_scs_free.argtypes = [vp, vp]
    L.gm_plonk_scs_wires.argtypes = [vp, pvp]
    L.gm_plonk_scs_selector.argtypes = [vp, vp, ctypes.c_uint, vp]
    L.gm_plonk_pk_setup_scs.argtypes = [vp, vp, vp, sz, ctypes.c_uint, pvp, vp, vp]
    L.gm_plonk_scs_check.argtypes = [vp, vp, vp, psz, psz]
    L.gm_set_fixed_base_window.argtypes = [vp, i]
    L.gm_batch_mul_fixed.argtypes = [vp, i, i, vp, vp, sz, vp]
    L.gm_set_g16_setup_column_cut.argtypes = [vp, i]
    L.gm_g16_setup_sizes.argtypes = [vp, vp, ctypes.POINTER(_G16SetupIn), psz, psz, psz]
    L.gm_g16_setup.argtypes = [vp, vp, ctypes.POINTER(_G16SetupIn), ctypes.POINTER(_G16SetupOut)]
    L.gm_g16_pk_setup.argtypes = [vp, vp, ctypes.POINTER(_G16SetupIn), ctypes.c_uint, pvp,
                                  ctypes.POINTER(_G16SetupOut)]
    L.gm_points_check.argtypes = [vp, i, i, vp, sz, vp, ctypes.POINTER(_PointsReport)]
    L.gm_points_check_host.argtypes = [vp, i, i, vp, sz, ctypes.POINTER(_PointsReport)]
    L.gm_set_points_check_chunk.argtypes = [vp, sz]
    L.gm_g16_pk_check.argtypes = [vp, i, vp, ctypes.POINTER(_G16PkReport)]
    L.gm_g16_pk_check_dump.argtypes = [vp, i, vp, i, u64, ctypes.POINTER(_G16PkReport), ctypes.POINTER(u64)]
    L.gm_points_decode.argtypes = [vp, i, i, i, ctypes.c_uint, vp, sz, vp, vp, ctypes.POINTER(_PointsDecodeReport)]
    L.gm_points_decode_host.argtypes = [vp, i, i, i, ctypes.c_uint, vp, sz, vp, vp,
                                        ctypes.POINTER(_PointsDecodeReport)]
    L.gm_points_encode.argtypes = [vp, i, i, i, vp, sz, vp, ctypes.POINTER(u64)]
    L.gm_g16_pk_upload_encoded.argtypes = [vp, i, vp, i, u64, i, ctypes.c_uint, vp,
                                           ctypes.POINTER(_G16PkDecodeReport), ctypes.POINTER(u64), pvp]
    L.gm_pairing_check.argtypes = [vp, i, vp, vp, sz, sz, vp]
    L.gm_pairing_check_device.argtypes = [vp, i, vp, vp, sz, sz, vp]
    L.gm_g16_vk_upload.argtypes = [vp, i, ctypes.POINTER(_G16VkHost), pvp]
    L.gm_g16_vk_free.argtypes = [vp, vp]
    L.gm_g16_verify_batch.argtypes = [vp, vp, vp, vp, sz, vp, psz]
    L.gm_kzg_vk_upload.argtypes = [vp, i, ctypes.POINTER(_KzgVkHost), pvp]
    L.gm_kzg_vk_free.argtypes = [vp, vp]
    L.gm_kzg_verify_batch.argtypes = [vp, vp, ctypes.POINTER(_KzgOpeningsHost), sz, vp, psz]
    L.gm_kzg_verify_folded.argtypes = [vp, vp, ctypes.POINTER(_KzgOpeningsHost), sz, vp]
    L.gm_plonk_vk_upload.argtypes = [vp, i, ctypes.POINTER(_PlonkVkHost), pvp]
    L.gm_plonk_vk_free.argtypes = [vp, vp]
    L.gm_plonk_verify_batch.argtypes = [vp, vp, ctypes.POINTER(_PlonkProofsHost), sz, vp, psz]
    _lib = L
    return L


def _check(rc: int):
    if rc != 0:
        raise GmError(f"gnark_mi355x error {rc}: {load_library().gm_last_error().decode()}")


def _buf(b) -> np.ndarray:
    if isinstance(b, np.ndarray):
        return np.ascontiguousarray(b).view(np.uint8).reshape(-1)
    return np.frombuffer(bytes(b), dtype=np.uint8)


def _p(a: np.ndarray):
    return a.ctypes.data_as(ctypes.c_void_p)


def curve_id(curve) -> int:
    return CURVES[curve] if isinstance(curve, str) else int(curve)


def point_bytes(curve, g2: bool) -> int:
    return FP_BYTES[curve_id(curve)] * (4 if g2 else 2)


def record_bytes(curve, g2: bool, encoding: int) -> int:
    """Bytes of one gnark-crypto record of a point (ENC_COMPRESSED or ENC_RAW)."""
    return FP_BYTES[curve_id(curve)] * (2 if g2 else 1) * (2 if encoding == ENC_RAW else 1)


def jac_bytes(curve, g2: bool) -> int:
    return FP_BYTES[curve_id(curve)] * (6 if g2 else 3)


def generator(curve, g2: bool = False) -> bytes:
    out = np.zeros(point_bytes(curve, g2), np.uint8)
    _check(load_library().gm_generator(curve_id(curve), int(g2), _p(out)))
    return out.tobytes()


def jac_add(curve, g2: bool, p: bytes, q: bytes) -> bytes:
    out = np.zeros(jac_bytes(curve, g2), np.uint8)
    a, b = _buf(p), _buf(q)
    _check(load_library().gm_jac_add(curve_id(curve), int(g2), _p(a), _p(b), _p(out)))
    return out.tobytes()


def jac_to_affine(curve, g2: bool, p: bytes) -> bytes:
    out = np.zeros(point_bytes(curve, g2), np.uint8)
    a = _buf(p)
    _check(load_library().gm_jac_to_affine(curve_id(curve), int(g2), _p(a), _p(out)))
    return out.tobytes()


def msm_geometry(curve, g2: bool, n: int, c: int = 0, layout: int = TGEOM_PLAIN) -> dict:
    """gm_test_msm_geometry: what an MSM of n scalars derives from its sizes
    (windows, sort bins, segment length, tree levels, allocations), from the
    driver's own host functions.  Needs no device.  Raises GmError where the plan
    refuses the MSM."""
    g = _MsmGeom()
    _check(load_testhooks().gm_test_msm_geometry(curve_id(curve), int(g2), n, c, layout, ctypes.byref(g)))
    out = {k: int(getattr(g, k)) for k, _ in _MsmGeom._fields_ if k != "lg"}
    out["lg"] = tuple(int(g.lg[i]) for i in range(g.levels))
    return out


class DeviceBuffer:
    """A device allocation owned by a Context (OnDeviceData{P, Size}, icicle.go:228)."""

    def __init__(self, ctx: "Context", ptr: int, nbytes: int):
        self.ctx, self.ptr, self.nbytes = ctx, ptr, nbytes

    def to_host(self, nbytes: int | None = None) -> bytes:
        n = self.nbytes if nbytes is None else nbytes
        out = np.zeros(n, np.uint8)
        _check(load_library().gm_memcpy_d2h(self.ctx.handle, _p(out), self.ptr, n))
        return out.tobytes()

    def write(self, data, offset: int = 0):
        a = _buf(data)
        _check(load_library().gm_memcpy_h2d(self.ctx.handle, self.ptr + offset, _p(a), a.size))

    def copy_from(self, src: "DeviceBuffer", nbytes: int | None = None):
        n = min(self.nbytes, src.nbytes) if nbytes is None else nbytes
        _check(load_library().gm_memcpy_d2d(self.ctx.handle, self.ptr, src.ptr, n))

    def free(self):
        if self.ptr:
            _check(load_library().gm_free(self.ctx.handle, self.ptr))
            self.ptr = 0


class Context:
    """One HIP device + stream (gm_ctx)."""

    def __init__(self, device: int = 0):
        L = load_library()
        h = ctypes.c_void_p()
        _check(L.gm_init(device, ctypes.byref(h)))
        self.handle = h
        self.device = device

    def trim(self):
        """gm_trim: release the memory the context keeps between calls."""
        _check(load_library().gm_trim(self.handle))

    def close(self):
        if self.handle:
            load_library().gm_destroy(self.handle)
            self.handle = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    # ---- memory ----------------------------------------------------------
    def malloc(self, nbytes: int) -> DeviceBuffer:
        p = ctypes.c_void_p()
        _check(load_library().gm_malloc(self.handle, nbytes, ctypes.byref(p)))
        return DeviceBuffer(self, p.value, nbytes)

    def copy_to_device(self, data) -> DeviceBuffer:
        a = _buf(data)
        p = ctypes.c_void_p()
        _check(load_library().gm_copy_to_device(self.handle, _p(a), a.size, ctypes.byref(p)))
        return DeviceBuffer(self, p.value, a.size)

    def copy_points_to_device(self, curve, points, g2: bool = False) -> DeviceBuffer:
        a = _buf(points)
        n = a.size // point_bytes(curve, g2)
        p = ctypes.c_void_p()
        _check(load_library().gm_copy_points_to_device(self.handle, curve_id(curve), int(g2), _p(a), n,
                                                       ctypes.byref(p)))
        return DeviceBuffer(self, p.value, a.size)

    def free_device_pointer(self, buf: DeviceBuffer):
        buf.free()

    # ---- point validation --------------------------------------------------
    def points_check(self, curve, points: DeviceBuffer, n: int, g2: bool = False, status: bool = False):
        """gm_points_check over n device-resident gnark points: the report as a
        dict, and with status=True also the class byte of every point."""
        rep = _PointsReport()
        st = self.malloc(max(n, 1)) if status else None
        try:
            _check(load_library().gm_points_check(self.handle, curve_id(curve), int(g2), points.ptr, n,
                                                  st.ptr if st else None, ctypes.byref(rep)))
            if st is None:
                return rep.as_dict()
            return rep.as_dict(), np.frombuffer(st.to_host(n), np.uint8)
        finally:
            if st is not None:
                st.free()

    def points_check_host(self, curve, points, g2: bool = False) -> dict:
        """gm_points_check_host: gnark points in host memory, streamed in chunks."""
        a = _buf(points)
        rep = _PointsReport()
        _check(load_library().gm_points_check_host(self.handle, curve_id(curve), int(g2), _p(a),
                                                   a.size // point_bytes(curve, g2), ctypes.byref(rep)))
        return rep.as_dict()

    # ---- pairing-product checks ---------------------------------------------
    def pairing_check(self, curve, g1, g2, k: int) -> np.ndarray:
        """gm_pairing_check: gnark points in host memory, products of k pairs each;
        one byte per product, 1 where the product of pairings is 1."""
        a, b = _buf(g1), _buf(g2)
        n = a.size // point_bytes(curve, False)
        assert k and n % k == 0 and b.size // point_bytes(curve, True) == n
        ok = np.full(max(n // k, 1), 0xEE, np.uint8)
        _check(load_library().gm_pairing_check(self.handle, curve_id(curve), _p(a), _p(b), n // k, k, _p(ok)))
        return ok[:n // k]

    def pairing_check_device(self, curve, g1: DeviceBuffer, g2: DeviceBuffer, n_products: int, k: int) -> np.ndarray:
        ok = np.full(max(n_products, 1), 0xEE, np.uint8)
        _check(load_library().gm_pairing_check_device(self.handle, curve_id(curve), g1.ptr, g2.ptr, n_products, k,
                                                      _p(ok)))
        return ok[:n_products]

    def test_pairing_op(self, curve, op: int, a: bytes, b: bytes | None, n: int, guard: int = 64) -> bytes:
        """gm_test_pairing_op over n elements; the output buffer carries `guard`
        bytes of 0xA5 behind it, which must come back untouched."""
        out_bytes = n * 12 * FP_BYTES[curve_id(curve)]
        A = self.copy_to_device(a)
        B = self.copy_to_device(b) if b else None
        O = self.copy_to_device(bytes([0xA5]) * (out_bytes + guard))
        try:
            _check(load_testhooks().gm_test_pairing_op(self.handle, curve_id(curve), op, A.ptr, B.ptr if B else None, n,
                                                       O.ptr))
            got = O.to_host()
            if got[out_bytes:] != bytes([0xA5]) * guard:
                raise GmError("gm_test_pairing_op wrote behind its output")
            return got[:out_bytes]
        finally:
            for x in (A, B, O):
                if x is not None:
                    x.free()

    def set_points_check_chunk(self, nbytes: int):
        """Test knob: the chunk of the streamed point checks (0 = the default)."""
        _check(load_library().gm_set_points_check_chunk(self.handle, nbytes))

    # ---- point encodings ---------------------------------------------------
    def points_decode(self, curve, records: DeviceBuffer, n: int, g2: bool = False, encoding: int = ENC_COMPRESSED,
                      flags: int = 0, status: bool = False):
        """gm_points_decode over n device-resident records: (points, report), the
        points as a new DeviceBuffer in gnark layout; with status=True also the
        class byte of every record."""
        rep = _PointsDecodeReport()
        pts = self.malloc(max(n, 1) * point_bytes(curve, g2))
        st = self.malloc(max(n, 1)) if status else None
        try:
            _check(load_library().gm_points_decode(self.handle, curve_id(curve), int(g2), encoding, flags,
                                                   records.ptr, n, pts.ptr, st.ptr if st else None,
                                                   ctypes.byref(rep)))
            if st is None:
                return pts, rep.as_dict()
            return pts, rep.as_dict(), np.frombuffer(st.to_host(n), np.uint8)
        except Exception:
            pts.free()
            raise
        finally:
            if st is not None:
                st.free()

    def points_decode_host(self, curve, records, g2: bool = False, encoding: int = ENC_COMPRESSED, flags: int = 0,
                           points_dev: DeviceBuffer = None, to_host: bool = True):
        """gm_points_decode_host: records in host memory, streamed in chunks.
        Returns (the points as bytes, or None with to_host=False; the report)."""
        a = _buf(records)
        n = a.size // record_bytes(curve, g2, encoding)
        out = np.zeros(n * point_bytes(curve, g2), np.uint8) if to_host else None
        rep = _PointsDecodeReport()
        _check(load_library().gm_points_decode_host(self.handle, curve_id(curve), int(g2), encoding, flags, _p(a), n,
                                                    points_dev.ptr if points_dev else None,
                                                    _p(out) if to_host else None, ctypes.byref(rep)))
        return (out.tobytes() if to_host else None), rep.as_dict()

    def points_encode(self, curve, points: DeviceBuffer, n: int, g2: bool = False, encoding: int = ENC_COMPRESSED):
        """gm_points_encode: (the records as a new DeviceBuffer, the count of
        points with a coordinate >= p, which are written as zero records)."""
        enc = self.malloc(max(n, 1) * record_bytes(curve, g2, encoding))
        bad = ctypes.c_uint64()
        try:
            _check(load_library().gm_points_encode(self.handle, curve_id(curve), int(g2), encoding, points.ptr, n,
                                                   enc.ptr, ctypes.byref(bad)))
        except Exception:
            enc.free()
            raise
        return enc, int(bad.value)

    def test_fe_sqrt(self, curve, elems, fp2: bool = False):
        """gm_test_fe_sqrt (test-only library): gnark-form Fp or Fp2 elements ->
        (roots in gnark form, exists bytes)."""
        a = _buf(elems)
        eb = FP_BYTES[curve_id(curve)] * (2 if fp2 else 1)
        n = a.size // eb
        src, root, ex = self.copy_to_device(a), self.malloc(max(a.size, 1)), self.malloc(max(n, 1))
        try:
            rc = load_testhooks().gm_test_fe_sqrt(self.handle, curve_id(curve), 2 if fp2 else 1, src.ptr, n, root.ptr,
                                                  ex.ptr)
            _check(rc)
            return root.to_host(n * eb), np.frombuffer(ex.to_host(n), np.uint8)
        finally:
            for b in (src, root, ex):
                b.free()

    def g16_pk_check(self, curve, pk: dict, domain_size: int, nb_wires: int, nb_public: int) -> dict:
        """gm_g16_pk_check: one report per member of the key ProvingKey would upload."""
        h, arrs = _pk_host_struct(curve, pk, domain_size, nb_wires, nb_public)
        rep = _G16PkReport()
        _check(load_library().gm_g16_pk_check(self.handle, curve_id(curve), ctypes.byref(h), ctypes.byref(rep)))
        del arrs
        return rep.as_dict()

    def g16_pk_check_dump(self, curve, path: str, offset: int, counts, domain_size: int):
        """gm_g16_pk_check_dump: the five point slices of a WriteDump file from byte
        `offset`; counts = (nbA, nbB, nbK).  Returns (report, end_offset)."""
        h = _PkHost()
        h.domain_size = domain_size
        h.nbA, h.nbB, h.nbK = counts
        rep, end = _G16PkReport(), ctypes.c_uint64()
        fd = os.open(path, os.O_RDONLY)
        try:
            _check(load_library().gm_g16_pk_check_dump(self.handle, curve_id(curve), ctypes.byref(h), fd, offset,
                                                       ctypes.byref(rep), ctypes.byref(end)))
        finally:
            os.close(fd)
        return rep.as_dict(), end.value

    def synchronize(self):
        _check(load_library().gm_synchronize(self.handle))

    # ---- profiling ---------------------------------------------------------
    def profile(self, on: bool = True):
        _check(load_library().gm_profile_enable(self.handle, int(on)))

    def profile_reset(self):
        _check(load_library().gm_profile_reset(self.handle))

    def profile_stats(self) -> dict:
        buf = ctypes.create_string_buffer(1 << 16)
        _check(load_library().gm_profile_dump(self.handle, buf, len(buf)))
        out = {}
        for line in buf.value.decode().splitlines():
            name, ms, cnt = line.split()
            out[name] = (float(ms), int(cnt))
        return out

    def set_msm_window(self, c: int):
        _check(load_library().gm_set_msm_window(self.handle, c))

    def set_msm_glv(self, mode: int):
        """GLV split of plain MSMs: 1 on, 0 off, -1 the size rule (on up to 2^21 points)."""
        _check(load_library().gm_set_msm_glv(self.handle, mode))

    def set_msm_piece_len(self, t: int):
        """G1 piece length (entries of one bucket per accumulation lane); 0 = the size rule."""
        _check(load_library().gm_set_msm_piece_len(self.handle, t))

    # ---- MSM -----------------------------------------------------------------
    def msm(self, curve, scalars: DeviceBuffer, points: DeviceBuffer, n: int, g2: bool = False):
        """Returns (jacobian_bytes, affine_bytes) in gnark layout."""
        jac = np.zeros(jac_bytes(curve, g2), np.uint8)
        aff = np.zeros(point_bytes(curve, g2), np.uint8)
        sp = scalars.ptr if isinstance(scalars, DeviceBuffer) else scalars
        pp = points.ptr if isinstance(points, DeviceBuffer) else points
        _check(load_library().gm_msm(self.handle, curve_id(curve), int(g2), sp, pp, n, _p(jac), _p(aff)))
        return jac.tobytes(), aff.tobytes()

    def msm_async(self, curve, scalars: DeviceBuffer, points: DeviceBuffer, n: int, g2: bool = False):
        """Queues an MSM (gm_msm_async); .wait() returns (jacobian_bytes, affine_bytes).
        At most three in flight per context, waited in issue order."""
        h = ctypes.c_void_p()
        sp = scalars.ptr if isinstance(scalars, DeviceBuffer) else scalars
        pp = points.ptr if isinstance(points, DeviceBuffer) else points
        _check(load_library().gm_msm_async(self.handle, curve_id(curve), int(g2), sp, pp, n, ctypes.byref(h)))
        return PendingMsm(h, curve, g2)

    def points_upload(self, curve, points, g2: bool = False) -> DeviceBuffer:
        """Device-resident point set in the MSM's internal layout (pk arrays, SRS)."""
        a = _buf(points)
        n = a.size // point_bytes(curve, g2)
        p = ctypes.c_void_p()
        _check(load_library().gm_points_upload(self.handle, curve_id(curve), int(g2), _p(a), n, ctypes.byref(p)))
        buf = DeviceBuffer(self, p.value, a.size)
        buf.count = n
        return buf

    def msm_prepared(self, curve, scalars: DeviceBuffer, prepared: DeviceBuffer, n: int, g2: bool = False):
        jac = np.zeros(jac_bytes(curve, g2), np.uint8)
        aff = np.zeros(point_bytes(curve, g2), np.uint8)
        _check(load_library().gm_msm_prepared(self.handle, curve_id(curve), int(g2), scalars.ptr, prepared.ptr, n,
                                              _p(jac), _p(aff)))
        return jac.tobytes(), aff.tobytes()

    def points_upload_precomputed(self, curve, points, g2: bool = False, window: int = 0) -> DeviceBuffer:
        """Point set plus its fixed-base window copies (gm_points_upload_precomputed)."""
        a = _buf(points)
        n = a.size // point_bytes(curve, g2)
        p = ctypes.c_void_p()
        _check(load_library().gm_points_upload_precomputed(self.handle, curve_id(curve), int(g2), _p(a), n, window,
                                                           ctypes.byref(p)))
        buf = DeviceBuffer(self, p.value, a.size)
        buf.count = n
        buf.window = window
        return buf

    def msm_precomputed(self, curve, scalars: DeviceBuffer, prepared: DeviceBuffer, n: int, g2: bool = False):
        jac = np.zeros(jac_bytes(curve, g2), np.uint8)
        aff = np.zeros(point_bytes(curve, g2), np.uint8)
        _check(load_library().gm_msm_precomputed(self.handle, curve_id(curve), int(g2), scalars.ptr, prepared.ptr,
                                                 prepared.count, prepared.window, n, _p(jac), _p(aff)))
        return jac.tobytes(), aff.tobytes()

    def kzg_commit(self, curve, srs: DeviceBuffer, coeffs) -> bytes:
        """kzg.Commit(p, pk): G1 digest of the polynomial coefficients (host)."""
        c = _buf(coeffs)
        out = np.zeros(point_bytes(curve, False), np.uint8)
        _check(load_library().gm_kzg_commit(self.handle, curve_id(curve), srs.ptr, srs.count, _p(c),
                                            c.size // FR_BYTES, _p(out)))
        return out.tobytes()

    # ---- KZG openings on resident polynomials ----------------------------------
    @staticmethod
    def _poly_table(polys, lens):
        """(pointer array, length array, k) of DeviceBuffer polynomials; lens
        defaults to each buffer's size in elements, None is the empty polynomial."""
        k = len(polys)
        if lens is None:
            lens = [0 if p is None else p.nbytes // FR_BYTES for p in polys]
        ptrs = (ctypes.c_void_p * max(k, 1))(*[None if p is None else p.ptr for p in polys])
        ls = (ctypes.c_size_t * max(k, 1))(*lens)
        return ptrs, ls, k

    def kzg_eval(self, curve, polys, z: bytes, lens=None) -> list:
        """gm_kzg_eval: [f_i(z)] as 32-byte Montgomery elements."""
        ptrs, ls, k = self._poly_table(polys, lens)
        zz = _buf(z)
        out = np.zeros(FR_BYTES * max(k, 1), np.uint8)
        _check(load_library().gm_kzg_eval(self.handle, curve_id(curve), ptrs, ls, k, _p(zz), _p(out)))
        b = out.tobytes()
        return [b[FR_BYTES * j:FR_BYTES * (j + 1)] for j in range(k)]

    def poly_div_linear(self, curve, f: DeviceBuffer, z: bytes, q: DeviceBuffer, m: int | None = None) -> bytes:
        """gm_poly_div_linear: q <- (f - f(z)) / (X - z) (m - 1 elements); returns f(z)."""
        m = f.nbytes // FR_BYTES if m is None else m
        zz = _buf(z)
        out = np.zeros(FR_BYTES, np.uint8)
        _check(load_library().gm_poly_div_linear(self.handle, curve_id(curve), f.ptr, m, _p(zz),
                                                 q.ptr if q is not None else None, _p(out)))
        return out.tobytes()

    def poly_fold(self, curve, polys, gamma: bytes, out: DeviceBuffer, lens=None):
        """gm_poly_fold: out <- sum_i gamma^i f_i (max(lens) elements)."""
        ptrs, ls, k = self._poly_table(polys, lens)
        g = _buf(gamma)
        _check(load_library().gm_poly_fold(self.handle, curve_id(curve), ptrs, ls, k, _p(g), out.ptr))

    def kzg_open(self, curve, srs: DeviceBuffer, f: DeviceBuffer, z: bytes, m: int | None = None):
        """kzg.Open on a resident polynomial: (claimed value, H affine) bytes."""
        m = f.nbytes // FR_BYTES if m is None else m
        zz = _buf(z)
        val = np.zeros(FR_BYTES, np.uint8)
        h = np.zeros(point_bytes(curve, False), np.uint8)
        _check(load_library().gm_kzg_open(self.handle, curve_id(curve), srs.ptr, srs.count, f.ptr, m, _p(zz),
                                          _p(val), _p(h)))
        return val.tobytes(), h.tobytes()

    def kzg_batch_open(self, curve, srs: DeviceBuffer, polys, z: bytes, gamma: bytes, lens=None):
        """kzg.BatchOpenSinglePoint once gamma is known: (F(z), H affine) bytes for
        F = sum_i gamma^i f_i."""
        ptrs, ls, k = self._poly_table(polys, lens)
        zz, g = _buf(z), _buf(gamma)
        val = np.zeros(FR_BYTES, np.uint8)
        h = np.zeros(point_bytes(curve, False), np.uint8)
        _check(load_library().gm_kzg_batch_open(self.handle, curve_id(curve), srs.ptr, srs.count, ptrs, ls, k,
                                                _p(zz), _p(g), _p(val), _p(h)))
        return val.tobytes(), h.tobytes()

    # ---- PLONK quotient on resident polynomials ---------------------------------
    def plonk_quotient(self, curve, n: int, polys: dict, qcp, pi2, blinds: dict, alpha: bytes, beta: bytes,
                       gamma: bytes, h: DeviceBuffer):
        """gm_plonk_quotient: h <- the quotient (4n elements, canonical, regular).
        polys: DeviceBuffers keyed by PLONK_POLYS (n unblinded elements each); qcp /
        pi2: lists of DeviceBuffers (BSB22 gates, may be empty; None passes a NULL
        table); blinds: bytes keyed bl, br, bo (2 elements) and bz (3 elements)."""
        a = _PlonkQuotientIn()
        a.n = n
        for k in PLONK_POLYS:
            setattr(a, k, polys[k].ptr)
        nb = max(len(qcp) if qcp is not None else 0, len(pi2) if pi2 is not None else 0)
        a.nb_bsb = nb
        tabs = []
        for name, t in (("qcp", qcp), ("pi2", pi2)):
            if t is not None and nb:
                arr = (ctypes.c_void_p * nb)(*[b.ptr for b in t])
                tabs.append(arr)
                setattr(a, name, ctypes.cast(arr, ctypes.POINTER(ctypes.c_void_p)))
        keep = [_buf(blinds[k]) for k in ("bl", "br", "bo", "bz")] + [_buf(alpha), _buf(beta), _buf(gamma)]
        for k, v in zip(("bl", "br", "bo", "bz", "alpha", "beta", "gamma"), keep):
            setattr(a, k, v.ctypes.data)
        _check(load_library().gm_plonk_quotient(self.handle, curve_id(curve), ctypes.byref(a), h.ptr))

    # ---- PLONK permutation polynomial Z on resident wires ------------------------
    def plonk_perm_z(self, curve, n: int, polys: dict, beta: bytes, gamma: bytes, z_lagrange: DeviceBuffer,
                     z_canonical: DeviceBuffer = None):
        """gm_plonk_perm_z: z_lagrange <- the copy-constraint accumulator Z (n
        elements, Lagrange regular); z_canonical, if given, <- the same polynomial
        in canonical regular form.  polys: DeviceBuffers keyed by PLONK_PERM_POLYS
        (n elements each, Lagrange regular; None passes a NULL pointer)."""
        a = _PlonkPermIn()
        a.n = n
        for k in PLONK_PERM_POLYS:
            setattr(a, k, polys[k].ptr if polys[k] is not None else None)
        keep = [_buf(beta), _buf(gamma)]
        a.beta, a.gamma = keep[0].ctypes.data, keep[1].ctypes.data
        _check(load_library().gm_plonk_perm_z(self.handle, curve_id(curve), ctypes.byref(a),
                                              z_lagrange.ptr if z_lagrange is not None else None,
                                              z_canonical.ptr if z_canonical is not None else None))

    # ---- PLONK linearized polynomial on resident buffers --------------------------
    def plonk_linearize(self, curve, n: int, polys: dict, qcp, pi2, blinds: dict, h: DeviceBuffer, alpha: bytes,
                        beta: bytes, gamma: bytes, zeta: bytes, lin: DeviceBuffer, h_rand: bytes = None,
                        blinded: dict = None) -> list:
        """gm_plonk_linearize: lin <- the linearized polynomial (n + 3 elements);
        returns [l~(zeta), r~(zeta), o~(zeta), s1(zeta), s2(zeta), z~(w zeta), qcp_j(zeta)...]
        as 32-byte Montgomery elements.  polys, qcp, pi2, blinds as plonk_quotient
        (a None in polys passes a NULL pointer); h: the quotient's 4n elements;
        h_rand: two elements (StatisticalZK) or None; blinded: DeviceBuffers keyed
        by PLONK_LIN_BLINDED (n + 2 elements, z_blinded n + 3), any of them absent."""
        a = _PlonkLinearizeIn()
        a.n = n
        for k in PLONK_POLYS:
            setattr(a, k, polys[k].ptr if polys[k] is not None else None)
        nb = max(len(qcp) if qcp is not None else 0, len(pi2) if pi2 is not None else 0)
        a.nb_bsb = nb
        tabs = []
        for name, t in (("qcp", qcp), ("pi2", pi2)):
            if t is not None and nb:
                arr = (ctypes.c_void_p * nb)(*[None if b is None else b.ptr for b in t])
                tabs.append(arr)
                setattr(a, name, ctypes.cast(arr, ctypes.POINTER(ctypes.c_void_p)))
        keep = {k: _buf(v) for k, v in (("bl", blinds["bl"]), ("br", blinds["br"]), ("bo", blinds["bo"]),
                                        ("bz", blinds["bz"]), ("h_rand", h_rand), ("alpha", alpha), ("beta", beta),
                                        ("gamma", gamma), ("zeta", zeta)) if v is not None}
        for k, v in keep.items():
            setattr(a, k, v.ctypes.data)
        a.h = h.ptr if h is not None else None
        o = _PlonkLinearizeOut()
        o.lin = lin.ptr if lin is not None else None
        for k in PLONK_LIN_BLINDED:
            b = (blinded or {}).get(k)
            setattr(o, k, b.ptr if b is not None else None)
        ev = np.zeros(FR_BYTES * (6 + nb), np.uint8)
        o.evals = ev.ctypes.data
        _check(load_library().gm_plonk_linearize(self.handle, curve_id(curve), ctypes.byref(a), ctypes.byref(o)))
        b = ev.tobytes()
        return [b[FR_BYTES * j:FR_BYTES * (j + 1)] for j in range(6 + nb)]

    def msm_on_device(self, scalars, points, n, curve="bn254"):
        """MsmOnDevice(scalars_d, points_d, count, convert=true) -> G1Jac bytes."""
        return self.msm(curve, scalars, points, n, g2=False)[0]

    def msm_g2_on_device(self, scalars, points, n, curve="bn254"):
        """MsmG2OnDevice -> G2Jac bytes."""
        return self.msm(curve, scalars, points, n, g2=True)[0]

    # ---- NTT -----------------------------------------------------------------
    def ntt(self, curve, data: DeviceBuffer, n: int, inverse: bool, dit: bool, coset: bool):
        _check(load_library().gm_ntt(self.handle, curve_id(curve), data.ptr, n, int(inverse), int(dit),
                                     int(coset)))

    def generate_twiddle_factors(self, curve, n: int, inverse: bool = False):
        """Twiddle tables are built and cached per (curve, n) inside the context on
        first use; this warms that cache (GenerateTwiddleFactors)."""
        tmp = self.malloc(FR_BYTES * n)
        try:
            _check(load_library().gm_ntt(self.handle, curve_id(curve), tmp.ptr, n, int(inverse), 0, 0))
        finally:
            tmp.free()

    # ---- iciclegnark call-for-call binding (icicle.go:68-76,489-510) ----------
    def icicle_generate_twiddle_factors(self, curve, n: int, inverse: bool) -> DeviceBuffer:
        """GenerateTwiddleFactors: a freeable handle; the tables live in the context."""
        p = ctypes.c_void_p()
        _check(load_library().gm_icicle_generate_twiddles(self.handle, curve_id(curve), n, int(inverse),
                                                          ctypes.byref(p)))
        return DeviceBuffer(self, p.value, 64)

    def icicle_intt_on_device(self, curve, scalars: DeviceBuffer, n: int, is_coset: bool) -> DeviceBuffer:
        """INttOnDevice: natural evaluations -> NEW buffer of natural coefficients."""
        p = ctypes.c_void_p()
        _check(load_library().gm_icicle_intt_on_device(self.handle, curve_id(curve), scalars.ptr, n, int(is_coset),
                                                       ctypes.byref(p)))
        return DeviceBuffer(self, p.value, FR_BYTES * n)

    def icicle_ntt_on_device(self, curve, out: DeviceBuffer, scalars: DeviceBuffer, n: int, is_coset: bool):
        """NttOnDevice(out, in): natural coefficients -> natural evaluations in out."""
        _check(load_library().gm_icicle_ntt_on_device(self.handle, curve_id(curve), out.ptr, scalars.ptr, n,
                                                      int(is_coset)))

    def icicle_poly_ops(self, curve, a: DeviceBuffer, b: DeviceBuffer, c: DeviceBuffer, den: DeviceBuffer, n: int):
        """PolyOps(a, b, c, den_d, n) with a device den vector."""
        _check(load_library().gm_icicle_poly_ops(self.handle, curve_id(curve), a.ptr, b.ptr, c.ptr, den.ptr, n))

    def poly_ops(self, curve, a: DeviceBuffer, b: DeviceBuffer, c: DeviceBuffer, n: int, den: bytes):
        d = _buf(den)
        _check(load_library().gm_poly_ops(self.handle, curve_id(curve), a.ptr, b.ptr, c.ptr, n, _p(d)))

    def reverse_scalars(self, curve, data: DeviceBuffer, n: int):
        _check(load_library().gm_reverse_scalars(self.handle, curve_id(curve), data.ptr, n))

    def compute_h(self, curve, a: DeviceBuffer, b: DeviceBuffer, c: DeviceBuffer, length: int, n: int):
        _check(load_library().gm_groth16_compute_h(self.handle, curve_id(curve), a.ptr, b.ptr, c.ptr,
                                                   length, n))

    # ---- synthetic inputs ---------------------------------------------------
    def random_scalars(self, curve, n: int, seed: int) -> DeviceBuffer:
        buf = self.malloc(FR_BYTES * n)
        _check(load_library().gm_random_scalars(self.handle, curve_id(curve), seed, n, buf.ptr))
        return buf

    def batch_mul_base(self, curve, g2: bool, base: bytes, scalars: DeviceBuffer, n: int) -> DeviceBuffer:
        out = self.malloc(point_bytes(curve, g2) * n)
        b = _buf(base)
        _check(load_library().gm_batch_mul_base(self.handle, curve_id(curve), int(g2), _p(b), scalars.ptr,
                                                n, out.ptr))
        return out

    # ---- Groth16 setup: fixed-base batch multiplication ---------------------------
    def set_fixed_base_window(self, c: int):
        """Window of batch_mul_fixed's table, 2..16; 0 = the cost model in n."""
        _check(load_library().gm_set_fixed_base_window(self.handle, c))

    def batch_mul_fixed(self, curve, g2: bool, base: bytes, scalars: DeviceBuffer, n: int,
                        out: DeviceBuffer | None = None) -> DeviceBuffer:
        """gm_batch_mul_fixed: out[i] = [k_i] base through a window table (the bytes
        of batch_mul_base), into out or a new buffer of n points."""
        own = out is None
        if own:
            out = self.malloc(point_bytes(curve, g2) * n)
        b = _buf(base)
        try:
            _check(load_library().gm_batch_mul_fixed(self.handle, curve_id(curve), int(g2), _p(b), scalars.ptr,
                                                     n, out.ptr))
        except GmError:
            if own:
                out.free()
            raise
        return out

    def set_g16_setup_column_cut(self, t: int):
        """Column length above which R1CS.g16_setup splits a column's sum over several
        blocks; 0 = the default."""
        _check(load_library().gm_set_g16_setup_column_cut(self.handle, t))

    # ---- PLONK setup ----------------------------------------------------------
    def kzg_srs_lagrange(self, curve, srs: DeviceBuffer, n: int, out: DeviceBuffer | None = None) -> DeviceBuffer:
        """gm_kzg_srs_lagrange: the Lagrange form of the first n points of srs (gnark
        G1Affine on the device), into out (srs itself for in place) or a new buffer."""
        if out is None:
            out = self.malloc(point_bytes(curve, False) * n)
        _check(load_library().gm_kzg_srs_lagrange(self.handle, curve_id(curve), srs.ptr, n, out.ptr))
        return out

    def plonk_sigma(self, curve, n: int, permutation) -> tuple[DeviceBuffer, DeviceBuffer, DeviceBuffer]:
        """gm_plonk_sigma: s1, s2, s3 (n Montgomery elements each, on the device) from
        gnark's trace.S, 3n integers (anything numpy takes as int64)."""
        perm = np.ascontiguousarray(permutation, dtype=np.int64)
        if perm.size != 3 * n:
            raise ValueError("the permutation has 3n entries")
        s = [self.malloc(FR_BYTES * n) for _ in range(3)]
        try:
            _check(load_library().gm_plonk_sigma(self.handle, curve_id(curve), n,
                                                 perm.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)),
                                                 s[0].ptr, s[1].ptr, s[2].ptr))
        except GmError:
            for b in s:
                b.free()
            raise
        return s[0], s[1], s[2]

    def plonk_sigma_wires(self, curve, wires: "PlonkWires") -> tuple[DeviceBuffer, DeviceBuffer, DeviceBuffer]:
        """gm_plonk_sigma_wires: s1, s2, s3 from resident wire tables, the permutation
        derived on the device."""
        s = [self.malloc(FR_BYTES * wires.n) for _ in range(3)]
        try:
            _check(load_library().gm_plonk_sigma_wires(self.handle, curve_id(curve), wires.handle,
                                                       s[0].ptr, s[1].ptr, s[2].ptr))
        except GmError:
            for b in s:
                b.free()
            raise
        return s[0], s[1], s[2]

    # ---- test hooks ---------------------------------------------------------
    def test_field_op(self, curve, kind: int, op: int, a: bytes, b: bytes) -> bytes:
        A, B = self.copy_to_device(a), self.copy_to_device(b)
        O = self.malloc(len(a))
        esz = {0: 32, 1: FP_BYTES[curve_id(curve)], 2: 2 * FP_BYTES[curve_id(curve)]}[kind]
        try:
            _check(load_testhooks().gm_test_field_op(self.handle, curve_id(curve), kind, op, A.ptr, B.ptr, O.ptr,
                                                   len(a) // esz))
            return O.to_host()
        finally:
            for x in (A, B, O):
                x.free()

    def test_point_op(self, curve, g2: bool, op: int, a: bytes, b: bytes) -> bytes:
        A, B = self.copy_to_device(a), self.copy_to_device(b)
        O = self.malloc(len(a))
        try:
            _check(load_testhooks().gm_test_point_op(self.handle, curve_id(curve), int(g2), op, A.ptr, B.ptr,
                                                   O.ptr, len(a) // point_bytes(curve, g2)))
            return O.to_host()
        finally:
            for x in (A, B, O):
                x.free()

    def test_field_raw_op(self, curve, kind: int, op: int, chain: int, operands, n: int, out_bytes: int) -> bytes:
        """gm_test_field_raw_op: up to four operand arrays of raw internal limbs
        (bytes, or None for an unused one) in, out_bytes of raw limbs out."""
        ops = list(operands) + [None] * (4 - len(operands))
        bufs = [self.copy_to_device(x) if x is not None else None for x in ops]
        O = self.malloc(out_bytes)
        try:
            _check(load_testhooks().gm_test_field_raw_op(self.handle, curve_id(curve), kind, op, chain,
                                                       *[b.ptr if b else None for b in bufs], O.ptr, n))
            return O.to_host()
        finally:
            for x in bufs + [O]:
                if x:
                    x.free()

    def test_point_raw_op(self, curve, g2: bool, op: int, chain: int, acc_in: bytes, other, flags, n: int) -> bytes:
        """gm_test_point_raw_op: raw XYZZ accumulators in and out (same size);
        other: gnark-layout affine points or raw XYZZ (None where the op takes
        none), flags: n bytes, bit 0 the digit sign (or None)."""
        bufs = [self.copy_to_device(x) if x is not None else None for x in (acc_in, other, flags)]
        O = self.malloc(len(acc_in))
        try:
            _check(load_testhooks().gm_test_point_raw_op(self.handle, curve_id(curve), int(g2), op, chain,
                                                       *[b.ptr if b else None for b in bufs], O.ptr, n))
            return O.to_host()
        finally:
            for x in bufs + [O]:
                if x:
                    x.free()

    def test_msm_g2_keyless_plan(self, curve, scalars: DeviceBuffer, points: DeviceBuffer, n: int):
        """A G2 launch over a plan built without sorted keys: the launch must refuse
        it, so this raises GmError naming the missing keys."""
        _check(load_testhooks().gm_test_msm_g2_keyless_plan(self.handle, curve_id(curve), scalars.ptr, points.ptr, n))

    def test_scan(self, op: int, out_init, n: int, data=None) -> bytes:
        """gm_test_scan over n u32.  The output buffer starts as out_init (u32: room
        for the result and the caller's guard words) and comes back whole.  data:
        the n input words, or None to scan in place on out_init's first n words."""
        O = self.copy_to_device(np.ascontiguousarray(out_init, dtype=np.uint32))
        I = self.copy_to_device(np.ascontiguousarray(data, dtype=np.uint32)) if data is not None and n else None
        try:
            _check(load_testhooks().gm_test_scan(self.handle, op, I.ptr if I else O.ptr, n, O.ptr))
            return O.to_host()
        finally:
            for x in (I, O):
                if x:
                    x.free()


# ---------------------------------------------------------------------------
# Multi-GPU MSM sharding: one process per GPU, each rank owns a
# contiguous slice of the point / scalar arrays, computes its partial Pippenger
# sum, and the N partial Jacobians (96 B G1 / 192 B G2 for BN254) are
# all-gathered (RCCL over xGMI with backend "nccl", or gloo on CPU) and reduced
# by N-1 host EC adds.  No other data-path communication.
# ---------------------------------------------------------------------------
def shard_range(n: int, world: int, rank: int) -> tuple[int, int]:
    """[lo, hi) of the contiguous shard of n items owned by `rank` (the first
    n % world ranks hold one extra item; a shard may be empty)."""
    if world <= 0 or not 0 <= rank < world:
        raise ValueError("bad rank/world")
    q, r = divmod(n, world)
    lo = rank * q + min(rank, r)
    return lo, lo + q + (1 if rank < r else 0)


def jac_infinity(curve, g2: bool) -> bytes:
    """gnark's G1Jac/G2Jac point at infinity {X: 1, Y: 1, Z: 0} (Montgomery one)."""
    out = np.zeros(jac_bytes(curve, g2), np.uint8)
    one = _mont_one(curve, g2)
    out[:one.size] = one
    out[one.size:2 * one.size] = one
    return out.tobytes()


_MONT_ONE_CACHE: dict = {}


def _mont_one(curve, g2: bool) -> np.ndarray:
    """Montgomery encoding of 1 in Fp (or Fp2 = (1, 0)), gnark layout."""
    key = (curve_id(curve), g2)
    if key not in _MONT_ONE_CACHE:
        cid = curve_id(curve)
        p = {BN254: 21888242871839275222246405745257275088696311157297823662689037894645226208583,
             BLS12_377: 258664426012969094010652733694893533536393512754914660539884262666720468348340822774968888139573360124440321458177,
             BLS12_381: 0x1a0111ea397fe69a4b1ba7b6434bacd764774b84f38512bf6730d2a0f6b0f6241eabfffeb153ffffb9feffffffffaaab}[cid]
        nb = FP_BYTES[cid]
        r = (1 << (8 * nb)) % p
        v = np.frombuffer(r.to_bytes(nb, "little"), np.uint8)
        if g2:
            v = np.concatenate([v, np.zeros(nb, np.uint8)])
        _MONT_ONE_CACHE[key] = v
    return _MONT_ONE_CACHE[key]


def reduce_partials(curve, g2: bool, partials) -> bytes:
    """Sum of gnark Jacobian partial results (host EC adds)."""
    acc = None
    for p in partials:
        acc = bytes(p) if acc is None else jac_add(curve, g2, acc, p)
    return acc if acc is not None else jac_infinity(curve, g2)


def allgather_partial(local_jac: bytes, group=None, device=None) -> list:
    """All-gathers one Jacobian partial (fixed size) from every rank."""
    import torch
    import torch.distributed as dist
    dev = device if device is not None else ("cuda" if dist.get_backend(group) == "nccl" else "cpu")
    t = torch.frombuffer(bytearray(local_jac), dtype=torch.uint8).to(dev)
    parts = [torch.empty_like(t) for _ in range(dist.get_world_size(group))]
    dist.all_gather(parts, t, group=group)
    return [q.cpu().numpy().tobytes() for q in parts]


def sharded_msm(ctx: "Context", curve, scalars, points, n_local: int, g2: bool = False, group=None,
                device=None) -> bytes:
    """Full MSM over the union of every rank's shard: local Pippenger on this
    rank's GPU, one all-gather of the partial sums, host reduction.  Returns the
    gnark Jacobian bytes (identical on every rank)."""
    if n_local:
        local = ctx.msm(curve, scalars, points, n_local, g2=g2)[0]
    else:
        local = jac_infinity(curve, g2)
    return reduce_partials(curve, g2, allgather_partial(local, group=group, device=device))


# ---------------------------------------------------------------------------
# Groth16 (icicle_bn254 ProvingKey / Prove mirror)
# ---------------------------------------------------------------------------
class _PkHost(ctypes.Structure):
    _fields_ = [(k, ctypes.c_size_t) for k in ["domain_size", "nb_wires", "nb_public", "nbA", "nbB", "nbK"]] + \
               [(k, ctypes.c_void_p) for k in ["g1_alpha", "g1_beta", "g1_delta", "g1_A", "g1_B", "g1_Z", "g1_K",
                                                "g2_beta", "g2_delta", "g2_B", "infA", "infB", "k_wires"]]


def _pk_host_struct(curve, pk: dict, domain_size: int, nb_wires: int, nb_public: int, shard=None,
                    pk_is_shard: bool = False):
    """gm_g16_pk_host for `pk` (a dict of gnark-layout arrays, see ProvingKey).
    shard = (rank, world): point arrays are sliced to the rank's shard unless
    pk_is_shard (they already are; the counts then come from pk['shard_sizes'])."""
    g1b, g2b = point_bytes(curve, False), point_bytes(curve, True)
    keys = ("g1_alpha", "g1_beta", "g1_delta", "g1_A", "g1_B", "g1_Z", "g1_K", "g2_beta", "g2_delta", "g2_B",
            "infA", "infB")
    arrs = {k: _buf(pk[k]) for k in keys}
    h = _PkHost()
    h.domain_size, h.nb_wires, h.nb_public = domain_size, nb_wires, nb_public
    if pk_is_shard:
        h.nbA, h.nbB, h.nbK = pk["shard_sizes"]
    else:
        h.nbA = arrs["g1_A"].size // g1b
        h.nbB = arrs["g1_B"].size // g1b
        h.nbK = arrs["g1_K"].size // g1b
    if "k_wires" in pk and pk["k_wires"] is not None:
        kw = np.ascontiguousarray(np.asarray(pk["k_wires"], dtype=np.uint32))
        h.nbK = kw.size
        h.k_wires = kw.ctypes.data
        arrs["k_wires"] = kw
    if shard is not None and not pk_is_shard:
        rank, world = shard
        for key, count, pb in (("g1_A", h.nbA, g1b), ("g1_B", h.nbB, g1b), ("g1_K", h.nbK, g1b),
                               ("g1_Z", domain_size - 1, g1b), ("g2_B", h.nbB, g2b)):
            lo, hi = shard_range(count, world, rank)
            arrs[key] = arrs[key][pb * lo:pb * hi].copy() if hi > lo else np.zeros(pb, np.uint8)
    for k in ["g1_alpha", "g1_beta", "g1_delta", "g1_A", "g1_B", "g1_Z", "g1_K", "g2_beta", "g2_delta",
              "g2_B", "infA", "infB"]:
        setattr(h, k, arrs[k].ctypes.data)
    return h, arrs


class ProvingKey:
    """Device-resident Groth16 proving key (icicle_bn254.ProvingKey + deviceInfo,
    provingkey.go:10-28; uploaded once like setupDevicePointers, icicle.go:31-130).

    `pk` is a dict of gnark-layout byte arrays: g1_alpha, g1_beta, g1_delta, g1_A,
    g1_B, g1_Z (n-1, bit-reversed), g1_K, g2_beta, g2_delta, g2_B, infA, infB, and
    optionally k_wires (the wire index of each pk.G1.K point when BSB22
    commitments filter K, prove.go:243-245; default nb_public + i).

    shard = (rank, world) keeps only this rank's slice of every point array on
    the device (gm_g16_pk_upload_shard; sharded_prove); with pk_is_shard the
    point arrays in `pk` already are the slices and pk['shard_sizes'] = (nbA, nbB, nbK)
    gives the whole key's counts.
    """

    PRECOMPUTE = 1  # GM_PK_PRECOMPUTE
    PRECOMPUTE_AUTO = 2  # GM_PK_PRECOMPUTE_AUTO: window copies iff they fit the device

    @classmethod
    def _flags(cls, precompute):
        """precompute: False / True / "auto" (GM_PK_PRECOMPUTE_AUTO)."""
        if precompute == "auto":
            return cls.PRECOMPUTE_AUTO
        return cls.PRECOMPUTE if precompute else 0

    @property
    def precomputed(self) -> bool:
        """Whether the device key holds the window copies (the auto choice)."""
        v = ctypes.c_int()
        _check(load_library().gm_g16_pk_precomputed(self.handle, ctypes.byref(v)))
        return bool(v.value)

    def __init__(self, ctx: Context, curve, pk: dict, domain_size: int, nb_wires: int, nb_public: int,
                 precompute: bool = False, shard=None, pk_is_shard: bool = False):
        self.ctx = ctx
        self.curve = curve_id(curve)
        h, arrs = _pk_host_struct(curve, pk, domain_size, nb_wires, nb_public, shard, pk_is_shard)
        self._keep = arrs
        self._h = h
        handle = ctypes.c_void_p()
        flags = self._flags(precompute)
        rank, world = shard if shard is not None else (0, 1)
        if shard is None:
            # the whole key: the entry every curve serves (a rank's share is BN254 / BLS12-377 only)
            _check(load_library().gm_g16_pk_upload_ex(ctx.handle, self.curve, ctypes.byref(h), flags,
                                                      ctypes.byref(handle)))
        else:
            _check(load_library().gm_g16_pk_upload_shard(ctx.handle, self.curve, ctypes.byref(h), flags, rank,
                                                         world, ctypes.byref(handle)))
        self.handle = handle
        self.n, self.nb_wires, self.nb_public = domain_size, nb_wires, nb_public
        self.shard = (rank, world)

    @classmethod
    def from_encoded(cls, ctx: Context, curve, path: str, offset: int, meta: dict, domain_size: int, nb_wires: int,
                     nb_public: int, encoding: int = ENC_COMPRESSED, flags: int = 0, precompute: bool = False):
        """Streams the points of a gnark WriteTo (ENC_COMPRESSED) or WriteRawTo
        (ENC_RAW) key file from byte `offset` (where G1.Alpha begins) through the
        device decoder into a resident key (gm_g16_pk_upload_encoded).  `meta` holds
        infA, infB, an optional k_wires and counts = (nbA, nbB, nbK).  Returns
        (key, end_offset, report, singles): singles are the five decoded single
        points in gnark layout.  A refused file raises GmError with the report as
        its `report` attribute."""
        self = cls.__new__(cls)
        self.ctx = ctx
        self.curve = curve_id(curve)
        g1b, g2b = point_bytes(curve, False), point_bytes(curve, True)
        stub = dict(meta)
        for k, pb in (("g1_alpha", g1b), ("g1_beta", g1b), ("g1_delta", g1b), ("g2_beta", g2b), ("g2_delta", g2b),
                      ("g1_A", g1b), ("g1_B", g1b), ("g1_Z", g1b), ("g1_K", g1b), ("g2_B", g2b)):
            stub[k] = np.zeros(pb, np.uint8)
        counts = stub.pop("counts")
        h, arrs = _pk_host_struct(curve, stub, domain_size, nb_wires, nb_public)
        h.nbA, h.nbB = counts[0], counts[1]
        if not ("k_wires" in meta and meta["k_wires"] is not None):
            h.nbK = counts[2]
        self._keep, self._h = arrs, h
        handle, end, rep = ctypes.c_void_p(), ctypes.c_uint64(), _G16PkDecodeReport()
        singles = np.zeros(3 * g1b + 2 * g2b, np.uint8)
        fd = os.open(path, os.O_RDONLY)
        try:
            rc = load_library().gm_g16_pk_upload_encoded(ctx.handle, self.curve, ctypes.byref(h), fd, offset, encoding,
                                                         flags | cls._flags(precompute), _p(singles),
                                                         ctypes.byref(rep), ctypes.byref(end), ctypes.byref(handle))
        finally:
            os.close(fd)
        if rc != 0:
            err = GmError(f"gnark_mi355x error {rc}: {load_library().gm_last_error().decode()}")
            err.rc, err.report, err.handle = rc, rep.as_dict(), handle.value
            raise err
        self.handle = handle
        self.n, self.nb_wires, self.nb_public = domain_size, nb_wires, nb_public
        self.shard = (0, 1)
        return self, end.value, rep.as_dict(), singles.tobytes()

    @classmethod
    def from_dump(cls, ctx: Context, curve, path: str, offset: int, meta: dict, domain_size: int, nb_wires: int,
                  nb_public: int, precompute: bool = False, shard=None):
        """Streams the point slices of a gnark WriteDump file (marshal.go:389-456)
        from byte `offset` into device buffers (gm_g16_pk_upload_dump_shard).
        `meta` holds the header fields (g1_alpha, g1_beta, g1_delta, g2_beta,
        g2_delta, infA, infB, optional k_wires) and the counts nbA / nbB / nbK.
        Returns (key, end_offset)."""
        self = cls.__new__(cls)
        self.ctx = ctx
        self.curve = curve_id(curve)
        g1b, g2b = point_bytes(curve, False), point_bytes(curve, True)
        stub = dict(meta)
        for k, pb in (("g1_A", g1b), ("g1_B", g1b), ("g1_Z", g1b), ("g1_K", g1b), ("g2_B", g2b)):
            stub[k] = np.zeros(pb, np.uint8)
        counts = stub.pop("counts")
        h, arrs = _pk_host_struct(curve, stub, domain_size, nb_wires, nb_public)
        h.nbA, h.nbB = counts[0], counts[1]
        if not ("k_wires" in meta and meta["k_wires"] is not None):
            h.nbK = counts[2]
        self._keep, self._h = arrs, h
        handle, end = ctypes.c_void_p(), ctypes.c_uint64()
        rank, world = shard if shard is not None else (0, 1)
        fd = os.open(path, os.O_RDONLY)
        try:
            _check(load_library().gm_g16_pk_upload_dump_shard(ctx.handle, self.curve, ctypes.byref(h),
                                                              fd, offset, cls._flags(precompute),
                                                              rank, world, ctypes.byref(end), ctypes.byref(handle)))
        finally:
            os.close(fd)
        self.handle = handle
        self.n, self.nb_wires, self.nb_public = domain_size, nb_wires, nb_public
        self.shard = (rank, world)
        return self, end.value

    def save_cache(self, path: str):
        """Device-layout copy of this key (gm_g16_pk_save_cache)."""
        fd = os.open(path, os.O_WRONLY | os.O_CREAT | os.O_TRUNC, 0o644)
        try:
            _check(load_library().gm_g16_pk_save_cache(self.ctx.handle, self.handle, fd))
        finally:
            os.close(fd)

    @classmethod
    def from_cache(cls, ctx: Context, path: str, like: "ProvingKey" = None):
        """Key read back from save_cache (gm_g16_pk_load_cache); `like` supplies
        the host-side metadata (the host finishing only needs what the cache holds)."""
        self = cls.__new__(cls)
        self.ctx = ctx
        handle = ctypes.c_void_p()
        fd = os.open(path, os.O_RDONLY)
        try:
            _check(load_library().gm_g16_pk_load_cache(ctx.handle, fd, ctypes.byref(handle)))
        finally:
            os.close(fd)
        self.handle = handle
        if like is not None:
            self.curve, self._h, self._keep = like.curve, like._h, like._keep
            self.n, self.nb_wires, self.nb_public, self.shard = like.n, like.nb_wires, like.nb_public, like.shard
        return self

    @classmethod
    def setup(cls, ctx: Context, r1cs: "R1CS", toxic, nb_public: int, gamma_wires=None, precompute=False,
              host_copy: bool = False):
        """gm_g16_pk_setup: the resident key derived on the device from the resident
        constraint system and the toxic scalars; nothing of it crosses PCIe.  Returns
        the key, or (key, the arrays as R1CS.g16_setup returns them) with host_copy."""
        self = cls.__new__(cls)
        self.ctx, self.curve = ctx, r1cs.curve
        self._keep = self._h = None
        handle = ctypes.c_void_p()
        if host_copy:
            a, o, collect, _keep = r1cs._setup_out(toxic, nb_public, gamma_wires)
        else:
            a, _keep = r1cs._setup_in(toxic, nb_public, gamma_wires)
            o, collect = None, None
        _check(load_library().gm_g16_pk_setup(ctx.handle, r1cs.handle, ctypes.byref(a), cls._flags(precompute),
                                              ctypes.byref(handle), ctypes.byref(o) if o is not None else None))
        self.handle = handle
        n = 1
        while n < r1cs.nc:
            n <<= 1
        self.n, self.nb_wires, self.nb_public = n, r1cs.nb_wires, nb_public
        self.shard = (0, 1)
        return (self, collect()) if host_copy else self

    def stage(self, nb_constraints: int) -> "Stage":
        return Stage(self, nb_constraints)

    def free(self):
        if self.handle:
            load_library().gm_g16_pk_free(self.ctx.handle, self.handle)
            self.handle = None

    def prove(self, wires, a, b, c, r: bytes, s: bytes):
        """Returns (Ar, Bs, Krs) affine bytes (gnark layout)."""
        W, A, B, C, R, S = (_buf(x) for x in (wires, a, b, c, r, s))
        ar = np.zeros(point_bytes(self.curve, False), np.uint8)
        krs = np.zeros(point_bytes(self.curve, False), np.uint8)
        bs = np.zeros(point_bytes(self.curve, True), np.uint8)
        _check(load_library().gm_g16_prove(self.ctx.handle, self.handle, _p(W), _p(A), _p(B), _p(C),
                                           A.size // FR_BYTES, _p(R), _p(S), _p(ar), _p(bs), _p(krs)))
        return ar.tobytes(), bs.tobytes(), krs.tobytes()

    def prove_r1cs(self, r1cs: "R1CS", wires, r: bytes, s: bytes):
        """gm_g16_prove_r1cs: the wires are the only host input; a, b, c come
        from the device-resident constraint system."""
        W, R, S = (_buf(x) for x in (wires, r, s))
        ar = np.zeros(point_bytes(self.curve, False), np.uint8)
        krs = np.zeros(point_bytes(self.curve, False), np.uint8)
        bs = np.zeros(point_bytes(self.curve, True), np.uint8)
        _check(load_library().gm_g16_prove_r1cs(self.ctx.handle, self.handle, r1cs.handle, _p(W), _p(R), _p(S),
                                                _p(ar), _p(bs), _p(krs)))
        return ar.tobytes(), bs.tobytes(), krs.tobytes()

    def prove_device(self, wires: DeviceBuffer, a: DeviceBuffer, b: DeviceBuffer, c: DeviceBuffer,
                     nb_constraints: int, r: bytes, s: bytes):
        R, S = _buf(r), _buf(s)
        ar = np.zeros(point_bytes(self.curve, False), np.uint8)
        krs = np.zeros(point_bytes(self.curve, False), np.uint8)
        bs = np.zeros(point_bytes(self.curve, True), np.uint8)
        _check(load_library().gm_g16_prove_device(self.ctx.handle, self.handle, wires.ptr, a.ptr, b.ptr, c.ptr,
                                                  nb_constraints, _p(R), _p(S), _p(ar), _p(bs), _p(krs)))
        return ar.tobytes(), bs.tobytes(), krs.tobytes()

    def prove_partial_device(self, wires: DeviceBuffer, a: DeviceBuffer, b: DeviceBuffer, c: DeviceBuffer,
                             nb_constraints: int) -> bytes:
        """This shard's raw MSM sums (gm_g16_prove_partial): 4 G1Jac + 1 G2Jac."""
        out = np.zeros(g16_partial_bytes(self.curve), np.uint8)
        _check(load_library().gm_g16_prove_partial(self.ctx.handle, self.handle, wires.ptr, a.ptr, b.ptr, c.ptr,
                                                   nb_constraints, _p(out)))
        return out.tobytes()


class VerifyingKey:
    """A Groth16 verifying key resident on the device (gm_g16_vk_upload).  vk: gnark
    point bytes alpha_g1, beta_g2, gamma_g2, delta_g2 and k_g1 (nb_k points)."""

    def __init__(self, ctx: Context, curve, vk: dict):
        self.ctx, self.curve = ctx, curve_id(curve)
        arrs = {k: _buf(vk[k]) for k in ("alpha_g1", "beta_g2", "gamma_g2", "delta_g2", "k_g1")}
        self.nb_k = arrs["k_g1"].size // point_bytes(curve, False)
        host = _G16VkHost(*[arrs[k].ctypes.data for k in ("alpha_g1", "beta_g2", "gamma_g2", "delta_g2", "k_g1")],
                          self.nb_k)
        h = ctypes.c_void_p()
        _check(load_library().gm_g16_vk_upload(ctx.handle, self.curve, ctypes.byref(host), ctypes.byref(h)))
        self.handle = h

    def verify_batch(self, proofs, publics) -> tuple[np.ndarray, int]:
        """gm_g16_verify_batch: proofs = m records Ar | Bs | Krs (gnark points),
        publics = m x (nb_k - 1) Montgomery fr.Elements; (status bytes, accepted)."""
        a, b = _buf(proofs), _buf(publics)
        m = a.size // (8 * FP_BYTES[self.curve])
        assert b.size == m * (self.nb_k - 1) * FR_BYTES
        st = np.full(max(m, 1), 0xEE, np.uint8)
        nb_ok = ctypes.c_size_t(0)
        _check(load_library().gm_g16_verify_batch(self.ctx.handle, self.handle, _p(a), _p(b) if b.size else None, m,
                                                  _p(st), ctypes.byref(nb_ok)))
        return st[:m], int(nb_ok.value)

    def free(self):
        if self.handle:
            _check(load_library().gm_g16_vk_free(self.ctx.handle, self.handle))
            self.handle = None


class KzgVk:
    """A KZG verifying key resident on the device (gm_kzg_vk_upload): gnark point
    bytes g1 (the G1 generator), g2_0 and g2_1 = [tau] G2."""

    def __init__(self, ctx: Context, curve, g1, g2_0, g2_1):
        self.ctx, self.curve = ctx, curve_id(curve)
        arrs = [_buf(g1), _buf(g2_0), _buf(g2_1)]
        host = _KzgVkHost(*[a.ctypes.data for a in arrs])
        h = ctypes.c_void_p()
        _check(load_library().gm_kzg_vk_upload(ctx.handle, self.curve, ctypes.byref(host), ctypes.byref(h)))
        self.handle = h

    def _openings(self, digests, proofs, points, values, lambdas=None):
        arrs = [_buf(x) for x in (digests, proofs, points, values)] + [_buf(lambdas) if lambdas is not None else None]
        m = arrs[2].size // FR_BYTES
        pb = point_bytes(self.curve, False)
        assert arrs[0].size == m * pb and arrs[1].size == m * pb and arrs[3].size == m * FR_BYTES
        assert arrs[4] is None or arrs[4].size == m * FR_BYTES
        return arrs, _KzgOpeningsHost(*[a.ctypes.data if a is not None and a.size else None for a in arrs]), m

    def verify_batch(self, digests, proofs, points, values, per_chunk=None) -> tuple[np.ndarray, int]:
        """gm_kzg_verify_batch: m openings (digest C, proof H, point z, value y);
        (status bytes, accepted).  per_chunk: through the test hook, that many
        openings per chunk."""
        keep, host, m = self._openings(digests, proofs, points, values)
        st = np.full(max(m, 1), 0xEE, np.uint8)
        nb_ok = ctypes.c_size_t(0)
        if per_chunk is None:
            _check(load_library().gm_kzg_verify_batch(self.ctx.handle, self.handle, ctypes.byref(host), m, _p(st),
                                                      ctypes.byref(nb_ok)))
        else:
            _check(load_testhooks().gm_test_kzg_verify_chunked(self.ctx.handle, self.handle, ctypes.byref(host), m,
                                                               per_chunk, 0, _p(st), ctypes.byref(nb_ok)))
        return st[:m], int(nb_ok.value)

    def verify_folded(self, digests, proofs, points, values, lambdas, per_chunk=None) -> int:
        """gm_kzg_verify_folded: the m openings folded with the caller's lambdas
        (lambda_0 is taken as 1) into one product; the batch's status byte."""
        keep, host, m = self._openings(digests, proofs, points, values, lambdas)
        st = np.full(1, 0xEE, np.uint8)
        if per_chunk is None:
            _check(load_library().gm_kzg_verify_folded(self.ctx.handle, self.handle, ctypes.byref(host), m, _p(st)))
        else:
            _check(load_testhooks().gm_test_kzg_verify_chunked(self.ctx.handle, self.handle, ctypes.byref(host), m,
                                                               per_chunk, 1, _p(st), None))
        return int(st[0])

    def free(self):
        if self.handle:
            _check(load_library().gm_kzg_vk_free(self.ctx.handle, self.handle))
            self.handle = None


class PlonkVk:
    """A PLONK verifying key resident on the device (gm_plonk_vk_upload).  vk: n,
    nb_public, gnark G1 point bytes ql, qr, qm, qo, qk, s1, s2, s3, qcp (nb_bsb points,
    one after the other), commitment_row (absolute rows) and the KZG members kzg_g1,
    kzg_g2_0, kzg_g2_1."""
    POINTS = ("ql", "qr", "qm", "qo", "qk", "s1", "s2", "s3")

    def __init__(self, ctx: Context, curve, vk: dict):
        self.ctx, self.curve = ctx, curve_id(curve)
        arrs = {k: _buf(vk[k]) for k in self.POINTS + ("kzg_g1", "kzg_g2_0", "kzg_g2_1")}
        qcp = _buf(vk.get("qcp", b""))
        rows = (ctypes.c_size_t * max(len(vk.get("commitment_row", ())), 1))(*vk.get("commitment_row", ()))
        self.nb_bsb = qcp.size // point_bytes(curve, False)
        self.n, self.nb_public = int(vk["n"]), int(vk["nb_public"])
        host = _PlonkVkHost(self.n, self.nb_public, *[arrs[k].ctypes.data for k in self.POINTS], self.nb_bsb,
                            qcp.ctypes.data if qcp.size else None, rows if self.nb_bsb else None,
                            *[arrs[k].ctypes.data for k in ("kzg_g1", "kzg_g2_0", "kzg_g2_1")])
        h = ctypes.c_void_p()
        _check(load_library().gm_plonk_vk_upload(ctx.handle, self.curve, ctypes.byref(host), ctypes.byref(h)))
        self.handle = h

    def _proofs(self, points, values, publics, hashed_cmt, challenges):
        arrs = [_buf(x if x is not None else b"") for x in (points, values, publics, hashed_cmt, challenges)]
        m = arrs[4].size // (6 * FR_BYTES)
        assert arrs[0].size == m * (9 + self.nb_bsb) * point_bytes(self.curve, False)
        assert arrs[1].size == m * (7 + self.nb_bsb) * FR_BYTES and arrs[2].size == m * self.nb_public * FR_BYTES
        assert arrs[3].size == m * self.nb_bsb * FR_BYTES
        return arrs, _PlonkProofsHost(*[a.ctypes.data if a.size else None for a in arrs]), m

    def verify_batch(self, points, values, publics, hashed_cmt, challenges, per_chunk=None) -> tuple[np.ndarray, int]:
        """gm_plonk_verify_batch: m proofs, each array holding the proofs' parts one
        after the other (the header has the order); (status bytes, accepted).
        per_chunk: through the test hook, that many proofs per chunk."""
        keep, host, m = self._proofs(points, values, publics, hashed_cmt, challenges)
        st = np.full(max(m, 1), 0xEE, np.uint8)
        nb_ok = ctypes.c_size_t(0)
        if per_chunk is None:
            _check(load_library().gm_plonk_verify_batch(self.ctx.handle, self.handle, ctypes.byref(host), m, _p(st),
                                                        ctypes.byref(nb_ok)))
        else:
            _check(load_testhooks().gm_test_plonk_verify_chunked(self.ctx.handle, self.handle, ctypes.byref(host), m,
                                                                 per_chunk, _p(st), ctypes.byref(nb_ok)))
        return st[:m], int(nb_ok.value)

    def test_scalars(self, values, publics, hashed_cmt, challenges):
        """gm_test_plonk_verify_scalars: (scalars bytes, m x (18 + 2 nb_bsb) Fr; aux
        bytes, m x (PI(zeta), constLin); class bytes)."""
        m = _buf(challenges).size // (6 * FR_BYTES)
        pts = np.zeros(m * (9 + self.nb_bsb) * point_bytes(self.curve, False), np.uint8)
        keep, host, m = self._proofs(pts, values, publics, hashed_cmt, challenges)
        T = 18 + 2 * self.nb_bsb
        scal, aux = np.zeros(m * T * FR_BYTES, np.uint8), np.zeros(m * 2 * FR_BYTES, np.uint8)
        cls = np.full(m, 0xEE, np.uint8)
        _check(load_testhooks().gm_test_plonk_verify_scalars(self.ctx.handle, self.handle, ctypes.byref(host), m,
                                                             _p(scal), _p(aux), _p(cls)))
        return scal.tobytes(), aux.tobytes(), cls

    def free(self):
        if self.handle:
            _check(load_library().gm_plonk_vk_free(self.ctx.handle, self.handle))
            self.handle = None


def kzg_vk_upload(ctx: Context, curve, g1, g2_0, g2_1) -> KzgVk:
    return KzgVk(ctx, curve, g1, g2_0, g2_1)


def kzg_verify_batch(vk: KzgVk, digests, proofs, points, values) -> tuple[np.ndarray, int]:
    return vk.verify_batch(digests, proofs, points, values)


def plonk_vk_upload(ctx: Context, curve, vk: dict) -> PlonkVk:
    return PlonkVk(ctx, curve, vk)


class PendingMsm:
    def __init__(self, handle, curve, g2):
        self.handle, self.curve, self.g2 = handle, curve, g2

    def wait(self):
        jac = np.zeros(jac_bytes(self.curve, self.g2), np.uint8)
        aff = np.zeros(point_bytes(self.curve, self.g2), np.uint8)
        h, self.handle = self.handle, None
        _check(load_library().gm_msm_wait(h, _p(jac), _p(aff)))
        return jac.tobytes(), aff.tobytes()


class Stage:
    """Prover inputs handed over while Solve runs (gm_g16_stage_*): put_range /
    put_indexed per solver level (constraint/bn254/solver.go:426-532), then prove."""

    A, B, C, WIRES = 0, 1, 2, 3

    def __init__(self, pk: ProvingKey, nb_constraints: int):
        self.pk = pk
        h = ctypes.c_void_p()
        _check(load_library().gm_g16_stage_begin(pk.ctx.handle, pk.handle, nb_constraints, ctypes.byref(h)))
        self.handle = h

    def put_range(self, which: int, lo: int, data):
        d = _buf(data)
        _check(load_library().gm_g16_stage_put_range(self.handle, which, lo, d.size // FR_BYTES, _p(d)))

    def put_indexed(self, which: int, base, idx):
        b = _buf(base)
        ix = np.ascontiguousarray(np.asarray(idx, dtype=np.uint32))
        _check(load_library().gm_g16_stage_put_indexed(self.handle, which, _p(b), ix.ctypes.data, ix.size))

    def replay_chain(self, wires, nb_inputs: int, nb_constraints: int, abc=None, coalesce=True,
                     flush_at: int = 1 << 16) -> float:
        """Test hook (gm_test_stage_replay_chain): stages the squaring chain's
        level shape -- level j finishes constraint j and solves wire nb_inputs + j
        -- one put per level (coalesce=False) or gathered as the Go level hook
        does.  abc = (a, b, c) host vectors to stage as well.  Returns host ns per
        level."""
        w = _buf(wires)
        bufs = [_buf(x) for x in abc] if abc is not None else []
        ptrs = [_p(x) for x in bufs] if bufs else [None, None, None]
        ns = ctypes.c_double()
        _check(load_testhooks().gm_test_stage_replay_chain(self.handle, _p(w), nb_inputs, ptrs[0], ptrs[1], ptrs[2],
                                                           nb_constraints, 1 if coalesce else 0, 1 if bufs else 0,
                                                           flush_at, ctypes.byref(ns)))
        return ns.value

    def prove(self, r: bytes, s: bytes):
        R, S = _buf(r), _buf(s)
        ar = np.zeros(point_bytes(self.pk.curve, False), np.uint8)
        krs = np.zeros(point_bytes(self.pk.curve, False), np.uint8)
        bs = np.zeros(point_bytes(self.pk.curve, True), np.uint8)
        _check(load_library().gm_g16_stage_prove(self.handle, _p(R), _p(S), _p(ar), _p(bs), _p(krs)))
        return ar.tobytes(), bs.tobytes(), krs.tobytes()

    def prove_r1cs(self, r1cs: "R1CS", r: bytes, s: bytes):
        """gm_g16_stage_prove_r1cs: the wires were staged (during Solve), a, b, c
        come from the device-resident constraint system."""
        R, S = _buf(r), _buf(s)
        ar = np.zeros(point_bytes(self.pk.curve, False), np.uint8)
        krs = np.zeros(point_bytes(self.pk.curve, False), np.uint8)
        bs = np.zeros(point_bytes(self.pk.curve, True), np.uint8)
        _check(load_library().gm_g16_stage_prove_r1cs(self.handle, r1cs.handle, _p(R), _p(S), _p(ar), _p(bs),
                                                      _p(krs)))
        return ar.tobytes(), bs.tobytes(), krs.tobytes()

    def free(self):
        if self.handle:
            load_library().gm_g16_stage_free(self.handle)
            self.handle = None


class PlonkProvingKey:
    """A PLONK proving key resident on the device (gm_plonk_pk_upload).  polys:
    host bytes keyed by PLONK_PK_POLYS (n elements each, Lagrange regular; qk
    without public inputs and commitment values); qcp: list of host bytes;
    commitment_row: their rows of Qk; srs_canonical / srs_lagrange: gnark G1Affine
    bytes.  cache=False uploads with GM_PLONK_PK_NO_COSET_CACHE; lin_key_qk=True with
    GM_PLONK_PK_LIN_KEY_QK (round 4 linearises with the key's Qk: the proofs a gnark
    verifier and PlonkVk.verify_batch accept).  A None among
    the inputs passes a NULL pointer; srs_canonical_len overrides the length
    taken from the bytes."""

    def __init__(self, ctx: Context, curve, n: int, nb_public: int, polys: dict, qcp, commitment_row,
                 srs_canonical, srs_lagrange, cache: bool = True, srs_canonical_len: int | None = None,
                 lin_key_qk: bool = False):
        self.ctx, self.curve, self.n, self.nb_public = ctx, curve, n, nb_public
        self.nb_bsb = len(qcp) if qcp is not None else len(commitment_row or [])
        h = _PlonkPkHost()
        h.n, h.nb_public, h.nb_bsb = n, nb_public, self.nb_bsb
        keep = []

        def ptr(b):
            if b is None:
                return None
            keep.append(_buf(b))
            return keep[-1].ctypes.data

        for k in PLONK_PK_POLYS:
            setattr(h, k, ptr(polys[k]))
        if qcp is not None and self.nb_bsb:
            tab = (ctypes.c_void_p * self.nb_bsb)(*[ptr(b) for b in qcp])
            keep.append(tab)
            h.qcp = ctypes.cast(tab, ctypes.POINTER(ctypes.c_void_p))
        if commitment_row is not None and self.nb_bsb:
            rows = (ctypes.c_size_t * self.nb_bsb)(*commitment_row)
            keep.append(rows)
            h.commitment_row = ctypes.cast(rows, ctypes.POINTER(ctypes.c_size_t))
        h.srs_canonical, h.srs_lagrange = ptr(srs_canonical), ptr(srs_lagrange)
        pb = point_bytes(curve, False)
        h.srs_canonical_len = (len(srs_canonical) // pb if srs_canonical is not None else 0) \
            if srs_canonical_len is None else srs_canonical_len
        out = ctypes.c_void_p()
        _check(load_library().gm_plonk_pk_upload(ctx.handle, curve_id(curve), ctypes.byref(h),
                                                 (0 if cache else PLONK_PK_NO_COSET_CACHE)
                                                 | (PLONK_PK_LIN_KEY_QK if lin_key_qk else 0), ctypes.byref(out)))
        self.handle = out

    @classmethod
    def setup(cls, ctx: Context, curve, n: int, nb_public: int, polys: dict, permutation, qcp, commitment_row,
              srs_canonical, cache: bool = True, srs_canonical_len: int | None = None, lagrange: bool = False,
              digests: bool = True, wires: "PlonkWires | None" = None, lin_key_qk: bool = False):
        """The key from what gnark's Setup holds (gm_plonk_pk_setup): polys keyed by
        PLONK_SETUP_POLYS, permutation = trace.S (3n integers), the canonical SRS
        alone.  Returns (key, the 8 + nb_bsb digests S1 S2 S3 Ql Qr Qm Qo Qk Qcp_j as
        gnark G1Affine bytes, the derived Lagrange SRS bytes or None).  A None among
        the inputs, or digests=False, passes a NULL pointer."""
        self = cls.__new__(cls)
        self.ctx, self.curve, self.n, self.nb_public = ctx, curve, n, nb_public
        self.nb_bsb = len(qcp) if qcp is not None else len(commitment_row or [])
        self.handle = None
        h = _PlonkSetupHost()
        h.n, h.nb_public, h.nb_bsb = n, nb_public, self.nb_bsb
        keep = []

        def ptr(b):
            if b is None:
                return None
            keep.append(_buf(b))
            return keep[-1].ctypes.data

        for k in PLONK_SETUP_POLYS:
            setattr(h, k, ptr(polys[k]))
        if permutation is not None:
            perm = np.ascontiguousarray(permutation, dtype=np.int64)
            if perm.size != 3 * n:
                raise ValueError("the permutation has 3n entries")
            keep.append(perm)
            h.permutation = perm.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))
        if qcp is not None and self.nb_bsb:
            tab = (ctypes.c_void_p * self.nb_bsb)(*[ptr(b) for b in qcp])
            keep.append(tab)
            h.qcp = ctypes.cast(tab, ctypes.POINTER(ctypes.c_void_p))
        if commitment_row is not None and self.nb_bsb:
            rows = (ctypes.c_size_t * self.nb_bsb)(*commitment_row)
            keep.append(rows)
            h.commitment_row = ctypes.cast(rows, ctypes.POINTER(ctypes.c_size_t))
        h.srs_canonical = ptr(srs_canonical)
        pb = point_bytes(curve, False)
        h.srs_canonical_len = (len(srs_canonical) // pb if srs_canonical is not None else 0) \
            if srs_canonical_len is None else srs_canonical_len
        dig = np.zeros(pb * (8 + self.nb_bsb), np.uint8) if digests else None
        lag = np.zeros(pb * n, np.uint8) if lagrange else None
        out = ctypes.c_void_p()
        flags = (0 if cache else PLONK_PK_NO_COSET_CACHE) | (PLONK_PK_LIN_KEY_QK if lin_key_qk else 0)
        tail = (ctypes.byref(out), _p(dig) if digests else None, _p(lag) if lagrange else None)
        if wires is None:
            _check(load_library().gm_plonk_pk_setup(ctx.handle, curve_id(curve), ctypes.byref(h), flags, *tail))
        else:
            _check(load_library().gm_plonk_pk_setup_wires(ctx.handle, curve_id(curve), ctypes.byref(h), wires.handle,
                                                          flags, *tail))
        self.handle = out
        db = dig.tobytes() if digests else b""
        return self, [db[i:i + pb] for i in range(0, len(db), pb)], (lag.tobytes() if lagrange else None)

    @classmethod
    def setup_from_wires(cls, ctx: Context, curve, n: int, nb_public: int, polys: dict, wires: "PlonkWires", qcp,
                         commitment_row, srs_canonical, cache: bool = True, srs_canonical_len: int | None = None,
                         lagrange: bool = False, digests: bool = True, permutation=None):
        """setup() with the permutation taken from resident wire tables
        (gm_plonk_pk_setup_wires).  permutation stays None: the call refuses one."""
        return cls.setup(ctx, curve, n, nb_public, polys, permutation, qcp, commitment_row, srs_canonical,
                         cache=cache, srs_canonical_len=srs_canonical_len, lagrange=lagrange, digests=digests,
                         wires=wires)

    @classmethod
    def setup_from_circuit(cls, circuit: "PlonkCircuit", srs_canonical, cache: bool = True,
                           srs_canonical_len: int | None = None, lagrange: bool = False, digests: bool = True):
        """The key from a resident circuit and the canonical SRS alone
        (gm_plonk_pk_setup_scs); returns what setup() returns."""
        self = cls.__new__(cls)
        ctx, curve, n = circuit.ctx, circuit.curve, circuit.n
        self.ctx, self.curve, self.n, self.nb_public = ctx, curve, n, circuit.nb_public
        self.nb_bsb = circuit.nb_bsb
        self.handle = None
        can = _buf(srs_canonical) if srs_canonical is not None else None
        pb = point_bytes(curve, False)
        can_len = (can.size // pb if can is not None else 0) if srs_canonical_len is None else srs_canonical_len
        dig = np.zeros(pb * (8 + self.nb_bsb), np.uint8) if digests else None
        lag = np.zeros(pb * n, np.uint8) if lagrange else None
        out = ctypes.c_void_p()
        _check(load_library().gm_plonk_pk_setup_scs(
            ctx.handle, circuit.handle, _p(can) if can is not None else None, can_len,
            0 if cache else PLONK_PK_NO_COSET_CACHE, ctypes.byref(out), _p(dig) if digests else None,
            _p(lag) if lagrange else None))
        self.handle = out
        db = dig.tobytes() if digests else b""
        return self, [db[i:i + pb] for i in range(0, len(db), pb)], (lag.tobytes() if lagrange else None)

    def resident_bytes(self) -> tuple[int, int]:
        """(resident bytes, coset cache bytes) of gm_plonk_pk_bytes."""
        a, b = ctypes.c_size_t(), ctypes.c_size_t()
        _check(load_library().gm_plonk_pk_bytes(self.handle, ctypes.byref(a), ctypes.byref(b)))
        return a.value, b.value

    def session(self) -> "PlonkSession":
        return PlonkSession(self)

    def free(self):
        if self.handle:
            _check(load_library().gm_plonk_pk_free(self.ctx.handle, self.handle))
            self.handle = None


class PlonkSession:
    """One proof on a PlonkProvingKey (gm_plonk_session_*): bsb22 per commitment,
    then round1 .. round5 with the caller's challenges between them.  Challenges
    and scalars are Montgomery fr.Element bytes, digests gnark G1Affine bytes."""

    def __init__(self, pk: PlonkProvingKey):
        self.pk = pk
        h = ctypes.c_void_p()
        _check(load_library().gm_plonk_session_begin(pk.ctx.handle, pk.handle, ctypes.byref(h)))
        self.handle = h

    def _pt(self, k: int = 1) -> np.ndarray:
        return np.zeros(k * point_bytes(self.pk.curve, False), np.uint8)

    @staticmethod
    def _split(a: np.ndarray, k: int) -> list:
        b = a.tobytes()
        w = len(b) // k
        return [b[w * j:w * (j + 1)] for j in range(k)]

    def bsb22(self, j: int, committed) -> bytes:
        c = _buf(committed) if committed is not None else None
        d = self._pt()
        _check(load_library().gm_plonk_session_bsb22(self.handle, j, _p(c) if c is not None else None, _p(d)))
        return d.tobytes()

    def round1(self, l, r, o, public_inputs, blinds: dict, commitment_vals=None, h_rand=None) -> list:
        """[commit(l~), commit(r~), commit(o~)]; blinds keyed bl, br, bo, bz."""
        a = _PlonkRound1In()
        vals = dict(blinds, l=l, r=r, o=o, public_inputs=public_inputs, commitment_vals=commitment_vals,
                    h_rand=h_rand)
        keep = {k: _buf(v) for k, v in vals.items() if v is not None and len(v)}
        for k, v in keep.items():
            setattr(a, k, v.ctypes.data)
        d = self._pt(3)
        _check(load_library().gm_plonk_session_round1(self.handle, ctypes.byref(a), _p(d)))
        return self._split(d, 3)

    def bsb22_sparse(self, j: int, rows, values) -> bytes:
        """bsb22 of the vector that is values[i] on row rows[i] and zero elsewhere
        (gm_plonk_session_bsb22_sparse); rows: integers, already offset by nb_public."""
        rw = np.ascontiguousarray(rows, dtype=np.uint32) if rows is not None else None
        v = _buf(values) if values is not None else None
        count = len(rw) if rw is not None else 0
        d = self._pt()
        _check(load_library().gm_plonk_session_bsb22_sparse(
            self.handle, j, _p(rw) if count else None, _p(v) if v is not None and v.size else None, count, _p(d)))
        return d.tobytes()

    def round1_witness(self, wires: "PlonkWires", witness, blinds: dict, commitment_vals=None, h_rand=None) -> list:
        """round1 from the solver's values (gm_plonk_session_round1_witness): l, r, o
        are gathered on the device through `wires`, the public inputs are the
        witness' first nb_public elements."""
        a = _PlonkRound1WitnessIn()
        vals = dict(blinds, witness=witness, commitment_vals=commitment_vals, h_rand=h_rand)
        keep = {k: _buf(v) for k, v in vals.items() if v is not None and len(v)}
        for k, v in keep.items():
            setattr(a, k, v.ctypes.data)
        d = self._pt(3)
        _check(load_library().gm_plonk_session_round1_witness(self.handle, wires.handle if wires is not None else None,
                                                              ctypes.byref(a), _p(d)))
        return self._split(d, 3)

    def round2(self, beta: bytes, gamma: bytes) -> bytes:
        b, g, d = _buf(beta), _buf(gamma), self._pt()
        _check(load_library().gm_plonk_session_round2(self.handle, _p(b), _p(g), _p(d)))
        return d.tobytes()

    def round3(self, alpha: bytes) -> list:
        a, d = _buf(alpha), self._pt(3)
        _check(load_library().gm_plonk_session_round3(self.handle, _p(a), _p(d)))
        return self._split(d, 3)

    def round4(self, zeta: bytes):
        """(commit(lin), claimed values [lin, l~, r~, o~, s1, s2, qcp_j at zeta],
        z~(w zeta), proof of its opening)."""
        z, lin, hz = _buf(zeta), self._pt(), self._pt()
        k = 6 + self.pk.nb_bsb
        claimed = np.zeros(FR_BYTES * k, np.uint8)
        zs = np.zeros(FR_BYTES, np.uint8)
        _check(load_library().gm_plonk_session_round4(self.handle, _p(z), _p(lin), _p(claimed), _p(zs), _p(hz)))
        return lin.tobytes(), self._split(claimed, k), zs.tobytes(), hz.tobytes()

    def round5(self, kzg_gamma: bytes) -> bytes:
        g, d = _buf(kzg_gamma), self._pt()
        _check(load_library().gm_plonk_session_round5(self.handle, _p(g), _p(d)))
        return d.tobytes()

    def free(self):
        if self.handle:
            _check(load_library().gm_plonk_session_free(self.handle))
            self.handle = None


class PlonkWires:
    """The wire tables of a PLONK circuit resident on the device
    (gm_plonk_wires_upload): xa, xb, xc are n wire ids each (anything numpy takes
    as uint32), complete rows as evaluateLROSmallDomain defines them, every id
    below nb_wires.  A None among them passes a NULL pointer."""

    def __init__(self, ctx: Context, n: int, nb_wires: int, xa, xb, xc):
        self.ctx, self.n, self.nb_wires = ctx, n, nb_wires
        tabs = [np.ascontiguousarray(t, dtype=np.uint32) if t is not None else None for t in (xa, xb, xc)]
        if any(t is not None and t.size != n for t in tabs):
            raise ValueError("PlonkWires: every table has n ids")
        out = ctypes.c_void_p()
        _check(load_library().gm_plonk_wires_upload(ctx.handle, n, nb_wires,
                                                    *[_p(t) if t is not None else None for t in tabs],
                                                    ctypes.byref(out)))
        self.handle = out

    def gather(self, witness: DeviceBuffer, l: DeviceBuffer, r: DeviceBuffer, o: DeviceBuffer):
        """gm_plonk_gather_lro: l[i] = witness[xa[i]], r[i] = witness[xb[i]],
        o[i] = witness[xc[i]] on resident buffers of 32-byte elements."""
        _check(load_library().gm_plonk_gather_lro(self.ctx.handle, self.handle, witness.ptr, l.ptr, r.ptr, o.ptr))

    def permutation(self, out: DeviceBuffer | None = None) -> DeviceBuffer:
        """gm_plonk_wires_permutation: gnark's trace.S (3n int64) on the device,
        derived from the tables; np.frombuffer(buf.to_host(), np.int64) reads it."""
        own = out is None
        if own:
            out = self.ctx.malloc(8 * 3 * self.n)
        try:
            _check(load_library().gm_plonk_wires_permutation(self.ctx.handle, self.handle, out.ptr))
        except GmError:
            if own:
                out.free()
            raise
        return out

    def resident_bytes(self) -> int:
        a = ctypes.c_size_t()
        _check(load_library().gm_plonk_wires_bytes(self.handle, ctypes.byref(a)))
        return a.value

    def free(self):
        if self.handle:
            _check(load_library().gm_plonk_wires_free(self.ctx.handle, self.handle))
            self.handle = None


class PlonkCircuit:
    """A PLONK constraint system resident on the device (gm_plonk_scs_upload).
    records: nb_constraints x 9 integers, gnark's SparseR1C as it lies in memory
    (XA XB XC QL QR QO QM QC Commitment); coeffs: the CoeffTable as Montgomery
    fr.Element bytes; committed: per BSB22 gate its constraint indices;
    commitment_index: per gate the constraint of its commitment.  A None among
    records / coeffs passes a NULL pointer; nb_constraints and ncoeffs override
    the sizes taken from the arrays."""

    def __init__(self, ctx: Context, curve, n: int, nb_public: int, nb_wires: int, records, coeffs, committed=(),
                 commitment_index=(), nb_constraints: int | None = None, ncoeffs: int | None = None):
        self.ctx, self.curve, self.n, self.nb_public, self.nb_wires = ctx, curve, n, nb_public, nb_wires
        rec = np.ascontiguousarray(records, dtype=np.uint32).reshape(-1) if records is not None else None
        co = _buf(coeffs) if coeffs is not None else None
        h = _PlonkScsHost()
        h.n, h.nb_public, h.nb_wires = n, nb_public, nb_wires
        h.nb_constraints = (rec.size // SCS_RECORD_WORDS if rec is not None else 0) \
            if nb_constraints is None else nb_constraints
        h.ncoeffs = (co.size // FR_BYTES if co is not None else 0) if ncoeffs is None else ncoeffs
        self.nb_constraints = h.nb_constraints
        if rec is not None and rec.size:
            h.records = rec.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32))
        if co is not None and co.size:
            h.coeffs = co.ctypes.data
        self.nb_bsb = h.nb_bsb = len(commitment_index)
        if self.nb_bsb:
            rows = [np.ascontiguousarray(c, dtype=np.uint32) for c in committed]
            p32 = ctypes.POINTER(ctypes.c_uint32)
            # an empty gate still gets a pointer: only its length says it is empty
            lens = (ctypes.c_size_t * self.nb_bsb)(*[a.size for a in rows])
            rows = [a if a.size else np.zeros(1, np.uint32) for a in rows]
            tab = (p32 * self.nb_bsb)(*[a.ctypes.data_as(p32) for a in rows])
            idx = (ctypes.c_size_t * self.nb_bsb)(*commitment_index)
            h.committed, h.committed_len, h.commitment_index = tab, lens, idx
        out = ctypes.c_void_p()
        _check(load_library().gm_plonk_scs_upload(ctx.handle, curve_id(curve), ctypes.byref(h), ctypes.byref(out)))
        self.handle = out

    def wires(self) -> "PlonkWires":
        """The wire tables inside the circuit (gm_plonk_scs_wires), for every call
        that takes a PlonkWires.  Borrowed: freed with the circuit, and free() on
        them is refused."""
        h = ctypes.c_void_p()
        _check(load_library().gm_plonk_scs_wires(self.handle, ctypes.byref(h)))
        w = PlonkWires.__new__(PlonkWires)
        w.ctx, w.n, w.nb_wires, w.handle = self.ctx, self.n, self.nb_wires, h
        return w

    def selector(self, which: int, out: DeviceBuffer | None = None) -> DeviceBuffer:
        """gm_plonk_scs_selector: column `which` (SCS_QL .. SCS_QK, SCS_QCP0 + j) as n
        elements on the device."""
        own = out is None
        if own:
            out = self.ctx.malloc(FR_BYTES * self.n)
        try:
            _check(load_library().gm_plonk_scs_selector(self.ctx.handle, self.handle, which, out.ptr))
        except GmError:
            if own:
                out.free()
            raise
        return out

    def check(self, witness) -> tuple[int, int | None]:
        """gm_plonk_scs_check: (number of unsatisfied constraints, the smallest such
        constraint index or None)."""
        w = _buf(witness) if witness is not None else None
        cnt, first = ctypes.c_size_t(), ctypes.c_size_t(2**64 - 1)
        _check(load_library().gm_plonk_scs_check(self.ctx.handle, self.handle, _p(w) if w is not None else None,
                                                 ctypes.byref(cnt), ctypes.byref(first)))
        return cnt.value, (None if first.value == 2**64 - 1 else first.value)

    def resident_bytes(self) -> int:
        a = ctypes.c_size_t()
        _check(load_library().gm_plonk_scs_bytes(self.handle, ctypes.byref(a)))
        return a.value

    def free(self):
        if self.handle:
            _check(load_library().gm_plonk_scs_free(self.ctx.handle, self.handle))
            self.handle = None


def write_dump_slices(path: str, curve, pk: dict, prefix: bytes = b"") -> int:
    """Writes `prefix` then pk's five point arrays as gnark-crypto
    utils/unsafe.WriteSlice records in WriteDump order (marshal.go:430-444):
    u64 little-endian count + raw points.  Returns the offset of the first
    slice.  (Test / tooling helper: the real file comes from gnark's WriteDump.)"""
    with open(path, "wb") as f:
        f.write(prefix)
        for key, g2 in (("g1_A", False), ("g1_B", False), ("g1_Z", False), ("g1_K", False), ("g2_B", True)):
            raw = _buf(pk[key]).tobytes()
            f.write(struct.pack("<Q", len(raw) // point_bytes(curve, g2)))
            f.write(raw)
    return len(prefix)


class Multi:
    """Several devices driven from ONE process (gm_multi): one context and host
    thread per entry of device_ids (entries may repeat: several contexts on one
    GPU rehearse the multi-GPU path).  The single-process seam gnark's
    groth16.Prove needs (backend/groth16/groth16.go:192-204)."""

    def __init__(self, device_ids):
        ids = (ctypes.c_int * len(device_ids))(*device_ids)
        h = ctypes.c_void_p()
        _check(load_library().gm_multi_init(ids, len(device_ids), ctypes.byref(h)))
        self.handle = h
        self.device_ids = list(device_ids)

    def close(self):
        if self.handle:
            load_library().gm_multi_destroy(self.handle)
            self.handle = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()


R1CS_CONST = 0xFFFFFFFF  # GM_R1CS_CONST: a constant term (constraint.Term.IsConstant)


class R1CS:
    """A constraint system resident on the device (gm_r1cs_upload): per matrix
    L, R, O a CSR of (coefficient id, wire id) terms over a coefficient table
    (gnark's CoeffTable: id 0 = 0, 1 = 1, 2 = 2, 3 = -1, 4 = -2, then the
    circuit's own).  from_terms builds the table from per-term coefficients."""

    def __init__(self, ctx: Context, curve, nb_constraints: int, nb_wires: int, rowptr, cid, vid, coeffs: bytes):
        self.ctx = ctx
        self.curve = curve_id(curve)
        self.nc, self.nb_wires = nb_constraints, nb_wires
        rp = [np.ascontiguousarray(np.asarray(x, np.uint32)) for x in rowptr]
        ci = [np.ascontiguousarray(np.asarray(x if len(x) else [0], np.uint32)) for x in cid]
        vi = [np.ascontiguousarray(np.asarray(x if len(x) else [0], np.uint32)) for x in vid]
        co = _buf(coeffs)
        arr = lambda xs: (ctypes.c_void_p * 3)(*[x.ctypes.data for x in xs])
        handle = ctypes.c_void_p()
        _check(load_library().gm_r1cs_upload(ctx.handle, self.curve, nb_constraints, nb_wires, arr(rp), arr(ci),
                                             arr(vi), _p(co), co.size // FR_BYTES, ctypes.byref(handle)))
        self.handle = handle

    @classmethod
    def from_terms(cls, ctx: Context, curve, nb_constraints: int, nb_wires: int, rowptr, wires, coeffs, modulus: int):
        """rowptr / wires / coeffs per matrix as in tests/r1cs.R1CS (coeffs: 32-byte
        Montgomery values per term)."""
        R = (1 << 256) % modulus
        enc = lambda v: (v * R % modulus).to_bytes(32, "little")
        table = [enc(0), enc(1), enc(2), enc(modulus - 1), enc(modulus - 2)]
        index = {t: k for k, t in enumerate(table)}
        cid = []
        for m in range(3):
            cb = bytes(np.asarray(coeffs[m], np.uint8).tobytes())
            nt = int(rowptr[m][-1])
            ids = []
            for q in range(nt):
                t = cb[32 * q:32 * q + 32]
                if t not in index:
                    index[t] = len(table)
                    table.append(t)
                ids.append(index[t])
            cid.append(ids)
        vid = [list(np.asarray(wires[m], np.uint32)[:int(rowptr[m][-1])]) for m in range(3)]
        return cls(ctx, curve, nb_constraints, nb_wires, rowptr, cid, vid, b"".join(table))

    def eval(self, wires: DeviceBuffer, a: DeviceBuffer, b: DeviceBuffer, c: DeviceBuffer):
        _check(load_library().gm_r1cs_eval(self.ctx.handle, self.handle, wires.ptr, a.ptr, b.ptr, c.ptr))

    def _setup_in(self, toxic, nb_public: int, gamma_wires):
        a = _G16SetupIn()
        keep = [_buf(toxic) if toxic is not None else None]
        a.toxic = keep[0].ctypes.data if keep[0] is not None else None
        a.nb_public = nb_public
        if gamma_wires is not None and len(gamma_wires):
            gw = np.ascontiguousarray(np.asarray(gamma_wires, dtype=np.uint32))
            keep.append(gw)
            a.gamma_wires = gw.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32))
            a.nb_gamma = gw.size
        return a, keep

    def g16_setup_sizes(self, toxic, nb_public: int, gamma_wires=None) -> tuple[int, int, int]:
        """gm_g16_setup_sizes: (nbA, nbB, nbK) from the scalar side alone."""
        a, _keep = self._setup_in(toxic, nb_public, gamma_wires)
        n = [ctypes.c_size_t() for _ in range(3)]
        _check(load_library().gm_g16_setup_sizes(self.ctx.handle, self.handle, ctypes.byref(a),
                                                 *[ctypes.byref(x) for x in n]))
        return tuple(x.value for x in n)

    def _setup_out(self, toxic, nb_public: int, gamma_wires):
        """(in struct, out struct, collect): host buffers sized by gm_g16_setup_sizes;
        collect() turns them into the dict g16_setup returns."""
        nbA, nbB, nbK = self.g16_setup_sizes(toxic, nb_public, gamma_wires)
        a, keep = self._setup_in(toxic, nb_public, gamma_wires)
        n = 1
        while n < self.nc:
            n <<= 1
        g1b, g2b = point_bytes(self.curve, False), point_bytes(self.curve, True)
        sizes = {"g1_alpha": g1b, "g1_beta": g1b, "g1_delta": g1b, "g1_A": g1b * nbA, "g1_B": g1b * nbB,
                 "g1_Z": g1b * (n - 1), "g1_K": g1b * nbK, "g1_K_gamma": g1b * (nb_public + a.nb_gamma),
                 "g2_beta": g2b, "g2_delta": g2b, "g2_gamma": g2b, "g2_B": g2b * nbB,
                 "infA": self.nb_wires, "infB": self.nb_wires, "k_wires": 4 * nbK}
        bufs = {k: np.zeros(max(v, 1), np.uint8) for k, v in sizes.items()}
        o = _G16SetupOut()
        for k in G16_SETUP_OUT_FIELDS:
            setattr(o, k, bufs[k].ctypes.data)

        def collect():
            out = {k: bufs[k][:sizes[k]].tobytes() for k in G16_SETUP_OUT_FIELDS if k != "k_wires"}
            out["k_wires"] = [int(w) for w in bufs["k_wires"][:4 * nbK].view(np.uint32)]
            return out

        return a, o, collect, keep

    def g16_setup(self, toxic, nb_public: int, gamma_wires=None) -> dict:
        """gm_g16_setup: gnark's Setup from the resident constraint system and the five
        toxic scalars (t, alpha, beta, gamma, delta as Montgomery bytes).  Returns the
        key's arrays as gnark-layout bytes under oracle.g16_setup's names, plus
        g1_K_gamma (the verifier's side: public wires, then gamma_wires), g2_gamma and
        k_wires (the wire of every g1_K point)."""
        a, o, collect, _keep = self._setup_out(toxic, nb_public, gamma_wires)
        _check(load_library().gm_g16_setup(self.ctx.handle, self.handle, ctypes.byref(a), ctypes.byref(o)))
        return collect()

    def free(self):
        if self.handle:
            load_library().gm_r1cs_free(self.ctx.handle, self.handle)
            self.handle = None


class ProvingKeyMulti:
    """A proving key sharded across the devices of a Multi (gm_g16_pk_upload_multi)."""

    def __init__(self, multi: Multi, curve, pk: dict, domain_size: int, nb_wires: int, nb_public: int,
                 precompute: bool = False):
        self.multi = multi
        self.curve = curve_id(curve)
        h, arrs = _pk_host_struct(curve, pk, domain_size, nb_wires, nb_public)
        self._keep, self._h = arrs, h
        handle = ctypes.c_void_p()
        _check(load_library().gm_g16_pk_upload_multi(multi.handle, self.curve, ctypes.byref(h),
                                                     ProvingKey.PRECOMPUTE if precompute else 0,
                                                     ctypes.byref(handle)))
        self.handle = handle

    def free(self):
        if self.handle:
            load_library().gm_g16_pk_free_multi(self.multi.handle, self.handle)
            self.handle = None

    def prove(self, wires, a, b, c, r: bytes, s: bytes):
        """(Ar, Bs, Krs) affine bytes; wires / a / b / c in host memory."""
        W, A, B, C, R, S = (_buf(x) for x in (wires, a, b, c, r, s))
        ar = np.zeros(point_bytes(self.curve, False), np.uint8)
        krs = np.zeros(point_bytes(self.curve, False), np.uint8)
        bs = np.zeros(point_bytes(self.curve, True), np.uint8)
        _check(load_library().gm_g16_prove_multi(self.multi.handle, self.handle, _p(W), _p(A), _p(B), _p(C),
                                                 A.size // FR_BYTES, _p(R), _p(S), _p(ar), _p(bs), _p(krs)))
        return ar.tobytes(), bs.tobytes(), krs.tobytes()


def device_count() -> int:
    n = ctypes.c_int()
    _check(load_library().gm_device_count(ctypes.byref(n)))
    return n.value


def g16_partial_bytes(curve) -> int:
    n = ctypes.c_size_t()
    _check(load_library().gm_g16_partial_bytes(curve_id(curve), ctypes.byref(n)))
    return n.value


def g16_reduce_partials(curve, partials) -> bytes:
    """Component-wise host sum of rank partials [A, B, K, Z (G1Jac), B2 (G2Jac)]."""
    j1, j2 = jac_bytes(curve, False), jac_bytes(curve, True)
    out = []
    for k in range(5):
        g2 = k == 4
        lo = 4 * j1 if g2 else k * j1
        sz = j2 if g2 else j1
        out.append(reduce_partials(curve, g2, [bytes(p)[lo:lo + sz] for p in partials]))
    return b"".join(out)


def g16_finish(curve, pk_host: "_PkHost", sums: bytes, r: bytes, s: bytes):
    """(Ar, Bs, Krs) affine bytes from summed partials (gm_g16_finish, host only)."""
    S, R, SS = _buf(sums), _buf(r), _buf(s)
    ar = np.zeros(point_bytes(curve, False), np.uint8)
    krs = np.zeros(point_bytes(curve, False), np.uint8)
    bs = np.zeros(point_bytes(curve, True), np.uint8)
    _check(load_library().gm_g16_finish(curve_id(curve), ctypes.byref(pk_host), _p(S), _p(R), _p(SS), _p(ar),
                                        _p(bs), _p(krs)))
    return ar.tobytes(), bs.tobytes(), krs.tobytes()


def sharded_prove(pk: ProvingKey, wires: DeviceBuffer, a: DeviceBuffer, b: DeviceBuffer, c: DeviceBuffer,
                  nb_constraints: int, r: bytes, s: bytes, group=None, device=None):
    """Multi-GPU Groth16 prove (BASELINE config 4): every rank computes its
    shard's five MSM sums, the fixed-size partials are all-gathered (RCCL over
    xGMI for backend "nccl", gloo on CPU) and every rank sums them and applies
    the blinding on the host.  Returns (Ar, Bs, Krs) on every rank."""
    local = pk.prove_partial_device(wires, a, b, c, nb_constraints)
    parts = allgather_partial(local, group=group, device=device)
    return g16_finish(pk.curve, pk._h, g16_reduce_partials(pk.curve, parts), r, s)
