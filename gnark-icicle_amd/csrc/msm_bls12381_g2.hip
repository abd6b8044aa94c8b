// Pippenger MSM instantiation: CurveBLS12381 G2 (templates in msm_impl.hpp).
// Lane-pair kernels at two waves per SIMD, as BLS12-377 G2 (msm_bls12377_g2.hip):
// the 14-limb pair add does not fit three.  Fp2 = Fp[u]/(u^2 + 1) at 14 limbs
// takes the unsigned forms throughout: pf2_mul's a0 b0 + (5p - a1) b1 in one
// fe_mul2_redc_u, and the two-product Y3 (the signed four-product reduction,
// fe_mul4_redc, holds its columns only up to 9 limbs).
#ifndef GM_PAIR_WPE
#define GM_PAIR_WPE 2
#endif
#include "msm_impl.hpp"

namespace gm {
GM_MSM_INSTANTIATE(CurveBLS12381, true)
}  // namespace gm
