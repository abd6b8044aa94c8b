// Pippenger MSM instantiation: CurveBLS12381 G1 (templates in msm_impl.hpp).
// 14 limbs, as BLS12-377: the two-wave prefetching accumulation k_msm_accum_seg_pf4.
#include "msm_impl.hpp"

namespace gm {
GM_MSM_INSTANTIATE(CurveBLS12381, false)
GM_MSM_INSTANTIATE_PLAN(CurveBLS12381)
}  // namespace gm
