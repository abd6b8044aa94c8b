// Point codec, BLS12-381: the G1 and G2 instantiations of points_codec_impl.hpp.
#include "points_codec_impl.hpp"

namespace gm {
GM_CD_INSTANTIATE(CurveBLS12381)
}  // namespace gm
