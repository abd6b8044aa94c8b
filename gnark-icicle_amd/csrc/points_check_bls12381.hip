// Point check, BLS12-381: the G1 and G2 instantiations of points_check_impl.hpp.
#include "points_check_impl.hpp"

namespace gm {
GM_PC_INSTANTIATE(CurveBLS12381)
}  // namespace gm
