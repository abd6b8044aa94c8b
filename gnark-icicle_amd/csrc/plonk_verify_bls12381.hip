// KZG and PLONK verification, BLS12-381: the instantiations of plonk_verify_impl.hpp.
#include "plonk_verify_impl.hpp"

namespace gm {
GM_PV_INSTANTIATE(CurveBLS12381)
}  // namespace gm
