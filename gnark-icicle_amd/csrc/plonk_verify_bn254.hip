// KZG and PLONK verification, BN254: the instantiations of plonk_verify_impl.hpp.
#include "plonk_verify_impl.hpp"

namespace gm {
GM_PV_INSTANTIATE(CurveBN254)
}  // namespace gm
