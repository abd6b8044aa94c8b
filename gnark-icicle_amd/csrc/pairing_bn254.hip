// Pairing, BN254: the instantiations of pairing_impl.hpp.
#include "pairing_impl.hpp"

namespace gm {
GM_PR_INSTANTIATE(CurveBN254)
}  // namespace gm
