// Pairing, BLS12-381: the instantiations of pairing_impl.hpp.
#include "pairing_impl.hpp"

namespace gm {
GM_PR_INSTANTIATE(CurveBLS12381)
}  // namespace gm
