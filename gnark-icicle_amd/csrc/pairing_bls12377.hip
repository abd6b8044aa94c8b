// Pairing, BLS12-377: the instantiations of pairing_impl.hpp.
#include "pairing_impl.hpp"

namespace gm {
GM_PR_INSTANTIATE(CurveBLS12377)
}  // namespace gm
