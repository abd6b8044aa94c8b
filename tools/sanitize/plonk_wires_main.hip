// Stand-alone sanitizer run of the host-side checks of gm_plonk_wires_upload
// (csrc/plonk_wires.hip): the three id loops, on a CPU, without a device.
//
//   hipcc -O1 -g --offload-arch=gfx950 -std=c++17 -Xarch_host -fsanitize=address,undefined \
//         tools/sanitize/plonk_wires_main.hip gnark-icicle_amd/csrc/plonk_wires.hip -o plonk_wires_san
//   HIP_VISIBLE_DEVICES=-1 ./plonk_wires_san
//
// Every refusal returns before the first device call.  Tables that pass the checks
// go on to the upload, which fails with GM_ERR_DEVICE where there is no device:
// the loops have then read all 3 n ids.  The tables are heap blocks of exactly n
// ids, so a read past either end is reported.
#include <cstdio>
#include <string>
#include <vector>

#include "../../gnark-icicle_amd/csrc/plonk_wires.hpp"
#include "../../gnark-icicle_amd/csrc/runtime.hpp"

static std::string g_err;
void gm::set_error(const std::string& msg) { g_err = msg; }

static int failures = 0;
static void expect(const char* what, int rc, int want, const char* needle) {
  const bool ok = rc == want && g_err.find(needle) != std::string::npos;
  printf("%-28s rc=%d  %s%s\n", what, rc, g_err.c_str(), ok ? "" : "   <-- UNEXPECTED");
  if (!ok) failures++;
  g_err.clear();
}

int main() {
  gm_ctx ctx;
  gm_plonk_wires* out = nullptr;
  for (size_t n : {size_t(8), size_t(1) << 16}) {
    std::vector<uint32_t> a(n), b(n), c(n);
    for (size_t i = 0; i < n; i++) {
      a[i] = (uint32_t)i;
      b[i] = (uint32_t)(n - 1 - i);
      c[i] = 0;
    }
    auto up = [&](size_t nn, size_t nw) { return gm::plonk_wires_upload(&ctx, nn, nw, a.data(), b.data(), c.data(), &out); };
    expect("n not a power of two", up(n - 1, n), GM_ERR_INVALID, "power of two");
    expect("n < 8", up(4, n), GM_ERR_INVALID, "power of two");
    expect("nb_wires = 0", up(n, 0), GM_ERR_INVALID, "nb_wires");
    expect("nb_wires = 2^32", up(n, size_t(1) << 32), GM_ERR_INVALID, "nb_wires");
    expect("last id of xa too large", up(n, n - 1), GM_ERR_INVALID, ("xa[" + std::to_string(n - 1) + "]").c_str());
    c[n - 1] = (uint32_t)n;
    expect("last id of xc too large", up(n, n), GM_ERR_INVALID, ("xc[" + std::to_string(n - 1) + "]").c_str());
    c[n - 1] = 0;
    b[0] = 0xffffffffu;
    expect("first id of xb = 2^32 - 1", up(n, 0xffffffffull), GM_ERR_INVALID, "xb[0]");
    b[0] = (uint32_t)(n - 1);
    // all ids pass: the upload itself needs a device
    expect("valid tables, no device", up(n, n), GM_ERR_DEVICE, "");
  }
  printf(failures ? "FAILED\n" : "ok\n");
  return failures ? 1 : 0;
}
