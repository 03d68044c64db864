// lincomb_shim.cpp -- a C entry point around hpi::lincomb_max_terms (hehub_amd/csrc/hp_drop.cpp) so the CPU test-suite can reach the
// moduli no GPU test uses (tests/test_lincomb_host.py).  Test infrastructure only.
#include "../../hehub_amd/csrc/hp_drop.h"

extern "C" size_t lc_max_terms(const uint64_t *moduli, size_t L, size_t table_max) {
    return hpi::lincomb_max_terms(moduli, L, table_max);
}
