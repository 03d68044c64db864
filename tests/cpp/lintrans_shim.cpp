// lintrans_shim.cpp -- a C entry point around hpi::hks_lintrans_max_rotations (hehub_amd/csrc/hp_drop.cpp) so the CPU test-suite can
// reach the moduli no GPU test uses (tests/test_lintrans_host.py).  Test infrastructure only.
#include "../../hehub_amd/csrc/hp_drop.h"

extern "C" size_t ls_max_rotations(const uint64_t *mext, size_t E, size_t nd, size_t table_max) {
    return hpi::hks_lintrans_max_rotations(mext, E, nd, table_max);
}
