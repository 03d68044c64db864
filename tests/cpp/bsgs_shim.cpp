// bsgs_shim.cpp -- a C entry point around hpi::hks_bsgs_plan (hehub_amd/csrc/hp_drop.cpp): the pass plan and the workspace of
// hp_dev_ckks_lintrans_bsgs_hks, so the CPU test-suite can reach the moduli no GPU test uses (tests/test_bsgs_host.py).
// Test infrastructure only.
#include "../../hehub_amd/csrc/hp_drop.h"

// out[0..5) = baby_pass, giant_pass, presum_giants, overlay_words, words; returns 1 where the plan exists
extern "C" int bs_plan(const uint64_t *mext, size_t n, size_t L, size_t k, size_t alpha, size_t batch, size_t babies, size_t giants,
                       size_t *out) {
    hpi::HksBsgsPlan p;
    const bool ok = hpi::hks_bsgs_plan(mext, n, L, k, alpha, batch, babies, giants, p);
    out[0] = p.baby_pass; out[1] = p.giant_pass; out[2] = p.presum_giants; out[3] = p.overlay_words; out[4] = p.words;
    return ok ? 1 : 0;
}
