// bfv_shim.cpp -- C entry points around hehub_amd/csrc/hp_bfv.h so the CPU test-suite can check the host's base-size decision and every
// constant of the BFV kernels without a GPU.  Test infrastructure only.
#include "../../hehub_amd/csrc/hp_bfv.h"

#include <cstring>

using namespace hpi;

extern "C" {

int bs_max() { return HP_BFV_MAX; }
size_t bs_consts_words() { return sizeof(HpBfvConsts) / 8; }
size_t bs_plain_words() { return sizeof(HpBfvPlain) / 8; }
size_t bs_dec_words() { return sizeof(HpBfvDecPlain) / 8; }

int bs_base_ok(const uint64_t *moduli_qb, size_t L, size_t M, uint64_t t, uint64_t n) { return bfv_base_ok(moduli_qb, L, M, t, n) ? 1 : 0; }

// HpBfvConsts as it lies in memory: one word (L, M), q2b, b2q (inv, inv_h, half, pref, pref_h, prod each), qinv_b, qinv_b_h, h_mod
int bs_consts(const uint64_t *moduli_qb, size_t L, size_t M, uint64_t *out) {
    HpBfvConsts c;
    const bool ok = bfv_build_consts(moduli_qb, L, M, c);
    std::memcpy(out, &c, sizeof(c));
    return ok ? 1 : 0;
}

void bs_plain(const uint64_t *moduli_qb, size_t cnt, uint64_t t, uint64_t *out) {
    HpBfvPlain p;
    bfv_plain(moduli_qb, cnt, t, p);
    std::memcpy(out, &p, sizeof(p));
}

int bs_dec_plain(const uint64_t *q, size_t L, uint64_t t, uint64_t *out) {
    HpBfvDecPlain p;
    const bool ok = bfv_dec_plain(q, L, t, p);
    std::memcpy(out, &p, sizeof(p));
    return ok ? 1 : 0;
}

uint64_t bs_inverse(uint64_t a, uint64_t m) { return bfv_inverse(a, m); }

} // extern "C"
