// gauss_shim.cpp -- C entry points around the discrete Gaussian rule of hehub_amd/csrc/hp_sample.h (kind 4: the table's literals, the
// word rule) and the host samplers of hp_sample_host.cpp under that kind, so the CPU test-suite can hold them against
// tests/gauss_model.py (tests/test_gauss_host.py).  The kernels of hp_sample.hip call the same functions.  Test infrastructure only;
// plain g++.
#include "../../hehub_amd/csrc/hp_sample.h"

// the rule is usable in a constant expression, as the header promises: zero carries no sign, the ends of the range
static_assert(hp_sample_gauss_word(0) == 0 && hp_sample_gauss_word(1) == 0, "zero carries no sign");
static_assert(hp_sample_gauss_word(~(u64)0) == -30 && hp_sample_gauss_word(~(u64)0 - 1) == 30, "the range is +-30");

extern "C" {

unsigned gs_kind(void) { return HP_SAMPLE_GAUSS; }
unsigned gs_entries(void) { return HP_SAMPLE_GAUSS_ENTRIES; }
uint64_t gs_table(unsigned i) { return HP_SAMPLE_GAUSS_CDT[i]; }
uint64_t gs_max_scale(void) { return HP_SAMPLE_MAX_SCALE; }
long long gs_gauss_word(uint64_t v) { return hp_sample_gauss_word(v); }
long long gs_small_word(unsigned kind, uint64_t v) { return hp_sample_small_word(kind, v); }

void gs_signed(unsigned kind, size_t logn, size_t batch, const uint8_t *seed, uint64_t stream, long long scale, long long *out) {
    hpi::sample_signed_host(kind, logn, batch, seed, stream, scale, (int64_t *)out);
}
void gs_small(unsigned kind, size_t logn, size_t L, const uint64_t *moduli, size_t batch, const uint8_t *seed, uint64_t stream,
              uint64_t id_step, long long scale, uint64_t *out) {
    hpi::sample_small_host(kind, logn, L, moduli, batch, seed, stream, id_step, scale, out);
}

} // extern "C"
