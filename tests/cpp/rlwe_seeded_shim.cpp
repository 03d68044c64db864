// rlwe_seeded_shim.cpp -- C entry points around the signed-to-residue rule of hehub_amd/csrc/hp_sample.h and the host twin of
// k_sample_spread (hp_sample_host.cpp), for tests/test_rlwe_seeded_host.py.  The kernel calls the same hp_sample_residue.  Test
// infrastructure only; plain g++.
#include "../../hehub_amd/csrc/hp_sample.h"

// the rule is constexpr: the compiler itself holds it to a few edges
static_assert(hp_sample_residue(0, 3) == 0 && hp_sample_residue(-1, 3) == 2 && hp_sample_residue(-3, 3) == 0 && hp_sample_residue(7, 3) == 1, "");

extern "C" {

uint64_t rs_residue(long long v, uint64_t q) { return hp_sample_residue(v, q); }

void rs_small(unsigned kind, size_t logn, size_t L, const uint64_t *moduli, size_t batch, const uint8_t *seed, uint64_t stream,
              uint64_t id_step, long long scale, uint64_t *out) {
    hpi::sample_small_host(kind, logn, L, moduli, batch, seed, stream, id_step, scale, out);
}

} // extern "C"
