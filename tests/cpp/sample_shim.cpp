// sample_shim.cpp -- C entry points around the sampling layout (hehub_amd/csrc/hp_sample.h) and its host implementation
// (hp_sample_host.cpp) so the CPU test-suite can hold them against tests/sample_model.py (tests/test_sample_host.py).  The kernels of
// hp_sample.hip call the same functions.  Test infrastructure only; plain g++.
#include "../../hehub_amd/csrc/hp_sample.h"

extern "C" {

unsigned ss_word13(unsigned attempt, unsigned kind, unsigned limb_id) { return hp_sample_word13(attempt, kind, limb_id); }

// the output words of the block (seed, j, word 13, stream)
void ss_block(const uint8_t *seed, unsigned j, unsigned word13, uint64_t stream, uint32_t *out) {
    u32 st[16] = {}, o[16] = {};
    hp_sample_state(hp_sample_seed(seed), j, word13, stream, st);
    hp_chacha20_block(st, o, HpRotl{});
    for (int i = 0; i < 16; i++) out[i] = o[i];
}

// the block of a caller's state, as RFC 8439's test vector gives it
void ss_block_of_state(const uint32_t *state, uint32_t *out) {
    u32 st[16] = {}, o[16] = {};
    for (int i = 0; i < 16; i++) st[i] = state[i];
    hp_chacha20_block(st, o, HpRotl{});
    for (int i = 0; i < 16; i++) out[i] = o[i];
}

uint64_t ss_candidate(const uint32_t *o16, unsigned c) {
    u32 o[16] = {};
    for (int i = 0; i < 16; i++) o[i] = o16[i];
    return hp_sample_candidate(o, c);
}

// the uniform word rule on a planted candidate sequence of HP_SAMPLE_ATTEMPTS entries; *used = candidates looked at
uint64_t ss_uniform_word(uint64_t q, const uint64_t *cands, unsigned *used) {
    unsigned n = 0;
    const u64 w = hp_sample_uniform_word(q, [&](u32 attempt) { n++; return cands[attempt]; });
    *used = n;
    return w;
}
long long ss_ternary_word(uint64_t v) { return hp_sample_ternary_word(v); }
long long ss_cbd_word(uint64_t v) { return hp_sample_cbd_word(v); }

void ss_uniform(size_t logn, size_t L, const uint64_t *moduli, const uint32_t *limb_ids, size_t batch, const uint8_t *seed, uint64_t stream,
                size_t stride_words, uint64_t *out) {
    hpi::sample_uniform_host(logn, L, moduli, limb_ids, batch, seed, stream, stride_words, out);
}
void ss_signed(unsigned kind, size_t logn, size_t batch, const uint8_t *seed, uint64_t stream, long long scale, long long *out) {
    hpi::sample_signed_host(kind, logn, batch, seed, stream, scale, (int64_t *)out);
}

} // extern "C"
