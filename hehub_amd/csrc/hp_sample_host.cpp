// hp_sample_host.cpp -- the four samplers of hp_sample.h on the host: one ChaCha20 block per 8 coefficients, the rules of the header.
// No HIP, no context; plain C++ (tests/cpp/sample_shim.cpp builds it with g++).  No entry point of the library calls these --
// there is no CPU fallback -- they are what tests/test_sample_host.py holds against the Python model, rule by rule.
#include "hp_sample.h"

namespace hpi {

void sample_uniform_host(size_t logn, size_t L, const u64 *moduli, const u32 *limb_ids, size_t batch, const uint8_t *seed, u64 stream,
                         size_t stride_words, u64 *out) {
    const size_t n = (size_t)1 << logn, stride = stride_words ? stride_words : L * n;
    const HpSampleSeed sd = hp_sample_seed(seed);
    for (size_t b = 0; b < batch; b++)
        for (size_t m = 0; m < L; m++) {
            const u64 q = moduli[m];
            const u32 id = limb_ids ? limb_ids[m] : (u32)m;
            for (size_t j = 0; j < n / 8; j++)
                for (u32 c = 0; c < 8; c++)   // (a block per word and attempt: this is the definition, not the fast way)
                    out[b * stride + m * n + 8 * j + c] = hp_sample_uniform_word(q, [&](u32 attempt) {
                        u32 st[16] = {}, o[16] = {};
                        hp_sample_state(sd, (u32)j, hp_sample_word13(attempt, HP_SAMPLE_UNIFORM, id), stream + b, st);
                        hp_chacha20_block(st, o, HpRotl{});
                        return hp_sample_candidate(o, c);
                    });
        }
}

void sample_signed_host(u32 kind, size_t logn, size_t batch, const uint8_t *seed, u64 stream, int64_t scale, int64_t *out) {
    const size_t n = (size_t)1 << logn;
    const HpSampleSeed sd = hp_sample_seed(seed);
    for (size_t b = 0; b < batch; b++)
        for (size_t j = 0; j < n / 8; j++) {
            u32 st[16] = {}, o[16] = {};
            hp_sample_state(sd, (u32)j, hp_sample_word13(0, kind, 0), stream + b, st);
            hp_chacha20_block(st, o, HpRotl{});
            for (u32 c = 0; c < 8; c++) {
                out[b * n + 8 * j + c] = scale * hp_sample_small_word(kind, hp_sample_candidate(o, c));
            }
        }
}

void sample_small_host(u32 kind, size_t logn, size_t L, const u64 *moduli, size_t batch, const uint8_t *seed, u64 stream, u64 id_step,
                       int64_t scale, u64 *out) {
    const size_t n = (size_t)1 << logn;
    const HpSampleSeed sd = hp_sample_seed(seed);
    for (size_t b = 0; b < batch; b++)
        for (size_t j = 0; j < n / 8; j++) {
            u32 st[16] = {}, o[16] = {};
            hp_sample_state(sd, (u32)j, hp_sample_word13(0, kind, 0), stream + b * id_step, st);
            hp_chacha20_block(st, o, HpRotl{});
            for (u32 c = 0; c < 8; c++) {
                const int64_t v = scale * hp_sample_small_word(kind, hp_sample_candidate(o, c));
                for (size_t m = 0; m < L; m++) out[(b * L + m) * n + 8 * j + c] = hp_sample_residue(v, moduli[m]);
            }
        }
}

} // namespace hpi
