// hp_sample.h -- the keystream layout of the device samplers (hp_sample.hip; include/hehub_amd.h: hp_dev_sample_*), as the kernels,
// the host implementation (hp_sample_host.cpp) and the Python model (tests/sample_model.py) share it.  No HIP here: every function is
// constexpr, which a plain C++ compiler takes as it is and the HIP compiler takes for host and device alike -- the kernels call
// exactly the code that tests/test_sample_host.py runs on the CPU (through tests/cpp/sample_shim.cpp).
//
// A sample is a function of (seed, stream) alone.  One ChaCha20 block (RFC 8439 section 2.3, 20 rounds) serves the 8 coefficients
// 8j .. 8j+7 of one row; its 16 state words:
//     0-3    the ChaCha constants
//     4-11   the 32 seed bytes as little-endian words
//     12     the block index j
//     13     attempt (bits 0-15) | kind << 16 (bits 16-23) | limb_id << 24 (bits 24-31)
//     14,15  low / high half of the 64-bit polynomial id `stream`
// Coefficient 8j + c owns the 64-bit candidate v_c = o[2c] | o[2c+1] << 32 of the block's output words o[0..15].
#pragma once
#include <cstddef>
#include <cstdint>
#include <utility>

typedef uint64_t u64;
typedef uint32_t u32;

// the kind tag of word 13: the four samplers never share keystream under one (seed, stream)
constexpr u32 HP_SAMPLE_UNIFORM = 1, HP_SAMPLE_TERNARY = 2, HP_SAMPLE_CBD = 3, HP_SAMPLE_GAUSS = 4;
constexpr u32 HP_SAMPLE_ATTEMPTS = 64;                 // candidates a uniform word may use up: attempts 0 .. 63
constexpr u32 HP_SAMPLE_ETA = 21;                      // centred binomial: popcount of 21 bits minus popcount of the next 21
constexpr u64 HP_SAMPLE_MAX_SCALE = (u64)1 << 58;      // error_scale below this: 21 * scale (binomial), 30 * scale (Gaussian) fit an int64_t
constexpr u32 HP_SAMPLE_MAX_LIMB_ID = 256;

struct HpSampleSeed {
    u32 w[8];
};
constexpr HpSampleSeed hp_sample_seed(const uint8_t *bytes) {
    HpSampleSeed s = {};
    for (int i = 0; i < 8; i++)
        s.w[i] = (u32)bytes[4 * i] | (u32)bytes[4 * i + 1] << 8 | (u32)bytes[4 * i + 2] << 16 | (u32)bytes[4 * i + 3] << 24;
    return s;
}

constexpr u32 hp_sample_word13(u32 attempt, u32 kind, u32 limb_id) { return (attempt & 0xffffu) | kind << 16 | limb_id << 24; }

constexpr void hp_sample_state(const HpSampleSeed &seed, u32 j, u32 word13, u64 stream, u32 (&s)[16]) {
    s[0] = 0x61707865u; s[1] = 0x3320646eu; s[2] = 0x79622d32u; s[3] = 0x6b206574u;
    for (int i = 0; i < 8; i++) s[4 + i] = seed.w[i];
    s[12] = j;
    s[13] = word13;
    s[14] = (u32)stream;
    s[15] = (u32)(stream >> 32);
}

// rot(x, n): x rotated left by n bits -- the caller's, so that the kernel names the instruction it wants
struct HpRotl {
    constexpr u32 operator()(u32 x, int n) const { return x << n | x >> (32 - n); }
};
template <class Rot> constexpr void hp_chacha_quarter(u32 &a, u32 &b, u32 &c, u32 &d, Rot rot) {
    a += b; d = rot(d ^ a, 16);
    c += d; b = rot(b ^ c, 12);
    a += b; d = rot(d ^ a, 8);
    c += d; b = rot(b ^ c, 7);
}
template <class Rot> constexpr void hp_chacha20_block(const u32 (&in)[16], u32 (&out)[16], Rot rot) {
    u32 x0 = in[0], x1 = in[1], x2 = in[2], x3 = in[3], x4 = in[4], x5 = in[5], x6 = in[6], x7 = in[7];
    u32 x8 = in[8], x9 = in[9], x10 = in[10], x11 = in[11], x12 = in[12], x13 = in[13], x14 = in[14], x15 = in[15];
    for (int r = 0; r < 10; r++) {
        hp_chacha_quarter(x0, x4, x8, x12, rot);
        hp_chacha_quarter(x1, x5, x9, x13, rot);
        hp_chacha_quarter(x2, x6, x10, x14, rot);
        hp_chacha_quarter(x3, x7, x11, x15, rot);
        hp_chacha_quarter(x0, x5, x10, x15, rot);
        hp_chacha_quarter(x1, x6, x11, x12, rot);
        hp_chacha_quarter(x2, x7, x8, x13, rot);
        hp_chacha_quarter(x3, x4, x9, x14, rot);
    }
    out[0] = x0 + in[0]; out[1] = x1 + in[1]; out[2] = x2 + in[2]; out[3] = x3 + in[3];
    out[4] = x4 + in[4]; out[5] = x5 + in[5]; out[6] = x6 + in[6]; out[7] = x7 + in[7];
    out[8] = x8 + in[8]; out[9] = x9 + in[9]; out[10] = x10 + in[10]; out[11] = x11 + in[11];
    out[12] = x12 + in[12]; out[13] = x13 + in[13]; out[14] = x14 + in[14]; out[15] = x15 + in[15];
}

constexpr u64 hp_sample_candidate(const u32 (&o)[16], u32 c) { return (u64)o[2 * c] | (u64)o[2 * c + 1] << 32; }

// ---- uniform modulo q, 2 <= q < 2^63 ------------------------------------------------------------------------------------------------
// w = candidate & (2^bit_length(q) - 1), accepted when below q (always with probability >= 1/2); a rejected word takes the same
// candidate position of the same block index under attempt + 1.  The sequence is bounded: the candidate of attempt 63 is final,
// as w - q where it is rejected too (per word: probability < 2^-64).
constexpr u64 hp_sample_mask(u64 q) { return ~(u64)0 >> __builtin_clzll(q); }
// one candidate of a word's sequence; true: w is the word
constexpr bool hp_sample_uniform_take(u64 q, u64 mask, u64 candidate, u32 attempt, u64 &w) {
    w = candidate & mask;
    if (w < q) return true;
    if (attempt + 1 < HP_SAMPLE_ATTEMPTS) return false;
    w -= q;
    return true;
}
// the word of a whole candidate sequence, next(attempt) its candidates in order
template <class Next> constexpr u64 hp_sample_uniform_word(u64 q, Next next) {
    const u64 mask = hp_sample_mask(q);
    u64 w = 0;
    for (u32 attempt = 0; attempt < HP_SAMPLE_ATTEMPTS; attempt++)
        if (hp_sample_uniform_take(q, mask, next(attempt), attempt, w)) break;
    return w;
}

// ---- ternary: the first of the candidate's 32 two-bit fields, from the low end, that is not 3, minus 1; 0 when all are 3 ------------------
constexpr int64_t hp_sample_ternary_word(u64 v) {
    const u64 t = ~v, not3 = (t | t >> 1) & 0x5555555555555555ull;   // bit 2f set: field f != 3
    if (not3 == 0) return 0;
    return (int64_t)(v >> __builtin_ctzll(not3) & 3u) - 1;
}

// ---- centred binomial, eta = 21: range +-21, variance 10.5 -------------------------------------------------------------------------------
constexpr int64_t hp_sample_cbd_word(u64 v) {
    const u64 m = ((u64)1 << HP_SAMPLE_ETA) - 1;
    return (int64_t)__builtin_popcountll(v & m) - (int64_t)__builtin_popcountll(v >> HP_SAMPLE_ETA & m);
}

// ---- discrete Gaussian, sigma = 16/5: range +-30, variance 10.24 ------------------------------------------------------------------------------
// rho(k) = exp(-25 k^2 / 512), S = the sum of rho over all integers; the magnitude m has P(0) = rho(0) / S, P(m) = 2 rho(m) / S.
// HP_SAMPLE_GAUSS_CDT[m] = floor(2^63 * (P(0) + .. + P(m))), m = 0 .. 29: entry 29 is 2^63 - 1 and every further one would be too.
// (tests/gauss_model.py recomputes the literals in decimal arithmetic.)  The candidate's bit 0 is the sign, u = its other 63 bits,
// m = the number of entries u has reached: statistical distance to D_{Z,3.2} below 2^-57.  All 30 compares, whatever the value:
// nothing to diverge on.  The count is a fold over the index pack, unrolled by the language and not by an optimiser's choice: every
// entry is a literal of its compare instruction -- no table in memory.
constexpr u32 HP_SAMPLE_GAUSS_ENTRIES = 30;
constexpr u64 HP_SAMPLE_GAUSS_CDT[HP_SAMPLE_GAUSS_ENTRIES] = {
    1149872835429266008ull, 3340023666152832877ull, 5231742854224525755ull, 6713673034491318533ull, 7766573326200196558ull,
    8445050402542556633ull, 8841576285654612683ull, 9051758678878186096ull, 9152802451769415979ull, 9196859074767746705ull,
    9214281206174004120ull, 9220529764022708440ull, 9222562339745873205ull, 9223161995634596963ull, 9223322447917711088ull,
    9223361386320111732ull, 9223369956674611011ull, 9223371667508612690ull, 9223371977254386295ull, 9223372028116140532ull,
    9223372035690845298ull, 9223372036713969870ull, 9223372036839307001ull, 9223372036853232777ull, 9223372036854636067ull,
    9223372036854764319ull, 9223372036854774950ull, 9223372036854775749ull, 9223372036854775804ull, 9223372036854775807ull};
template <u32... I> constexpr u32 hp_sample_gauss_count(u64 u, std::integer_sequence<u32, I...>) {
    return (0u + ... + (u32)(u >= HP_SAMPLE_GAUSS_CDT[I]));
}
constexpr int64_t hp_sample_gauss_word(u64 v) {
    const u32 m = hp_sample_gauss_count(v >> 1, std::make_integer_sequence<u32, HP_SAMPLE_GAUSS_ENTRIES>{});
    const u32 s = (u32)v & 1u;   // the conditional negation on the 32-bit count: (m ^ -s) + s
    return (int64_t)(int32_t)((m ^ (0u - s)) + s);
}

// ---- a scaled small coefficient as the canonical residue modulo q (k_sample_spread, hp_dev_sample_small_ntt) ---------------------------------
// v = scale * (a ternary, binomial or Gaussian word), |v| <= 30 * scale < 2^63: the magnitude modulo q, then the conditional negation
// q - r, where r = 0 stays 0 (hp_dev_poly_from_signed's rule).  The magnitude is below q whenever 30 * scale < q -- the usual case,
// no division; either way the same word.
constexpr u64 hp_sample_residue(int64_t v, u64 q) {
    const bool neg = v < 0;
    const u64 a = neg ? (u64)0 - (u64)v : (u64)v;
    const u64 r = a < q ? a : a % q;
    return (neg && r) ? q - r : r;
}
constexpr int64_t hp_sample_small_word(u32 kind, u64 candidate) {
    return kind == HP_SAMPLE_TERNARY ? hp_sample_ternary_word(candidate)
           : kind == HP_SAMPLE_GAUSS ? hp_sample_gauss_word(candidate)
                                     : hp_sample_cbd_word(candidate);
}

// ---- the samplers on the host (hp_sample_host.cpp): what the kernels of hp_sample.hip write, word for word --------------------------------------
namespace hpi {
// kind: HP_SAMPLE_TERNARY, HP_SAMPLE_CBD or HP_SAMPLE_GAUSS; out [batch][L][N]: hp_sample_residue of scale * the sample of id stream + b * id_step in
// every modulus -- the coefficient rows k_sample_spread writes, before the transform
void sample_small_host(u32 kind, size_t logn, size_t L, const u64 *moduli, size_t batch, const uint8_t *seed, u64 stream, u64 id_step,
                       int64_t scale, u64 *out);
// polynomial b of a call has the id stream + b; row m of it (modulus moduli[m], label limb_ids[m], or m where limb_ids == NULL)
// goes to out + b * stride_words + m * N
void sample_uniform_host(size_t logn, size_t L, const u64 *moduli, const u32 *limb_ids, size_t batch, const uint8_t *seed, u64 stream,
                         size_t stride_words, u64 *out);
// kind: HP_SAMPLE_TERNARY, HP_SAMPLE_CBD or HP_SAMPLE_GAUSS; out [batch][N], every value times scale
void sample_signed_host(u32 kind, size_t logn, size_t batch, const uint8_t *seed, u64 stream, int64_t scale, int64_t *out);
} // namespace hpi
