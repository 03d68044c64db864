// hp_sample.hip -- the device samplers (hp_dev_sample_*, the seeded key generators): a counter-based ChaCha20 keystream turned into
// uniform residues, ternary and centred-binomial coefficients.  hp_sample.h has the stream layout and every rule; the kernels call
// those functions as they are.
//
// One thread = one ChaCha20 block = 8 consecutive coefficients of one row = 64 bytes, written as four non-temporal 16-byte stores
// (written once, far more data than L2 holds).  Pure VALU: add / xor / rotate on 16 registers, no LDS, no inline assembly; seed,
// constants and the row table are kernel arguments.  The block is about 1000 VALU operations per lane for 64 bytes, which makes the
// kernel VALU-bound well below HBM speed (DESIGN 4.7 has the measured rate): the store pattern is not what limits it.
// A uniform word whose candidate is rejected recomputes the block under the next attempt.  The loop is bounded by the layout itself
// (hp_sample_uniform_take ends every word at attempt 63): no thread ever waits on data.
#include "hp_elem.h"
#include "hp_sample.h"

#define SAMPLE_THREADS 256

struct RotV {   // v_alignbit_b32
    constexpr u32 operator()(u32 x, int n) const { return __builtin_rotateleft32(x, (u32)n); }
};

// thread t of a launch: block j of row t >> logb (logb = log2 of the blocks per row)
HP_DEV bool sample_item(u64 total, u32 logb, u64 &row, u32 &j) {
    const u64 t = (u64)blockIdx.x * SAMPLE_THREADS + threadIdx.x;
    row = t >> logb;
    j = (u32)(t & (((u64)1 << logb) - 1));
    return t < total;
}

// MONT: the word times 2^64 mod q, canonical -- the form hp_dev_hks_keygen leaves a key's a-half in (k_hks_keygen's own expression)
template <bool MONT>
__global__ void __launch_bounds__(SAMPLE_THREADS) k_sample_uniform(HpSampleSeed seed, HpSampleRows rows, const HpLimb *__restrict__ limbs,
                                                                 u32 L, u32 logb, u64 total, u64 stream, u64 stride, u64 *__restrict__ out) {
    u64 row;
    u32 j;
    if (!sample_item(total, logb, row, j)) return;
    const u64 b = row / L;
    const u32 m = (u32)(row % L);
    const u64 q = rows.q[m], mask = hp_sample_mask(q);
    const u32 id = rows.id[m];
    u32 st[16], o[16];
    hp_sample_state(seed, j, hp_sample_word13(0, HP_SAMPLE_UNIFORM, id), stream + b, st);
    hp_chacha20_block(st, o, RotV{});
    u64 w[8];
    u32 pending = 0;
#pragma unroll
    for (u32 c = 0; c < 8; c++)
        if (!hp_sample_uniform_take(q, mask, hp_sample_candidate(o, c), 0, w[c])) pending |= 1u << c;
    for (u32 attempt = 1; pending && attempt < HP_SAMPLE_ATTEMPTS; attempt++) {
        st[13] = hp_sample_word13(attempt, HP_SAMPLE_UNIFORM, id);
        hp_chacha20_block(st, o, RotV{});
#pragma unroll
        for (u32 c = 0; c < 8; c++) {
            u64 v;
            if ((pending >> c & 1u) && hp_sample_uniform_take(q, mask, hp_sample_candidate(o, c), attempt, v)) {
                w[c] = v;
                pending &= ~(1u << c);
            }
        }
    }
    if (MONT) {
        const u64 r64 = limbs[m].r64, r64h = limbs[m].r64h;
#pragma unroll
        for (u32 c = 0; c < 8; c++) w[c] = hp_strict(hp_harvey_lazy(w[c], r64, r64h, q), q);
    }
    u64 *dst = out + b * stride + ((u64)m << (logb + 3)) + ((u64)j << 3);
#pragma unroll
    for (u32 c = 0; c < 8; c += 2) st_nt(dst + c, U2{w[c], w[c + 1]});
}

template <u32 KIND>
__global__ void __launch_bounds__(SAMPLE_THREADS) k_sample_signed(HpSampleSeed seed, u32 logb, u64 total, u64 stream, long long scale,
                                                                long long *__restrict__ out) {
    u64 b;
    u32 j;
    if (!sample_item(total, logb, b, j)) return;
    u32 st[16], o[16];
    hp_sample_state(seed, j, hp_sample_word13(0, KIND, 0), stream + b, st);
    hp_chacha20_block(st, o, RotV{});
    u64 w[8];
#pragma unroll
    for (u32 c = 0; c < 8; c++) {
        const u64 v = hp_sample_candidate(o, c);
        w[c] = (u64)(scale * (KIND == HP_SAMPLE_TERNARY ? hp_sample_ternary_word(v) : hp_sample_cbd_word(v)));
    }
    u64 *dst = reinterpret_cast<u64 *>(out) + (b << (logb + 3)) + ((u64)j << 3);
#pragma unroll
    for (u32 c = 0; c < 8; c += 2) st_nt(dst + c, U2{w[c], w[c + 1]});
}

template <class... KA, class... A>
static inline hipError_t sample_launch(void (*k)(KA...), u64 total, hipStream_t stream, const A &...args) {
    const u64 blocks = (total + SAMPLE_THREADS - 1) / SAMPLE_THREADS;
    if (blocks == 0 || blocks > HP_SAMPLE_MAX_BLOCKS) return hipErrorInvalidValue;
    k<<<dim3((u32)blocks, 1, 1), SAMPLE_THREADS, 0, stream>>>(args...);
    return hipGetLastError();
}

hipError_t hp_launch_sample_uniform(const HpSampleSeed &seed, const HpSampleRows &rows, const HpLimb *mont_limbs, u32 L, u32 logn, u64 batch,
                                    u64 stream_id, u64 stride, u64 *out, hipStream_t stream) {
    if (logn < 3 || L < 1 || L > HP_MAX_LIMBS) return hipErrorInvalidValue;
    const u32 logb = logn - 3;
    const u64 total = (batch * L) << logb;
    if (mont_limbs) return sample_launch(k_sample_uniform<true>, total, stream, seed, rows, mont_limbs, L, logb, total, stream_id, stride, out);
    return sample_launch(k_sample_uniform<false>, total, stream, seed, rows, mont_limbs, L, logb, total, stream_id, stride, out);
}

hipError_t hp_launch_sample_signed(u32 kind, const HpSampleSeed &seed, u32 logn, u64 batch, u64 stream_id, long long scale, long long *out,
                                   hipStream_t stream) {
    if (logn < 3) return hipErrorInvalidValue;
    const u32 logb = logn - 3;
    const u64 total = batch << logb;
    if (kind == HP_SAMPLE_TERNARY) return sample_launch(k_sample_signed<HP_SAMPLE_TERNARY>, total, stream, seed, logb, total, stream_id, scale, out);
    if (kind == HP_SAMPLE_CBD) return sample_launch(k_sample_signed<HP_SAMPLE_CBD>, total, stream, seed, logb, total, stream_id, scale, out);
    return hipErrorInvalidValue;
}
