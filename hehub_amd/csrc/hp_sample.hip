// hp_sample.hip -- the device samplers (hp_dev_sample_*, the seeded key generators): a counter-based ChaCha20 keystream turned into
// uniform residues, ternary, centred-binomial and discrete Gaussian coefficients.  hp_sample.h has the stream layout and every rule;
// the kernels call those functions as they are.  Further down, the kernels of the seeded ciphertext calls
// (hp_dev_sample_small_ntt, hp_dev_rlwe_encrypt_seeded, hp_dev_rlwe_encrypt_pk_seeded) over the same blocks.
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
    for (u32 c = 0; c < 8; c++) w[c] = (u64)(scale * hp_sample_small_word(KIND, hp_sample_candidate(o, c)));
    u64 *dst = reinterpret_cast<u64 *>(out) + (b << (logb + 3)) + ((u64)j << 3);
#pragma unroll
    for (u32 c = 0; c < 8; c += 2) st_nt(dst + c, U2{w[c], w[c + 1]});
}

// ---- fresh ciphertexts (hp_dev_sample_small_ntt, hp_dev_rlwe_encrypt_seeded, hp_dev_rlwe_encrypt_pk_seeded) ---------------------------------
// A small polynomial straight to the residues of all L moduli: the block is computed once and its 8 scaled coefficients stay in
// registers while the thread walks the moduli -- no int64 row crosses HBM.  Polynomial p has the id stream + p * id_step and its
// rows at out + p * pstride + m * N.  The forward transform reads the rows next: ordinary 16-byte stores.
template <u32 KIND>
HP_DEV void sample_spread_item(const HpSampleSeed &seed, const HpSampleRows &rows, u32 L, u32 logb, u64 total, u64 stream, u64 id_step,
                               long long scale, u64 pstride, u64 *__restrict__ out) {
    u64 p;
    u32 j;
    if (!sample_item(total, logb, p, j)) return;
    u32 st[16], o[16];
    hp_sample_state(seed, j, hp_sample_word13(0, KIND, 0), stream + p * id_step, st);
    hp_chacha20_block(st, o, RotV{});
    long long v[8];
#pragma unroll
    for (u32 c = 0; c < 8; c++) v[c] = scale * hp_sample_small_word(KIND, hp_sample_candidate(o, c));
    u64 *dst = out + p * pstride + ((u64)j << 3);
    for (u32 m = 0; m < L; m++, dst += (u64)8 << logb) {
        const u64 q = rows.q[m];
#pragma unroll
        for (u32 c = 0; c < 8; c += 2) *reinterpret_cast<U2 *>(dst + c) = U2{hp_sample_residue(v[c], q), hp_sample_residue(v[c + 1], q)};
    }
}
// ternary and centred binomial: what hp_dev_sample_small_ntt takes, and the errors of the default sampler
template <u32 KIND>
__global__ void __launch_bounds__(SAMPLE_THREADS) k_sample_spread(HpSampleSeed seed, HpSampleRows rows, u32 L, u32 logb, u64 total, u64 stream,
                                                                u64 id_step, long long scale, u64 pstride, u64 *__restrict__ out) {
    static_assert(KIND == HP_SAMPLE_TERNARY || KIND == HP_SAMPLE_CBD, "the Gaussian rows have a kernel of their own");
    sample_spread_item<KIND>(seed, rows, L, logb, total, stream, id_step, scale, pstride, out);
}
// the error rows of the seeded ciphertext calls under the Gaussian error sampler (hp_ctx_set_error_sampler): the same thread, the
// 30-entry compare chain of hp_sample_gauss_word in place of the popcounts
__global__ void __launch_bounds__(SAMPLE_THREADS) k_gauss_spread(HpSampleSeed seed, HpSampleRows rows, u32 L, u32 logb, u64 total, u64 stream,
                                                               u64 id_step, long long scale, u64 pstride, u64 *__restrict__ out) {
    sample_spread_item<HP_SAMPLE_GAUSS>(seed, rows, L, logb, total, stream, id_step, scale, pstride, out);
}

// the 8 uniform words of block j of a row: k_sample_uniform's draw and bounded redraw loop, statement for statement (that kernel
// keeps its own copy: its code is what the sampler measurements were taken on)
HP_DEV void sample_uniform_block(const HpSampleSeed &seed, u64 q, u32 id, u32 j, u64 stream, u64 (&w)[8]) {
    const u64 mask = hp_sample_mask(q);
    u32 st[16], o[16];
    hp_sample_state(seed, j, hp_sample_word13(0, HP_SAMPLE_UNIFORM, id), stream, st);
    hp_chacha20_block(st, o, RotV{});
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
}

// Seeded secret-key encryption, one thread = the 8 words 8j .. 8j+7 of row (b, m): a = the uniform sample, drawn in registers and
// never read from memory; c0 = NTT(e) + NTT(pt) - a * s, canonical, where NTT(e) lies in the c0 row on entry (any lazy transform
// word) and NTT(pt) in the rows ptn + b * pt_stride (with WITH_C1 these may be the c1 rows themselves: the thread has read its 8
// words before it stores a over them, so neither ptn nor ct is __restrict__).  Ciphertext b at ct + b * (WITH_C1 ? 2 : 1) * L * N.
// c0 / c1 are written once: non-temporal stores, as in k_sample_uniform.  The loads are ORDINARY: a lane's four 16-byte loads of a
// row fall into one 128-byte line, which it shares with its neighbour, and with non-temporal loads the line was fetched again for
// every one of them (measured at N = 32768, L = 10, batch 64: 0.636 ms against 0.225 ms).
template <bool WITH_C1, bool HAS_PT>
__global__ void __launch_bounds__(SAMPLE_THREADS) k_enc_seeded(HpSampleSeed seed, HpSampleRows rows, const HpLimb *__restrict__ limbs, u32 L,
                                                             u32 logb, u64 total, u64 stream, const u64 *__restrict__ sk, const u64 *ptn,
                                                             u64 pt_stride, u64 *ct) {
    u64 row;
    u32 j;
    if (!sample_item(total, logb, row, j)) return;
    const u64 b = row / L;
    const u32 m = (u32)(row % L);
    u64 a[8];
    sample_uniform_block(seed, rows.q[m], rows.id[m], j, stream + b, a);
    const HpLimb lm = limbs[m];
    const u64 off = ((u64)m << (logb + 3)) + ((u64)j << 3);
    u64 *c0 = ct + b * (((u64)(WITH_C1 ? 2 : 1) * L) << (logb + 3)) + off;
    const u64 *s = sk + off, *t = HAS_PT ? ptn + b * pt_stride + off : nullptr;
    const auto fin = [&](u64 ev, u64 av, u64 sw, u64 tw) {
        u64 v = hp_sub_lazy(hp_lazy_below_2q(ev, lm.two_q), hp_mul_hybrid_lazy(av, sw, lm), lm.two_q);
        if (HAS_PT) v = hp_add_lazy(v, hp_lazy_below_2q(tw, lm.two_q), lm.two_q);
        return hp_strict(v, lm.q);
    };
    // two halves of 4 words: 12 operand words in flight beside the 8 of a, which keeps the kernel at eight waves per SIMD (the block
    // is what the thread spends its time on; the other waves cover the loads)
#pragma unroll
    for (u32 h = 0; h < 8; h += 4) {
        U2 e[2], sv[2], tv[2];
#pragma unroll
        for (u32 c = 0; c < 2; c++) {
            e[c] = *reinterpret_cast<const U2 *>(c0 + h + 2 * c);
            sv[c] = *reinterpret_cast<const U2 *>(s + h + 2 * c);
            if (HAS_PT) tv[c] = *reinterpret_cast<const U2 *>(t + h + 2 * c);
        }
#pragma unroll
        for (u32 c = 0; c < 2; c++) {
            const u32 i = h + 2 * c;
            st_nt(c0 + i, U2{fin(e[c].x, a[i], sv[c].x, HAS_PT ? tv[c].x : 0), fin(e[c].y, a[i + 1], sv[c].y, HAS_PT ? tv[c].y : 0)});
            if (WITH_C1) st_nt(c0 + ((u64)L << (logb + 3)) + i, U2{a[i], a[i + 1]});
        }
    }
}

// Public-key encryption, the last step (tile skeleton of hp_elem.h, row = b * L + m): ct[b][0] = pk0 * u + e0 (+ pt), ct[b][1] =
// pk1 * u + e1, canonical; NTT(e0), NTT(e1) lie in the two halves of ct[b] on entry, NTT(u) and NTT(pt) in rows [batch][L][n] (any
// lazy transform words).  pk [2][L][n] is shared by the whole batch and stays in L2: ordinary loads; everything else streams.
__global__ void __launch_bounds__(ELEM_THREADS) k_enc_pk_fin(const HpLimb *__restrict__ limbs, u32 L, u32 n, u32 chunks, const u64 *__restrict__ pk,
                                                            const u64 *__restrict__ u, const u64 *__restrict__ ptn, u64 *__restrict__ ct) {
    const ElemTile tile(n, chunks);
    const u32 b = tile.row / L, m = tile.row % L;
    const HpLimb lm = limbs[m];
    u64 *c0 = ct + ((size_t)b * 2 * L + m) * n, *c1 = c0 + (size_t)L * n;
    const u64 *k0 = pk + (size_t)m * n, *k1 = k0 + (size_t)L * n, *ur = u + (size_t)tile.row * n;
    const u64 *t = ptn ? ptn + (size_t)tile.row * n : nullptr;
    const auto fin = [&](u64 kw, u64 uw, u64 ew) {
        return hp_add_lazy(hp_mul_hybrid_lazy(kw, uw, lm), hp_lazy_below_2q(ew, lm.two_q), lm.two_q);
    };
    for (const u32 i : tile.pairs()) {   // (n is a multiple of 8: every lane's words are a pair)
        const U2 uv = ld_nt(ur + i), e0 = ld_nt(c0 + i), e1 = ld_nt(c1 + i);
        const U2 p0 = *reinterpret_cast<const U2 *>(k0 + i), p1 = *reinterpret_cast<const U2 *>(k1 + i);
        const u64 ux = hp_lazy_below_2q(uv.x, lm.two_q), uy = hp_lazy_below_2q(uv.y, lm.two_q);
        u64 x0 = fin(p0.x, ux, e0.x), y0 = fin(p0.y, uy, e0.y);
        if (t) {
            const U2 tv = ld_nt(t + i);
            x0 = hp_add_lazy(x0, hp_lazy_below_2q(tv.x, lm.two_q), lm.two_q);
            y0 = hp_add_lazy(y0, hp_lazy_below_2q(tv.y, lm.two_q), lm.two_q);
        }
        st_nt(c0 + i, U2{hp_strict(x0, lm.q), hp_strict(y0, lm.q)});
        st_nt(c1 + i, U2{hp_strict(fin(p1.x, ux, e1.x), lm.q), hp_strict(fin(p1.y, uy, e1.y), lm.q)});
    }
}

// lazy transform words -> canonical residues, in place (hp_dev_sample_small_ntt's last step); row % L = the limb
__global__ void __launch_bounds__(ELEM_THREADS) k_sample_canonical(const HpLimb *__restrict__ limbs, u32 L, u32 n, u32 chunks, u64 *__restrict__ x) {
    const ElemTile tile(n, chunks);
    const u64 q = limbs[tile.row % L].q, two_q = limbs[tile.row % L].two_q;
    u64 *r = x + (size_t)tile.row * n;
    for (const u32 i : tile.pairs()) {
        const U2 v = *reinterpret_cast<const U2 *>(r + i);
        *reinterpret_cast<U2 *>(r + i) = U2{hp_strict(hp_lazy_below_2q(v.x, two_q), q), hp_strict(hp_lazy_below_2q(v.y, two_q), q)};
    }
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
    if (kind == HP_SAMPLE_GAUSS) return sample_launch(k_sample_signed<HP_SAMPLE_GAUSS>, total, stream, seed, logb, total, stream_id, scale, out);
    return hipErrorInvalidValue;
}

hipError_t hp_launch_sample_spread(u32 kind, const HpSampleSeed &seed, const HpSampleRows &rows, u32 L, u32 logn, u64 batch, u64 stream_id,
                                   u64 id_step, long long scale, u64 pstride, u64 *out, hipStream_t stream) {
    if (logn < 3 || L < 1 || L > HP_MAX_LIMBS) return hipErrorInvalidValue;
    const u32 logb = logn - 3;
    const u64 total = batch << logb;
    if (kind == HP_SAMPLE_TERNARY)
        return sample_launch(k_sample_spread<HP_SAMPLE_TERNARY>, total, stream, seed, rows, L, logb, total, stream_id, id_step, scale, pstride, out);
    if (kind == HP_SAMPLE_CBD)
        return sample_launch(k_sample_spread<HP_SAMPLE_CBD>, total, stream, seed, rows, L, logb, total, stream_id, id_step, scale, pstride, out);
    if (kind == HP_SAMPLE_GAUSS)
        return sample_launch(k_gauss_spread, total, stream, seed, rows, L, logb, total, stream_id, id_step, scale, pstride, out);
    return hipErrorInvalidValue;
}

hipError_t hp_launch_enc_seeded(const HpSampleSeed &seed, const HpSampleRows &rows, const HpLimb *limbs, u32 L, u32 logn, u64 batch, u64 stream_id,
                                const u64 *sk, const u64 *ptn, u64 pt_stride, bool with_c1, u64 *ct, hipStream_t stream) {
    if (logn < 3 || L < 1 || L > HP_MAX_LIMBS) return hipErrorInvalidValue;
    const u32 logb = logn - 3;
    const u64 total = (batch * L) << logb;
    const auto go = [&](auto k) { return sample_launch(k, total, stream, seed, rows, limbs, L, logb, total, stream_id, sk, ptn, pt_stride, ct); };
    if (with_c1) return ptn ? go(k_enc_seeded<true, true>) : go(k_enc_seeded<true, false>);
    return ptn ? go(k_enc_seeded<false, true>) : go(k_enc_seeded<false, false>);
}

hipError_t hp_launch_enc_pk_fin(const HpLimb *limbs, u32 L, u32 n, u32 P, const u64 *pk, const u64 *u, const u64 *ptn, u64 *ct,
                                hipStream_t stream) {
    return elem_launch(k_enc_pk_fin, P * L, n, stream, limbs, L, n, ElemChunks{}, pk, u, ptn, ct);
}

hipError_t hp_launch_sample_canonical(const HpLimb *limbs, u32 L, u32 n, u32 rows, u64 *x, hipStream_t stream) {
    return elem_launch(k_sample_canonical, rows, n, stream, limbs, L, n, ElemChunks{}, x);
}
