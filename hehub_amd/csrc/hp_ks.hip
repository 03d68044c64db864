// hp_ks.hip -- the two HBM-bound kernels of the headline step: the fused tensor product and the key-switch inner product
// (one ciphertext per thread, and blocked over ciphertexts).  Tile skeleton: hp_elem.h.
#include "hp_elem.h"

// ---- fused tensor product: ckks/arith.cpp:55-62 / bgv/arith.cpp:59-69 -------------------
// d0 = a0*b0, d1 = (a0*b1) + (a1*b0), d2 = a1*b1.  Reads 4 limbs, writes 3: 56n bytes per limb index.
// ROWS: the four operand polynomials of ciphertext pair p by address (an application's ciphertexts are separate objects: the
// fused pipelines read them where they lie, hp_dev_*_mult_*_rows); the addresses travel as kernel arguments
// the three output words of one coefficient: d0 = tensor_sq(x0, y0), d1 = tensor_cross(x0, x1, y0, y1), d2 = tensor_sq(x1, y1)
HP_DEV u64 tensor_sq(u64 x, u64 y, const HpLimb &m) { return hp_mul_hybrid_lazy(x, y, m); }
HP_DEV u64 tensor_cross(u64 x0, u64 x1, u64 y0, u64 y1, const HpLimb &m) {
    return hp_add_lazy(hp_mul_hybrid_lazy(x0, y1, m), hp_mul_hybrid_lazy(x1, y0, m), m.two_q);
}

template <bool ROWS>
__global__ void __launch_bounds__(ELEM_THREADS) k_tensor(const HpLimb *__restrict__ limbs, u32 L, u32 k_first, u32 kc,
                                                        u32 n, u32 chunks, u32 cw, const u64 *__restrict__ ct1,
                                                        const u64 *__restrict__ ct2, HpTensorRows rows, u64 *__restrict__ quad) {
    const ElemTile tile(n, chunks, cw);   // row = p*kc + (k - k_first); cw = words per workgroup
    const u32 p = tile.row / kc, k = k_first + tile.row % kc;
    const HpLimb m = limbs[k];
    const size_t poly = (size_t)L * n;
    const u64 *a0 = ROWS ? rows.p[p][0] + (size_t)k * n : ct1 + (size_t)p * 2 * poly + (size_t)k * n;
    const u64 *a1 = ROWS ? rows.p[p][1] + (size_t)k * n : a0 + poly;
    const u64 *b0 = ROWS ? rows.p[p][2] + (size_t)k * n : ct2 + (size_t)p * 2 * poly + (size_t)k * n;
    const u64 *b1 = ROWS ? rows.p[p][3] + (size_t)k * n : b0 + poly;
    u64 *d0 = quad + (size_t)p * 3 * poly + (size_t)k * n, *d1 = d0 + poly, *d2 = d1 + poly;
    // (issuing the loads of several steps together, which gains 5-9 % in k_poly_binary, measured +-0 here: 0.830 vs 0.827 ms)
    for (const u32 i : tile.pairs()) {
        if (tile.pair(i)) {
            const U2 va0 = ld_nt(a0 + i), va1 = ld_nt(a1 + i);
            const U2 vb0 = ld_nt(b0 + i), vb1 = ld_nt(b1 + i);
            const U2 r0{tensor_sq(va0.x, vb0.x, m), tensor_sq(va0.y, vb0.y, m)};
            const U2 r1{tensor_cross(va0.x, va1.x, vb0.x, vb1.x, m), tensor_cross(va0.y, va1.y, vb0.y, vb1.y, m)};
            const U2 r2{tensor_sq(va1.x, vb1.x, m), tensor_sq(va1.y, vb1.y, m)};
            st_nt(d0 + i, r0);
            st_nt(d1 + i, r1);
            st_nt(d2 + i, r2);
        } else {
            const u64 x0 = a0[i], x1 = a1[i], y0 = b0[i], y1 = b1[i];
            d0[i] = tensor_sq(x0, y0, m);
            d1[i] = tensor_cross(x0, x1, y0, y1, m);
            d2[i] = tensor_sq(x1, y1, m);
        }
    }
}

// a workgroup covers 2048 words of a limb in four dependent load -> multiply -> store steps per thread; a launch of a few limbs
// (one ciphertext through hehub's one-call-per-ciphertext interface: 160 workgroups at C3) is then four memory latencies long
// with a third of the CUs idle -- such a launch gets 512 words per workgroup (one step per thread)
static inline u32 tensor_chunk(u32 n, u32 rows) {
    return ((size_t)rows * ((n + ELEM_CHUNK - 1) / ELEM_CHUNK) < 1024 && n >= ELEM_THREADS * 2) ? ELEM_THREADS * 2 : ELEM_CHUNK;
}

hipError_t hp_launch_tensor(const HpLimb *limbs, u32 L, u32 k_first, u32 kc, u32 n, u32 P, const u64 *ct1,
                            const u64 *ct2, u64 *quad, hipStream_t stream) {
    if (kc == 0) return hipSuccess;
    const u32 cw = tensor_chunk(n, P * kc);
    return elem_launch_cw(k_tensor<false>, cw, P * kc, n, stream, limbs, L, k_first, kc, n, ElemChunks{}, cw, ct1, ct2,
                          HpTensorRows{}, quad);
}

hipError_t hp_launch_tensor_rows(const HpLimb *limbs, u32 L, u32 k_first, u32 kc, u32 n, u32 P, const HpTensorRows &rows, u64 *quad,
                                 hipStream_t stream) {
    if (kc == 0 || P == 0) return hipSuccess;
    if (P > HP_TENSOR_ROWS_MAX) return hipErrorInvalidValue;
    const u32 cw = tensor_chunk(n, P * kc);
    return elem_launch_cw(k_tensor<true>, cw, P * kc, n, stream, limbs, L, k_first, kc, n, ElemChunks{}, cw, nullptr, nullptr,
                          rows, quad);
}

// ---- sum of tensor products (hp_dev_ckks_tensor_sum) ------------------------------------------
// quad = (sum_t a0 b0, sum_t (a0 b1 + a1 b0), sum_t a1 b1) over the terms of the table, for lazy relinearisation: everything after the
// tensor product is linear in the quadratic ciphertext, so T products pay ONE key switch.  A thread owns one pair of words of a row
// (p, limb), as in k_tensor, and keeps them for every term: six carry-save accumulators (three outputs x two words), per term four
// 16-byte non-temporal loads (every operand word is read once per call) and four hp_mac2, and after the last term the tail of a sum
// of plain products (acc_store_plain, hp_elem.h): ONE Montgomery reduction per output word.  HBM traffic per output word: 32 T + 24
// bytes, against (56 + 24 + 24) T for T launches of k_tensor and a fold of their rows.
// Range: operand words below 2q, the d1 column with two products per term: a launch of T terms sums at most 2 T (2q - 1)^2, which the
// host keeps within the tail's limit (hpi::tensor_sum_max_terms, hp_drop.h: the whole table for every modulus the transforms accept).
// A larger operand word can wrap the sums unnoticed.  A longer list takes one launch per table, the later ones with add_prev.
// TWO: the lane's words i, i + 1 (16-byte accesses); else the single last word of an odd row
template <bool TWO>
HP_DEV void tensor_sum_words(const HpLimb &m, const HpTensorSumTable &tab, size_t at, size_t poly, u32 add_prev, u64 *d0) {
    HpAcc s[3][2];   // [output][word]
    acc_zero(s);
    for (u32 t = 0; t < tab.terms; t++) {
        const u64 *a0 = tab.a[t] + at, *b0 = tab.b[t] + at;
        U2 va0, va1, vb0, vb1;
        if (TWO) {
            va0 = ld_nt(a0); va1 = ld_nt(a0 + poly);
            vb0 = ld_nt(b0); vb1 = ld_nt(b0 + poly);
        } else {
            va0 = U2{a0[0], 0}; va1 = U2{a0[poly], 0};
            vb0 = U2{b0[0], 0}; vb1 = U2{b0[poly], 0};
        }
        hp_mac2(s[0][0], va0.x, vb0.x, s[0][1], va0.y, vb0.y);
        hp_mac2(s[1][0], va0.x, vb1.x, s[1][1], va0.y, vb1.y);
        hp_mac2(s[1][0], va1.x, vb0.x, s[1][1], va1.y, vb0.y);
        hp_mac2(s[2][0], va1.x, vb1.x, s[2][1], va1.y, vb1.y);
    }
#pragma unroll
    for (int c = 0; c < 3; c++) {
        u64 *dst = d0 + (size_t)c * poly;
        if (TWO) {
            acc_store_plain(s[c][0], s[c][1], m.q, m.mqinv, m.two_q, m.r64, m.r64h, add_prev, dst);
        } else {
            const u64 v = acc2_plain(s[c][0], s[c][1], m.q, m.mqinv, m.r64, m.r64h).x;
            dst[0] = add_prev ? hp_add_lazy(v, dst[0], m.two_q) : v;
        }
    }
}

__global__ void __launch_bounds__(ELEM_THREADS) k_tensor_sum(const HpLimb *__restrict__ limbs, u32 L, u32 n, u32 chunks, u32 cw,
                                                            HpTensorSumTable tab, u32 add_prev, u64 *__restrict__ quad) {
    const ElemTile tile(n, chunks, cw);   // row = p*L + k; cw = words per workgroup
    const u32 p = tile.row / L, k = tile.row % L;
    const HpLimb m = limbs[k];
    const size_t poly = (size_t)L * n;
    const size_t in = (size_t)p * 2 * poly + (size_t)k * n;   // row (p, polynomial 0, k) of every operand
    u64 *d0 = quad + (size_t)p * 3 * poly + (size_t)k * n;
    for (const u32 i : tile.pairs()) {
        if (tile.pair(i)) tensor_sum_words<true>(m, tab, in + i, poly, add_prev, d0 + i);
        else tensor_sum_words<false>(m, tab, in + i, poly, add_prev, d0 + i);
    }
}

hipError_t hp_launch_tensor_sum(const HpLimb *limbs, u32 L, u32 n, u32 P, const HpTensorSumTable &tab, bool add_prev, u64 *quad,
                                hipStream_t stream) {
    if (P == 0 || L == 0 || tab.terms == 0) return hipSuccess;
    if (tab.terms > HP_TENSOR_SUM_MAX) return hipErrorInvalidValue;
    const u32 cw = tensor_chunk(n, P * L);
    if ((u64)P * L * ((n + cw - 1) / cw) >= (1ull << 31)) return hipErrorInvalidValue;   // (workgroups of one launch)
    return elem_launch_cw(k_tensor_sum, cw, P * L, n, stream, limbs, L, n, ElemChunks{}, cw, tab, add_prev ? 1u : 0u, quad);
}

// ---- key-switch inner product: rgsw.cpp:121-153 --------------------------------------------
// out[p][half][k][i] = montgomery_128( sum_j D[p][j][k][i] * key[j][half][k][i] ), 128-bit accumulators
// in registers, both halves from one pass over the digits.  Per (p, k, i): reads L digit words and 2L key
// words (the key is shared by the whole batch and stays in L2 / Infinity Cache), writes 2 words.
// One ciphertext (or an odd one out) per call: a LATENCY kernel -- hehub's one-call-per-ciphertext interface (ckks.h:270-313)
// puts a single key switch on the critical path of every call.  A workgroup covers 512 coefficients (two per lane, one pass),
// and the three 16-byte loads of FOUR digits are issued before their multiplications: the dependent rounds to memory drop from
// 4 x L to L / 4.
// MANY: every ciphertext of the launch has its OWN key (hp_dev_ckks_rotate_many: the rotations of one vector by different steps
// in the diagonal loop of src/circuits/linear_algebra.h:123-130); the key addresses travel as kernel arguments.  Nothing is
// shared between ciphertexts then, so this one-ciphertext-per-thread kernel is also the right one for a batch: 3L rows per
// (p, k).
#define KS1_CHUNK 512u
template <bool MANY>
__global__ void __launch_bounds__(ELEM_THREADS) k_ks_inner(const HpLimb *__restrict__ limbs, u32 L, u32 k_first, u32 P,
                                                          u32 key_Le, u32 n, u32 chunks, const u64 *__restrict__ digits,
                                                          const u64 *__restrict__ pt,
                                                          u32 pt_pstride, const u64 *__restrict__ key_one, HpKeyTable keys,
                                                          u64 *__restrict__ out) {
    const u32 Le = L + 1;
    const ElemTile tile(n, chunks, KS1_CHUNK);   // row = k*P' ... decoded below
    // modulus-major numbering keeps one key column (2L limbs) hot per XCD slice
    const u32 k = k_first + tile.row / P, p = tile.row % P;
    const u64 *__restrict__ key = MANY ? keys.p[p] : key_one;
    const u64 q = limbs[k].q, mqinv = limbs[k].mqinv;
    const u32 i = tile.begin() + threadIdx.x * 2;
    if (i >= n) return;
    const bool two = (i + 1 < n);
    // a key made for more moduli than the ciphertext has (extension): its special-prime column is the last one
    const u32 kcol = (k == L) ? key_Le - 1 : k;
    u64 a0l[2] = {0, 0}, a0h[2] = {0, 0}, a1l[2] = {0, 0}, a1h[2] = {0, 0};
    constexpr u32 G = 4;
    for (u32 j0 = 0; j0 < L; j0 += G) {
        u64 dv[G][2], k0[G][2], k1[G][2];
#pragma unroll
        for (u32 t = 0; t < G; t++) {
            const u32 j = j0 + t < L ? j0 + t : L - 1;   // (a slot past the last digit reloads it and is skipped below)
            const u64 *d = (j == k) ? pt + ((size_t)p * pt_pstride + j) * n : digits + (((size_t)p * L + j) * Le + k) * n;
            const u64 *g0 = key + (((size_t)j * 2 + 0) * key_Le + kcol) * n;
            const u64 *g1 = key + (((size_t)j * 2 + 1) * key_Le + kcol) * n;
            if (two) {
                // digits are read exactly once: non-temporal, so they do not evict the key column from L2
                const U2 dvv = ld_nt(d + i);
                dv[t][0] = dvv.x; dv[t][1] = dvv.y;
                U2 w;
                w = *reinterpret_cast<const U2 *>(g0 + i); k0[t][0] = w.x; k0[t][1] = w.y;
                w = *reinterpret_cast<const U2 *>(g1 + i); k1[t][0] = w.x; k1[t][1] = w.y;
            } else {
                dv[t][0] = d[i]; k0[t][0] = g0[i]; k1[t][0] = g1[i]; dv[t][1] = k0[t][1] = k1[t][1] = 0;
            }
        }
#pragma unroll
        for (u32 t = 0; t < G; t++) {
            if (j0 + t >= L) break;
#pragma unroll
            for (int e = 0; e < 2; e++) {   // the sums in the reference's order j = 0 .. L-1 (rgsw.cpp:126-149)
                u64 lo, hi;
                hp_mul128(dv[t][e], k0[t][e], lo, hi);
                a0l[e] += lo; a0h[e] += hi + (a0l[e] < lo ? 1ull : 0ull);
                hp_mul128(dv[t][e], k1[t][e], lo, hi);
                a1l[e] += lo; a1h[e] += hi + (a1l[e] < lo ? 1ull : 0ull);
            }
        }
    }
    u64 *o0 = out + (((size_t)p * 2 + 0) * Le + k) * n;
    u64 *o1 = out + (((size_t)p * 2 + 1) * Le + k) * n;
    u64 r00 = hp_montgomery128_lazy(a0l[0], a0h[0], q, mqinv), r10 = hp_montgomery128_lazy(a1l[0], a1h[0], q, mqinv);
    if (two) {
        U2 v0{r00, hp_montgomery128_lazy(a0l[1], a0h[1], q, mqinv)};
        U2 v1{r10, hp_montgomery128_lazy(a1l[1], a1h[1], q, mqinv)};
        *reinterpret_cast<U2 *>(o0 + i) = v0;
        *reinterpret_cast<U2 *>(o1 + i) = v1;
    } else {
        o0[i] = r00; o1[i] = r10;
    }
}

// Same sums, PT ciphertexts per thread: the 2L key words of a (k, i) pair are loaded once and multiplied into PT
// ciphertexts' accumulators, so the key traffic through L2 / Infinity Cache (2L of the 3L+2 words per (p,k,i) above)
// drops by PT.  n is even for every supported ring (N >= 2) and chunks are even-sized: always two words per lane.
//
// Addressing is what bounded the first version of this kernel: a wave issued 218 SCALAR instructions per digit (64-bit row
// addresses for PT + 2 loads, each a multiply chain) next to 130 vector ones, and a SIMD issues at most one scalar instruction
// per turn -- VALUBusy 63 % with HBM at 57 %.  Now every stream is a buffer descriptor set up once per workgroup (PT digit
// rows, PT caller limbs for the diagonal, the key column), the lane offset is computed once per sweep, and the digit index
// moves ONE scalar offset per stream: ~10 scalar instructions per digit.
// The diagonal j == k (the caller's NTT-form limb, rgsw.cpp:99-101) comes first, then the L-1 (special prime: L) digit rows
// in a branch-free, hand double-buffered loop; u128 sums wrap, so the order of the terms does not matter.
typedef u32 __attribute__((ext_vector_type(4))) v4u;
typedef u32 __attribute__((ext_vector_type(2))) v2u;
constexpr int KS_NT = 2;   // buffer-load cache policy bit "nt": digits are read exactly once, keep them from evicting the key column

template <int PT> struct KsRow {
    U2 g0, g1;
    U2 d[PT];
};

HP_DEV __amdgpu_buffer_rsrc_t ks_rsrc(const void *base) {
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<void *>(base), 0, 0x7fffffff, 0x00020000);
}
HP_DEV U2 ks_u2(const v4u &v) { return U2{((u64)v.y << 32) | v.x, ((u64)v.w << 32) | v.z}; }

// PACK: 48 / 40 = the digit rows of this output modulus are in the HP_PACK48 / HP_PACK40 format (hp_device.h); 0 = plain words
template <int PT, int PACK>
HP_DEV void ks_sweep(const __amdgpu_buffer_rsrc_t (&rd)[PT], const __amdgpu_buffer_rsrc_t (&rp)[PT], __amdgpu_buffer_rsrc_t rk,
                     u32 i, u32 n, u32 L, u32 k, u32 d_stride, u32 k_stride, u32 k_half, u64 q, HpAcc (&acc)[PT][2][2]) {
    const u32 v16 = i << 3, v8 = i << 2, v4 = i << 1;   // lane byte offsets: plain words / low planes / high planes (48-bit rows)
    u64 ksum[2][2] = {{0, 0}, {0, 0}};                   // HP_PACK40: sum of the key words the offset rows were multiplied by
    const bool diag = k < L;
    const u32 T = diag ? L - 1 : L;                     // digit rows besides the diagonal
    auto load_key = [&](KsRow<PT> &r, u32 j) {
        const u32 so = __builtin_amdgcn_readfirstlane(j * k_stride);   // (wave-uniform: keeps the row offsets in SGPRs)
        r.g0 = ks_u2(__builtin_amdgcn_raw_buffer_load_b128(rk, v16, so, 0));
        r.g1 = ks_u2(__builtin_amdgcn_raw_buffer_load_b128(rk, v16, so + k_half, 0));
    };
    auto load_digit = [&](KsRow<PT> &r, u32 t) {
        const u32 j = t + ((diag && t >= k) ? 1u : 0u);
        load_key(r, j);
        const u32 so = __builtin_amdgcn_readfirstlane(j * d_stride);
#pragma unroll
        for (int c = 0; c < PT; c++) {
            if (PACK == 48) {
                const v2u lo = __builtin_amdgcn_raw_buffer_load_b64(rd[c], v8, so, KS_NT);
                const u32 hi = __builtin_amdgcn_raw_buffer_load_b32(rd[c], v4, so + (n << 2), KS_NT);
                r.d[c].x = lo.x | ((u64)(hi & 0xffffu) << 32);
                r.d[c].y = lo.y | ((u64)(hi >> 16) << 32);
            } else if (PACK == 40) {
                const v2u lo = __builtin_amdgcn_raw_buffer_load_b64(rd[c], v8, so, KS_NT);
                const u32 hi = (u32)(unsigned short)__builtin_amdgcn_raw_buffer_load_b16(rd[c], i, so + (n << 2), KS_NT);
                r.d[c].x = lo.x | ((u64)(hi & 0xffu) << 32);
                r.d[c].y = lo.y | ((u64)(hi >> 8) << 32);
            } else {
                r.d[c] = ks_u2(__builtin_amdgcn_raw_buffer_load_b128(rd[c], v16, so, KS_NT));
            }
        }
    };
    KsRow<PT> ra, rb;
    if (diag) {
        load_key(rb, k);
#pragma unroll
        for (int c = 0; c < PT; c++) rb.d[c] = ks_u2(__builtin_amdgcn_raw_buffer_load_b128(rp[c], v16, 0, KS_NT));
    }
    auto mac_digit = [&](const KsRow<PT> &r) {
        key_mac(r.g0, r.g1, r.d, acc);
        if (PACK == 40) { ksum[0][0] += r.g0.x; ksum[0][1] += r.g0.y; ksum[1][0] += r.g1.x; ksum[1][1] += r.g1.y; }
    };
    if (T) load_digit(ra, 0);
    if (diag) key_mac(rb.g0, rb.g1, rb.d, acc);
    if (!T) return;
    u32 t = 0;
    for (; t + 2 <= T; t += 2) {
        load_digit(rb, t + 1);
        mac_digit(ra);
        load_digit(ra, min(t + 2, T - 1));   // last: harmless re-read
        mac_digit(rb);
    }
    if (t < T) mac_digit(ra);
    if (PACK == 40) {
        const u64 qc = (q - 1) >> 1;
#pragma unroll
        for (int c = 0; c < PT; c++)
#pragma unroll
            for (int h = 0; h < 2; h++) hp_mac2(acc[c][h][0], qc, ksum[h][0], acc[c][h][1], qc, ksum[h][1]);
    }
}

template <int PT, bool P40 = false>
__global__ void __launch_bounds__(ELEM_THREADS) k_ks_inner_blk(const HpLimb *__restrict__ limbs, u32 L, u32 k_first, u32 P,
                                                              u32 key_Le, u32 n, u32 chunks, const u64 *__restrict__ digits,
                                                              const u64 *__restrict__ pt, u32 pt_pstride,
                                                              const u64 *__restrict__ key, u64 *__restrict__ out, u32 pack_mask,
                                                              u32 pack40_mask) {
    const u32 Le = L + 1;
    const u32 PG = (P + PT - 1) / PT;
    const ElemTile tile(n, chunks);
    const u32 k = k_first + tile.row / PG, p0 = (tile.row % PG) * PT;
    const u64 q = limbs[k].q, mqinv = limbs[k].mqinv;
    const u32 kcol = (k == L) ? key_Le - 1 : k;   // key made for more moduli (extension): special prime = its last column
    // (P40: its own kernel, so that the level-B one keeps its registers)
    const bool packed = ((pack_mask >> k) & 1u) != 0, packed40 = P40 && ((pack40_mask >> k) & 1u) != 0;
    // descriptors: digit row (p, j = 0, k) -- the digit index adds j * Le * 8n bytes; the caller's limb (p, k); the key column
    // (j = 0, half 0, kcol) -- j adds 2 * key_Le * 8n bytes, the second half key_Le * 8n.  (32-bit offsets: L (L + 1) * 8n and
    // 2 L key_Le * 8n stay below 2^30 bytes at N = 32768 with the 32 limbs the engine allows.)
    __amdgpu_buffer_rsrc_t rd[PT], rp[PT];
#pragma unroll
    for (int c = 0; c < PT; c++) {
        const u32 p = min(p0 + c, P - 1);   // a ragged last group re-reads its last ciphertext and skips the store
        rd[c] = ks_rsrc(digits + ((size_t)p * L * Le + k) * n);
        rp[c] = ks_rsrc(pt + ((size_t)p * pt_pstride + min(k, L - 1)) * n);
    }
    const __amdgpu_buffer_rsrc_t rk = ks_rsrc(key + (size_t)kcol * n);
    const u32 d_stride = (Le * n) << 3, k_half = (key_Le * n) << 3, k_stride = k_half << 1;
    for (const u32 i : tile.pairs()) {
        HpAcc acc[PT][2][2];   // [ciphertext][half][word]
        acc_zero(acc);
        if (P40 && packed40) ks_sweep<PT, 40>(rd, rp, rk, i, n, L, k, d_stride, k_stride, k_half, q, acc);
        else if (packed) ks_sweep<PT, 48>(rd, rp, rk, i, n, L, k, d_stride, k_stride, k_half, q, acc);
        else ks_sweep<PT, 0>(rd, rp, rk, i, n, L, k, d_stride, k_stride, k_half, q, acc);
        acc_store_montgomery(acc, p0, P, q, mqinv, out + ((size_t)p0 * 2 * Le + k) * n + i, (size_t)2 * Le * n, (size_t)Le * n);
    }
}

hipError_t hp_launch_ks_inner(const HpLimb *limbs, u32 L, u32 k_first, u32 kc, u32 key_Le, u32 n, u32 P, const u64 *digits,
                              const u64 *pt, u32 pt_pstride, const u64 *key, u64 *out, u32 pack_mask, u32 pack40_mask,
                              hipStream_t stream) {
    if (kc == 0) return hipSuccess;
    // the one-ciphertext kernel reads plain rows only
    if ((pack_mask | pack40_mask) && !(n >= 2 && P >= 2)) return hipErrorInvalidValue;
    // the blocked kernels address digit rows and key columns through buffer descriptors with 32-bit byte offsets
    // (j * (L+1) * 8n and j * 2 key_Le * 8n + key_Le * 8n, j < L): an offset past 2^31 would read zeros, not fault
    if ((u64)L * (L + 1) * 8u * n >= (1ull << 31) || 2ull * L * key_Le * 8u * n >= (1ull << 31)) return hipErrorInvalidValue;
    // ciphertexts per thread: four share every key word in registers (1 or 2 measured 1.5 % slower at the C3 shape)
    const u32 PT = (n >= 2 && P >= 4) ? 4 : (n >= 2 && P >= 2) ? 2 : 1;
    if (PT == 1)
        return elem_launch_cw(k_ks_inner<false>, KS1_CHUNK, P * kc, n, stream, limbs, L, k_first, P, key_Le, n, ElemChunks{}, digits,
                              pt, pt_pstride, key, HpKeyTable{}, out);
    const auto k = PT == 4 ? (pack40_mask ? k_ks_inner_blk<4, true> : k_ks_inner_blk<4>)
                           : (pack40_mask ? k_ks_inner_blk<2, true> : k_ks_inner_blk<2>);
    return elem_launch(k, ((P + PT - 1) / PT) * kc, n, stream, limbs, L, k_first, P, key_Le, n, ElemChunks{}, digits, pt, pt_pstride,
                       key, out, pack_mask, pack40_mask);
}

// every ciphertext with its own key: plain digit rows, P <= HP_KEY_TABLE_MAX per launch
hipError_t hp_launch_ks_inner_many(const HpLimb *limbs, u32 L, u32 k_first, u32 kc, u32 key_Le, u32 n, u32 P, const u64 *digits,
                                   const u64 *pt, u32 pt_pstride, const HpKeyTable &keys, u64 *out, hipStream_t stream) {
    if (kc == 0 || P == 0) return hipSuccess;
    if (P > HP_KEY_TABLE_MAX) return hipErrorInvalidValue;
    return elem_launch_cw(k_ks_inner<true>, KS1_CHUNK, P * kc, n, stream, limbs, L, k_first, P, key_Le, n, ElemChunks{}, digits, pt,
                          pt_pstride, nullptr, keys, out);
}
