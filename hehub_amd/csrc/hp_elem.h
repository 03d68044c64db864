// hp_elem.h -- the tile skeleton of the coefficient-wise kernels (hp_elem.hip, hp_ks.hip, hp_edge.hip, hp_hks.hip).
//
// One workgroup of ELEM_THREADS threads streams one chunk (ELEM_CHUNK words unless the kernel says otherwise) of one row of n
// words; blockIdx.x = row * chunks + chunk.  What a row is (a limb of a polynomial, a digit, a whole coefficient column) is the
// kernel's business: it decodes ElemTile::row itself.
#pragma once
#include "hp_kernels.h"
#include <type_traits>

#define ELEM_THREADS 256
#define ELEM_CHUNK 2048u   // words per workgroup = 256 threads x 4 x 16 B

struct alignas(16) U2 {
    u64 x, y;
};

// streaming accesses (read once / written once per launch, far more data than L2 holds): non-temporal
HP_DEV U2 ld_nt(const u64 *p) {
    typedef u64 __attribute__((ext_vector_type(2))) vv;
    const vv v = __builtin_nontemporal_load(reinterpret_cast<const vv *>(p));
    return U2{v.x, v.y};
}
HP_DEV void st_nt(u64 *p, const U2 &v) {
    typedef u64 __attribute__((ext_vector_type(2))) vv;
    __builtin_nontemporal_store(vv{v.x, v.y}, reinterpret_cast<vv *>(p));
}

// ---- device side: which words this workgroup owns ------------------------------------------------------------------------
// the words of a chunk as a range, W adjacent words per lane and round: for (const u32 i : ...) visits the lane's
// i = first + W * threadIdx.x, then every ELEM_THREADS * W further, below last
template <u32 W> struct ElemWords {
    u32 first, last;
    struct It {
        u32 i;
        HP_DEV u32 operator*() const { return i; }
        HP_DEV void operator++() { i += ELEM_THREADS * W; }
        HP_DEV bool operator!=(u32 end) const { return i < end; }
    };
    HP_DEV It begin() const { return It{first + threadIdx.x * W}; }
    HP_DEV u32 end() const { return last; }
};

struct ElemTile {
    u32 row, chunk;   // blockIdx.x = row * chunks + chunk
    u32 n, cw;        // words per row, words per chunk
    HP_DEV ElemTile(u32 n, u32 chunks, u32 cw = ELEM_CHUNK) : row(blockIdx.x / chunks), chunk(blockIdx.x % chunks), n(n), cw(cw) {}
    // a kernel that numbers its workgroups itself (k_hks_inner_hoisted: by XCD) names the tile
    struct At {
        u32 row, chunk;
    };
    HP_DEV ElemTile(At at, u32 n, u32 cw = ELEM_CHUNK) : row(at.row), chunk(at.chunk), n(n), cw(cw) {}
    HP_DEV u32 begin() const { return chunk * cw; }   // the chunk is the words [begin, end) of the row
    HP_DEV u32 end() const { return min(n, (chunk + 1) * cw); }
    HP_DEV bool full() const { return (chunk + 1) * cw <= n; }   // wholly inside the row (every chunk of the tiled ring degrees)
    // the two loop shapes: one word per lane and round; two adjacent words (16-byte accesses), where the last word of an odd
    // row is a lane's single word: for (const u32 i : tile.pairs()) if (tile.pair(i)) { words i, i + 1 } else { word i }
    // (nothing is computed before a kernel asks for it, and the end before the lane's first word: the order the kernels
    // were written and measured in, which the compiler's schedule follows -- tools/isa_diff.py shows when it moves)
    template <u32 W = 1> HP_DEV ElemWords<W> words() const {
        const u32 last = end();
        return ElemWords<W>{begin(), last};
    }
    HP_DEV ElemWords<2> pairs() const { return words<2>(); }
    HP_DEV bool pair(u32 i) const { return i + 1 < end(); }
};

// a full ELEM_CHUNK at two words per lane: round t of a thread is the 16 bytes at elem_full2(tile, row offset) + t * ELEM_STEP2,
// t < ELEM_IT2.
// The kernels issue all loads of a thread first, then the arithmetic and the stores -- the launch shape a plain copy streams
// fastest with (tools/ubench/ubench_copy.hip)
constexpr int ELEM_IT2 = ELEM_CHUNK / (ELEM_THREADS * 2);
constexpr size_t ELEM_STEP2 = ELEM_THREADS * 2;
HP_DEV size_t elem_full2(const ElemTile &t, size_t base) { return base + (size_t)t.chunk * ELEM_CHUNK + threadIdx.x * 2; }

// ---- host side: launches ------------------------------------------------------------------------------------------------
struct ElemChunks {};   // in elem_launch's argument list: the place of the kernel's `chunks` parameter
template <class T> static inline const T &elem_arg(const T &a, u32) { return a; }
static inline u32 elem_arg(ElemChunks, u32 chunks) { return chunks; }

// k<<<rows * chunks of cw words, ELEM_THREADS>>>(args...), rows of n words
template <class... KA, class... A>
static inline hipError_t elem_launch_cw(void (*k)(KA...), u32 cw, u32 rows, u32 n, hipStream_t stream, const A &...args) {
    const u32 chunks = (n + cw - 1) / cw;
    k<<<dim3(chunks * rows, 1, 1), ELEM_THREADS, 0, stream>>>(elem_arg(args, chunks)...);
    return hipGetLastError();
}
template <class... KA, class... A>
static inline hipError_t elem_launch(void (*k)(KA...), u32 rows, u32 n, hipStream_t stream, const A &...args) {
    return elem_launch_cw(k, ELEM_CHUNK, rows, n, stream, args...);
}

// a run-time v in 1..8 as a template integer: f(std::integral_constant<int, v>)
template <int I = 1, class F> static inline hipError_t elem_with_1to8(u32 v, F f) {
    if constexpr (I > 8) return hipErrorInvalidValue;
    else return v == I ? f(std::integral_constant<int, I>{}) : elem_with_1to8<I + 1>(v, f);
}

// ---- device helpers shared by several kernels ---------------------------------------------------------------------------
// Mixed-radix (Garner) digits of the CRT value x = v_0 + v_1 q_0 + v_2 q_0 q_1 + ... (0 <= v_a < q_a) behind strict residues,
// with word arithmetic, for E coefficients at once.  One step: u = the residues modulo q_a on entry, digit v_a on return, given
// the digits v[0..a) and inv[b][a] = q_b^-1 mod q_a (+ Harvey word).  N: the caller's compile-time bound on the number of
// digits, over which the loops are unrolled (1 where the number is known at run time only).
template <int N, int E, int R, int C>
HP_DEV void garner_digit(u64 (&u)[E], const u64 (*v)[E], int a, u64 qa, u64 bc, const u64 (&inv)[R][C], const u64 (&inv_h)[R][C]) {
#pragma unroll N
    for (int b = 0; b < a; b++) {
#pragma unroll
        for (int e = 0; e < E; e++) {
            const u64 vb = hp_strict(hp_barrett_lazy(v[b][e], qa, bc), qa);                    // v_b mod q_a
            u[e] = hp_strict(hp_harvey_lazy(u[e] + qa - vb, inv[b][a], inv_h[b][a], qa), qa);   // (u - v_b) / q_b mod q_a
        }
    }
}
// x < floor(Q/2), half = the digits of floor(Q/2): a lexicographic comparison from the most significant digit down
template <int N, int E> HP_DEV bool garner_below(const u64 (*v)[E], int e, int cnt, const u64 *half) {
    bool below = false, decided = false;
#pragma unroll N
    for (int a = cnt - 1; a >= 0; a--) {
        if (!decided && v[a][e] != half[a]) { below = v[a][e] < half[a]; decided = true; }
    }
    return below;
}

// the addend row of a drop epilogue (k_drop_fin, k_hks_down_fin): polynomial p2 & 1 of ciphertext p2 >> 1, limb k; nullptr where
// the launch has no addend or add_mask leaves this polynomial out
HP_DEV const u64 *drop_addend_row(const u64 *addend, u32 add_poly_stride, u32 add_ct_stride, u32 add_mask, u32 p2, u32 k, u32 n) {
    return (addend && ((add_mask >> (p2 & 1)) & 1u))
               ? addend + ((size_t)(p2 >> 1) * add_ct_stride + (size_t)(p2 & 1) * add_poly_stride + k) * n : nullptr;
}

// ---- the blocks the inner products are made of (hp_ks.hip, hp_hks.hip, hp_lincomb.hip) -------------------------------------------
// A thread owns two adjacent words of a row and one carry-save accumulator (HpAcc, hp_device.h) per word and output.
// every HpAcc of an array of any rank
HP_DEV void acc_zero(HpAcc &a) { hp_acc_zero(a); }
template <class T, int N> HP_DEV void acc_zero(T (&a)[N]) {
#pragma unroll
    for (int i = 0; i < N; i++) acc_zero(a[i]);
}

// one digit of a key-switch inner product: the key's two words of both halves (g0, g1), loaded once, times the digit's two words
// d of a ciphertext into its acc[half][word] -- or of each of PT ciphertexts into acc[ciphertext][half][word]
HP_DEV void key_mac(const U2 &g0, const U2 &g1, const U2 &d, HpAcc (&acc)[2][2]) {
    const u64 kw[2][2] = {{g0.x, g0.y}, {g1.x, g1.y}};
#pragma unroll
    for (int h = 0; h < 2; h++) hp_mac2(acc[h][0], d.x, kw[h][0], acc[h][1], d.y, kw[h][1]);
}
template <int PT> HP_DEV void key_mac(const U2 &g0, const U2 &g1, const U2 (&d)[PT], HpAcc (&acc)[PT][2][2]) {
    const u64 kw[2][2] = {{g0.x, g0.y}, {g1.x, g1.y}};
#pragma unroll
    for (int c = 0; c < PT; c++)
#pragma unroll
        for (int h = 0; h < 2; h++) hp_mac2(acc[c][h][0], d[c].x, kw[h][0], acc[c][h][1], d[c].y, kw[h][1]);
}

// The words (i, i + 1) of a row moved by a rotation: row[map[i]], row[map[i + 1]] -- one 8-byte load of the map's pair, then two
// 8-byte loads -- or, map == NULL, the involution i -> n - 1 - i: the 16 bytes at n - 2 - i, swapped.  The loads are ordinary cached
// ones: a moved row is read scattered, and again by every rotation.  map is wave-uniform (a kernel argument).
struct MovedPair {
    const u32 *map;
    uint2 j;
    HP_DEV MovedPair(const u32 *map, u32 n, u32 i) : map(map), j{n - 2 - i, 0} {
        if (map) j = *reinterpret_cast<const uint2 *>(map + i);
    }
    HP_DEV U2 operator()(const u64 *row) const {
        if (map) return U2{row[j.x], row[j.y]};
        const U2 v = *reinterpret_cast<const U2 *>(row + j.x);
        return U2{v.y, v.x};
    }
};

// tail of the blocked inner products: the accumulators of two adjacent words -> two Montgomery words, for one 16-byte st_nt
// (written once, read by the next kernel from HBM anyway: non-temporal, the key column keeps its place in L2)
HP_DEV U2 acc2_montgomery(const HpAcc &a0, const HpAcc &a1, u64 q, u64 mqinv) {
    u64 l0, h0, l1, h1;
    hp_acc_value(a0, l0, h0);
    hp_acc_value(a1, l1, h1);
    return U2{hp_montgomery128_lazy(l0, h0, q, mqinv), hp_montgomery128_lazy(l1, h1, q, mqinv)};
}
// ... of PT ciphertexts x 2 halves, a key's 2^64 in every product: ciphertext p0 + c (those below P: a ragged last group skips the
// rest) and half h go to the 16 bytes at dst + c * pstride + h * hstride (dst: where the kernel puts ciphertext p0, half 0)
template <int PT>
HP_DEV void acc_store_montgomery(const HpAcc (&acc)[PT][2][2], u32 p0, u32 P, u64 q, u64 mqinv, u64 *dst, size_t pstride, size_t hstride) {
#pragma unroll
    for (int c = 0; c < PT; c++) {
        if (p0 + c < P) {
#pragma unroll
            for (int h = 0; h < 2; h++) {
                const U2 v = acc2_montgomery(acc[c][h][0], acc[c][h][1], q, mqinv);
                st_nt(dst + c * pstride + h * hstride, v);
            }
        }
    }
}

// Tail of a sum of PLAIN products (no operand carries a 2^64: diagonals, tensor products): the one Montgomery reduction of the 128-bit
// sum leaves a factor 2^-64, undone by a Harvey multiplication by 2^64 mod q with the limb's own pair (r64, r64h) -- hp_mul_hybrid_lazy's
// tail: one high and two low products per OUTPUT word, no new constant, and below 2q for ANY 64-bit input, which is what the level-A
// range guard and the drops ask of these rows.  (A Montgomery multiplication by 2^128 mod q costs one more product and a per-limb constant.)
// Range: the Montgomery step returns hi + mulhi(u, q) + 1, so the sum's high half must stay at most 2^64 - 1 - q; how many terms
// that allows is each caller's host formula (hp_drop.h).
HP_DEV U2 acc2_plain(const HpAcc &a0, const HpAcc &a1, u64 q, u64 mqinv, u64 r64, u64 r64h) {
    U2 v = acc2_montgomery(a0, a1, q, mqinv);   // the sum * 2^-64 ...
    v.x = hp_harvey_lazy(v.x, r64, r64h, q);    // ... * 2^64, below 2q
    v.y = hp_harvey_lazy(v.y, r64, r64h, q);
    return v;
}
// ... to the 16 bytes at dst; add_prev: a later launch of a list longer than one table adds its word to the one the earlier launch
// left (the contract is on residues, so the intermediate reductions are free)
HP_DEV void acc_store_plain(const HpAcc &a0, const HpAcc &a1, u64 q, u64 mqinv, u64 two_q, u64 r64, u64 r64h, u32 add_prev, u64 *dst) {
    U2 v = acc2_plain(a0, a1, q, mqinv, r64, r64h);
    if (add_prev) {
        const U2 old = *reinterpret_cast<const U2 *>(dst);
        v.x = hp_add_lazy(v.x, old.x, two_q);
        v.y = hp_add_lazy(v.y, old.y, two_q);
    }
    st_nt(dst, v);
}
