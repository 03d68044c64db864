// hp_elem.hip -- coefficient-wise CDNA4 kernels (HBM-streaming, 16-byte accesses): polynomial arithmetic, copies, gathers and
// the single-vector entry points.  (The tensor product and the key-switch inner product: hp_ks.hip; drop helpers, encrypt /
// decrypt cores and base transforms: hp_edge.hip.)
//
// Bound: HBM.  Algorithmic bytes per limb of n words: binary op 24n, unary 16n
// (SURVEY.md section 8d).  One workgroup streams one 2048-word chunk of one
// limb with 16-byte loads/stores (hp_elem.h); the limb's constants are wave-uniform and
// come from scalar loads of the plan entry.
#include "hp_elem.h"
#include <cstdlib>

// ---- binary: rns.cpp:58-87 (add), :89-118 (sub), :120-140 (mul) ----------------
template <int OP> HP_DEV u64 poly_binary_op(u64 x, u64 y, const HpLimb &m) {
    if constexpr (OP == HP_ADD) return hp_add_lazy(x, y, m.two_q);
    else if constexpr (OP == HP_SUB) return hp_sub_lazy(x, y, m.two_q);
    else return hp_mul_hybrid_lazy(x, y, m);
}
template <int OP> HP_DEV U2 poly_binary_op(const U2 &x, const U2 &y, const HpLimb &m) {
    return U2{poly_binary_op<OP>(x.x, y.x, m), poly_binary_op<OP>(x.y, y.y, m)};
}

template <int OP>
__global__ void __launch_bounds__(ELEM_THREADS) k_poly_binary(const HpLimb *__restrict__ limbs, u32 L, u32 n,
                                                             u32 chunks, const u64 *a,
                                                             const u64 *b, u64 *out) {   // out may be a (operator+=)
    const ElemTile tile(n, chunks);
    const HpLimb m = limbs[tile.row % L];
    const size_t base = (size_t)tile.row * n;
    const auto pairs = tile.pairs();
    if (tile.full()) {
        // the eight 16-byte loads of a thread are issued together, then the arithmetic and the four stores (hp_elem.h)
        const size_t o = elem_full2(tile, base);
        U2 va[ELEM_IT2], vb[ELEM_IT2];
#pragma unroll
        for (int t = 0; t < ELEM_IT2; ++t) {
            va[t] = ld_nt(a + o + t * ELEM_STEP2);
            vb[t] = ld_nt(b + o + t * ELEM_STEP2);
        }
#pragma unroll
        for (int t = 0; t < ELEM_IT2; ++t) {
            const U2 r = poly_binary_op<OP>(va[t], vb[t], m);
            st_nt(out + o + t * ELEM_STEP2, r);
        }
        return;
    }
    for (const u32 i : pairs) {
        if (tile.pair(i)) {
            const U2 r = poly_binary_op<OP>(ld_nt(a + base + i), ld_nt(b + base + i), m);
            st_nt(out + base + i, r);
        } else {
            const u64 r = poly_binary_op<OP>(a[base + i], b[base + i], m);
            out[base + i] = r;
        }
    }
}

hipError_t hp_launch_poly_binary(int op, const HpLimb *limbs, u32 L, u32 n, u32 rows, const u64 *a,
                                 const u64 *b, u64 *out, hipStream_t stream) {
    static constexpr decltype(&k_poly_binary<HP_ADD>) kernels[] = {k_poly_binary<HP_ADD>, k_poly_binary<HP_SUB>, k_poly_binary<HP_MUL>};
    return elem_launch(kernels[op == HP_ADD || op == HP_SUB ? op : HP_MUL], rows, n, stream, limbs, L, n, ElemChunks{}, a, b, out);
}

// ---- a chain of += / -= in one pass: rns.cpp:58-118 term after term ----------------------------------------------------
// out[p] = ((x_0 op_1 x_1) op_2 x_2) ... of polynomial p's `terms` operand rows (anywhere; addresses as kernel arguments),
// op_j = -= where bit j of neg is set: the words of the single calls in their order (each step is the lazy add / sub of
// rns.cpp), the intermediate sums never cross HBM.  The accumulate of a diagonal loop (src/circuits/linear_algebra.h:117-121)
// is such a chain.
__global__ void __launch_bounds__(ELEM_THREADS) k_poly_fold(const HpLimb *__restrict__ limbs, u32 L, u32 n, u32 chunks, u32 terms,
                                                           HpFoldRows rows, u64 *__restrict__ out) {
    const ElemTile tile(n, chunks);   // row = p * L + k
    const u32 p = tile.row / L, k = tile.row % L;
    const u64 two_q = limbs[k].two_q;
    const size_t off = (size_t)k * n;
    const u64 *const *src = rows.p + (size_t)p * terms;
    u64 *dst = out + (size_t)tile.row * n;
    const auto words = tile.words();
    if (tile.full()) {   // four 16-byte loads of a term in flight per thread
        const size_t o = elem_full2(tile, off);
        U2 acc[ELEM_IT2];
#pragma unroll
        for (int t = 0; t < ELEM_IT2; ++t) acc[t] = ld_nt(src[0] + o + t * ELEM_STEP2);
        for (u32 j = 1; j < terms; ++j) {
            const u64 *x = src[j] + o;
            U2 v[ELEM_IT2];
#pragma unroll
            for (int t = 0; t < ELEM_IT2; ++t) v[t] = ld_nt(x + t * ELEM_STEP2);
            if ((rows.neg >> j) & 1u) {
#pragma unroll
                for (int t = 0; t < ELEM_IT2; ++t) {
                    acc[t].x = hp_sub_lazy(acc[t].x, v[t].x, two_q);
                    acc[t].y = hp_sub_lazy(acc[t].y, v[t].y, two_q);
                }
            } else {
#pragma unroll
                for (int t = 0; t < ELEM_IT2; ++t) {
                    acc[t].x = hp_add_lazy(acc[t].x, v[t].x, two_q);
                    acc[t].y = hp_add_lazy(acc[t].y, v[t].y, two_q);
                }
            }
        }
#pragma unroll
        for (int t = 0; t < ELEM_IT2; ++t) st_nt(dst + (o - off) + t * ELEM_STEP2, acc[t]);
        return;
    }
    for (const u32 i : words) {
        u64 acc = src[0][off + i];
        for (u32 j = 1; j < terms; ++j) {
            const u64 v = src[j][off + i];
            acc = ((rows.neg >> j) & 1u) ? hp_sub_lazy(acc, v, two_q) : hp_add_lazy(acc, v, two_q);
        }
        dst[i] = acc;
    }
}

hipError_t hp_launch_poly_fold(const HpLimb *limbs, u32 L, u32 n, u32 polys, u32 terms, const HpFoldRows &rows, u64 *out,
                               hipStream_t stream) {
    return elem_launch(k_poly_fold, polys * L, n, stream, limbs, L, n, ElemChunks{}, terms, rows, out);
}

// ---- unary: rns.cpp:142-171 (scalar multiply), mod_arith.h:65-72 (strict) --------
template <int STRICT> HP_DEV u64 poly_unary_op(u64 x, u64 s, u64 sh, u64 q) {
    return STRICT ? hp_strict(x, q) : hp_harvey_lazy(x, s, sh, q);
}
template <int STRICT> HP_DEV U2 poly_unary_op(const U2 &x, u64 s, u64 sh, u64 q) {
    return U2{poly_unary_op<STRICT>(x.x, s, sh, q), poly_unary_op<STRICT>(x.y, s, sh, q)};
}

template <int STRICT>
__global__ void __launch_bounds__(ELEM_THREADS) k_poly_unary(const HpLimb *__restrict__ limbs, HpScalars sc, u32 L,
                                                            u32 n, u32 chunks, const u64 *a,
                                                            u64 *out) {   // in-place use: out == a
    const ElemTile tile(n, chunks);
    const u32 k = tile.row % L;
    const u64 q = limbs[k].q;
    const u64 s = sc.s[k], sh = sc.sh[k];
    const size_t base = (size_t)tile.row * n;
    const auto pairs = tile.pairs();
    if (tile.full()) {   // all loads of the thread first (see k_poly_binary)
        const size_t o = elem_full2(tile, base);
        U2 v[ELEM_IT2];
#pragma unroll
        for (int t = 0; t < ELEM_IT2; ++t) v[t] = ld_nt(a + o + t * ELEM_STEP2);
#pragma unroll
        for (int t = 0; t < ELEM_IT2; ++t) {
            const U2 r = poly_unary_op<STRICT>(v[t], s, sh, q);
            st_nt(out + o + t * ELEM_STEP2, r);
        }
        return;
    }
    for (const u32 i : pairs) {
        if (tile.pair(i)) {
            const U2 r = poly_unary_op<STRICT>(ld_nt(a + base + i), s, sh, q);
            st_nt(out + base + i, r);
        } else {
            const u64 r = poly_unary_op<STRICT>(a[base + i], s, sh, q);
            out[base + i] = r;
        }
    }
}

hipError_t hp_launch_poly_scalar_mul(const HpLimb *limbs, const HpScalars &sc, u32 L, u32 n, u32 rows,
                                     const u64 *a, u64 *out, hipStream_t stream) {
    return elem_launch(k_poly_unary<0>, rows, n, stream, limbs, sc, L, n, ElemChunks{}, a, out);
}

hipError_t hp_launch_poly_strict(const HpLimb *limbs, u32 L, u32 n, u32 rows, u64 *x, hipStream_t stream) {
    return elem_launch(k_poly_unary<1>, rows, n, stream, limbs, HpScalars{}, L, n, ElemChunks{}, x, x);
}

// ---- deep copy of device words: allocator.h:113-118 (SmartArray's copy constructor) for limbs that live in HBM ----------
// Also the engine's measured stream ceiling (bench.py "hbm_copy_ceiling_GBps"): one read and one write stream, nothing else.
#define COPY_UNROLL 4
__global__ void __launch_bounds__(ELEM_THREADS) k_copy(size_t pairs, const u64 *__restrict__ in, u64 *__restrict__ out) {
    // a workgroup moves COPY_UNROLL x 4 KiB; the loads of a round are issued together
    const size_t base = (size_t)blockIdx.x * (ELEM_THREADS * COPY_UNROLL) + threadIdx.x;
    U2 v[COPY_UNROLL];
#pragma unroll
    for (int u = 0; u < COPY_UNROLL; ++u) {
        const size_t i = base + (size_t)u * ELEM_THREADS;
        if (i < pairs) v[u] = ld_nt(in + 2 * i);
    }
#pragma unroll
    for (int u = 0; u < COPY_UNROLL; ++u) {
        const size_t i = base + (size_t)u * ELEM_THREADS;
        if (i < pairs) st_nt(out + 2 * i, v[u]);
    }
}

hipError_t hp_launch_copy(size_t words, const u64 *in, u64 *out, hipStream_t stream) {
    const size_t pairs = words >> 1;
    if (pairs) {
        const size_t per = (size_t)ELEM_THREADS * COPY_UNROLL;
        k_copy<<<dim3((unsigned)((pairs + per - 1) / per)), ELEM_THREADS, 0, stream>>>(pairs, in, out);
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    if (words & 1) return hipMemcpyAsync(out + words - 1, in + words - 1, 8, hipMemcpyDeviceToDevice, stream);
    return hipSuccess;
}

// ---- rows that live in separate blocks of registered HOST memory (hehub's SmartArray limbs, allocator.h:105-223) --------
// One kernel moves a whole polynomial between its contiguous device rows and its scattered host blocks through their
// device-visible addresses: 47-49 GB/s over PCIe either way against 11-17 GB/s for one DMA command per 256 KiB block
// (tools/ubench/ubench_pcie.hip).
template <bool TO_HOST> __global__ void __launch_bounds__(256) k_host_rows(HpHostRows rows, u64 *dev, size_t pairs) {
    typedef u64 __attribute__((ext_vector_type(2))) vv;
    vv *d = reinterpret_cast<vv *>(dev) + (size_t)blockIdx.y * pairs;
    vv *h = reinterpret_cast<vv *>(rows.p[blockIdx.y]);
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < pairs; i += (size_t)gridDim.x * blockDim.x) {
        if (TO_HOST) h[i] = d[i];
        else d[i] = h[i];
    }
}
hipError_t hp_launch_host_rows(bool to_host, const HpHostRows &rows, u32 count, size_t words, u64 *dev, hipStream_t stream) {
    if (count == 0 || words == 0) return hipSuccess;
    const size_t pairs = words >> 1;
    const unsigned gx = (unsigned)((pairs + 256 * 16 - 1) / (256 * 16));   // 16 pairs per thread
    const auto k = to_host ? k_host_rows<true> : k_host_rows<false>;
    k<<<dim3(gx ? gx : 1, count), 256, 0, stream>>>(rows, dev, pairs);
    return hipGetLastError();
}

// ---- gathers: permutation.cpp:28-75 -------------------------------------------------
__global__ void __launch_bounds__(ELEM_THREADS) k_gather(const u32 *__restrict__ perm, u32 n, u32 chunks,
                                                        const u64 *__restrict__ in, u64 *__restrict__ out) {
    const ElemTile tile(n, chunks);
    const size_t base = (size_t)tile.row * n;
    const auto words = tile.words();
    // (the gathered row is re-read line by line and wants the caches; the output is written once)
    if (tile.full()) {   // the eight index loads, then the eight gathers, in flight together
        constexpr int IT = ELEM_CHUNK / ELEM_THREADS;
        const u32 i0 = tile.begin() + threadIdx.x;
        u32 idx[IT];
        u64 v[IT];
#pragma unroll
        for (int t = 0; t < IT; ++t) idx[t] = perm[i0 + t * ELEM_THREADS];
#pragma unroll
        for (int t = 0; t < IT; ++t) v[t] = in[base + idx[t]];
#pragma unroll
        for (int t = 0; t < IT; ++t) __builtin_nontemporal_store(v[t], out + base + i0 + t * ELEM_THREADS);
        return;
    }
    for (const u32 i : words) __builtin_nontemporal_store(in[base + perm[i]], out + base + i);
}

hipError_t hp_launch_gather(const u32 *perm, u32 n, u32 rows, const u64 *in, u64 *out, hipStream_t stream) {
    return elem_launch(k_gather, rows, n, stream, perm, n, ElemChunks{}, in, out);
}

__global__ void __launch_bounds__(ELEM_THREADS) k_reverse(u32 n, u32 chunks, const u64 *__restrict__ in,
                                                         u64 *__restrict__ out) {
    const ElemTile tile(n, chunks);
    const size_t base = (size_t)tile.row * n;
    for (const u32 i : tile.words()) out[base + i] = in[base + (n - 1 - i)];
}

hipError_t hp_launch_reverse(u32 n, u32 rows, const u64 *in, u64 *out, hipStream_t stream) {
    return elem_launch(k_reverse, rows, n, stream, n, ElemChunks{}, in, out);
}

// cycle / involution of several ciphertexts in one launch, each with its own map and its two polynomials anywhere in device
// memory (hp_dev_ckks_rotate_many: the sources and maps travel as kernel arguments): out u64[count][polys][L][N], polys = 2, or 1
// for polynomial 0 alone (hp_dev_ckks_rotate_hoisted_hks moves only c0)
__global__ void __launch_bounds__(ELEM_THREADS) k_gather_many(HpGatherTable tab, u32 n, u32 chunks, u32 L, u32 polys,
                                                             u64 *__restrict__ out) {
    const ElemTile tile(n, chunks);
    const u32 b = tile.row / (polys * L), r = tile.row % (polys * L), h = r / L, k = r % L;
    const u64 *__restrict__ in = tab.src[b][h] + (size_t)k * n;
    const u32 *__restrict__ perm = tab.perm[b];
    u64 *__restrict__ o = out + (size_t)tile.row * n;
    const auto words = tile.words();
    if (!perm) {   // involution: permutation.cpp:57-75
        for (const u32 i : words) __builtin_nontemporal_store(in[n - 1 - i], o + i);
        return;
    }
    if (tile.full()) {   // (as in k_gather)
        constexpr int IT = ELEM_CHUNK / ELEM_THREADS;
        const u32 i0 = tile.begin() + threadIdx.x;
        u32 idx[IT];
        u64 v[IT];
#pragma unroll
        for (int t = 0; t < IT; ++t) idx[t] = perm[i0 + t * ELEM_THREADS];
#pragma unroll
        for (int t = 0; t < IT; ++t) v[t] = in[idx[t]];
#pragma unroll
        for (int t = 0; t < IT; ++t) __builtin_nontemporal_store(v[t], o + i0 + t * ELEM_THREADS);
        return;
    }
    for (const u32 i : words) __builtin_nontemporal_store(in[perm[i]], o + i);
}

hipError_t hp_launch_gather_many(const HpGatherTable &tab, u32 count, u32 n, u32 L, u64 *out, hipStream_t stream, u32 polys) {
    if (count == 0) return hipSuccess;
    if (count > HP_GATHER_TABLE_MAX || polys < 1 || polys > 2) return hipErrorInvalidValue;
    return elem_launch(k_gather_many, count * polys * L, n, stream, tab, n, ElemChunks{}, L, polys, out);
}

// ---- single-vector kernels (drop-in mod_arith entry points) --------------------------
template <int OP>
__global__ void __launch_bounds__(ELEM_THREADS) k_vec(HpVecConsts c, size_t n, const u64 *__restrict__ a,
                                                     const u64 *__restrict__ b, u64 *__restrict__ out) {
    for (size_t i = (size_t)blockIdx.x * ELEM_THREADS + threadIdx.x; i < n; i += (size_t)gridDim.x * ELEM_THREADS) {
        u64 r = 0;
        if (OP == HP_V_BARRETT_LAZY) r = hp_barrett_lazy(a[i], c.q, c.barrett_c);            // mod_arith.cpp:9-17
        if (OP == HP_V_BARRETT) r = hp_strict(hp_barrett_lazy(a[i], c.q, c.barrett_c), c.q);   // mod_arith.h:18-25
        if (OP == HP_V_STRICT) r = hp_strict(a[i], c.q);                                       // mod_arith.h:58-63
        if (OP == HP_V_MUL_HYBRID) {                                                           // mod_arith.cpp:64-92
            u64 lo, hi;
            hp_mul128(a[i], b[i], lo, hi);
            u64 t = hp_montgomery128_lazy(lo, hi, c.q, c.mqinv);
            r = hp_harvey_lazy(t, c.r64, c.r64h, c.q);
        }
        if (OP == HP_V_MUL_BARRETT) {                                                          // mod_arith.cpp:94-111
            u64 al, ah;
            hp_mul128(a[i], b[i], al, ah);
            // approx_quotient = ah*ch + ((ah*cl + al*ch) >> 64)   (the inner sum is a wrapping u128)
            u64 p1l, p1h, p2l, p2h;
            hp_mul128(ah, c.c128_lo, p1l, p1h);
            hp_mul128(al, c.c128_hi, p2l, p2h);
            u64 sl = p1l + p2l;
            u64 sh = p1h + p2h + (sl < p1l ? 1ull : 0ull);
            u64 qhat = ah * c.c128_hi + sh;
            r = al - c.q * qhat;
        }
        if (OP == HP_V_MONTGOMERY128) r = hp_montgomery128_lazy(a[2 * i], a[2 * i + 1], c.q, c.mqinv);
        out[i] = r;
    }
}

hipError_t hp_launch_vec(int op, const HpVecConsts &c, size_t n, const u64 *a, const u64 *b, u64 *out,
                         hipStream_t stream) {
    static constexpr decltype(&k_vec<0>) kernels[] = {   // indexed by HpVecOp
        k_vec<HP_V_BARRETT_LAZY>, k_vec<HP_V_BARRETT>,     k_vec<HP_V_STRICT>,
        k_vec<HP_V_MUL_HYBRID>,   k_vec<HP_V_MUL_BARRETT>, k_vec<HP_V_MONTGOMERY128>};
    if (n == 0) return hipSuccess;
    if (op < 0 || op >= (int)(sizeof kernels / sizeof *kernels)) return hipErrorInvalidValue;
    size_t blocks = (n + ELEM_THREADS - 1) / ELEM_THREADS;
    if (blocks > 256 * 16) blocks = 256 * 16;
    kernels[op]<<<dim3((unsigned)blocks), ELEM_THREADS, 0, stream>>>(c, n, a, b, out);
    return hipGetLastError();
}
