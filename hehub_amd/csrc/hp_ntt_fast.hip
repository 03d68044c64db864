// hp_ntt_fast.hip -- register-tiled negacyclic NTT / INTT for N = 2^11 .. 2^15 on gfx950.
//
// One workgroup transforms one RNS limb.  The limb is read from HBM once and written once
// (algorithmic traffic 16*N bytes); everything in between happens in
// registers and LDS:
//
//   * every thread keeps 32 coefficients (64 VGPRs) and runs up to five radix-2 stages on
//     them per pass -- the butterflies are exactly the reference's lazy Harvey butterflies
//     (ntt.cpp:160-166), only their schedule changes, so raw output words are identical;
//   * N = 32 * T coefficients, T = N/32 threads; logN = a + 5 + 5 stages = three passes
//     (A: top a bits, B: bits 9..5, C: bits 4..0 of the coefficient index; the inverse runs
//     them in the opposite order, C' B' A');
//   * between passes the workgroup transposes through LDS, 32 bits at a time (low words, then
//     high words), so a whole limb needs only 4*N bytes of LDS: 128 KiB at N = 32768 (one
//     workgroup of 16 waves per CU) and 64 KiB at N = 16384 (two workgroups per CU);
//   * the exchange between the passes that work inside a 1024-coefficient block (B <-> C) and
//     the transposition that makes the HBM stores/loads of the contiguous pass coalesced are
//     wave-local: each wave owns 2048 consecutive coefficients there, so they need no
//     s_barrier and waves drift apart, overlapping one wave's LDS traffic with another's
//     integer multiplies.  Only the A <-> B exchange is workgroup-wide (3 barriers);
//   * LDS word address of coefficient i is i ^ ((i >> 5) & 31) (forward kernels at N = 32768: i + (i >> 5), a padded buffer
//     whose register offsets are all immediates): every ds_read_b32 / ds_write_b32 of every exchange hits 32 distinct banks
//     per 32-lane group;
//   * twiddles are (w, floor(w*2^64/q)) pairs read as one 16-byte load from per-modulus tables
//     laid out [slot][class] (hp_tables.cpp) so a wavefront reads consecutive pairs; the
//     tables are shared by the whole batch and live in L2 -- work items are numbered
//     modulus-major and handed to XCDs in contiguous slices (hp_xcd_remap) to keep them there.
//
// The kernel is bound by the integer ALUs, not by HBM: 10 multiply-type instructions of 16 per butterfly
// (tools/ubench/*.hip), 88 % VALUBusy in the PMC passes at 35-44 % of HBM peak; see DESIGN.md 4.1.
//
// What is here: the Harvey butterfly policy (HarveyBf), the load-side functor of the fused drop (DropPre), and the integer
// arithmetic of the kernels' prologues and epilogues.  The pass schedule, geometry, loads, stores, staging, the drop epilogue's
// row pipeline and the launch dispatch are hp_ntt_tile.h's, shared with hp_ntt_a.hip.
#include "hp_ntt_tile.h"

HP_TRACE_STORAGE(hp_debug_trace)

namespace {

// load-side work of a forward pass's first slot (pass_slots, hp_ntt_tile.h):
//   SwapPre  N = 32768: registers still hold the loads as they arrived; the lane-pair swap sorts them into columns (load_flight)
//   DropPre  fused drop-last-prime: that swap, then the Barrett / centring / [* t] prologue of rescaling.cpp:54-69, mod_switch.cpp:52-70
template <bool SWAP, bool BGV, bool SMALL> struct DropPre {
    static constexpr bool on = true;
    u64 q, bc, bump, half, tk, tkh;
    u32 n0, n1;
    HP_DEV void operator()(u64 (&x)[32], int r) const {
        if (SWAP) lazy_swap(x, r);
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            const u64 c = x[r + e];
            u64 v = SMALL ? hp_strict(c, q) : hp_strict(hp_barrett_lazy_nq(c, bc, n0, n1), q);   // SMALL: c < q_last <= 2q
            if (c >= half) v += bump;
            if (BGV) v = hp_harvey_lazy_nq(v, tk, tkh, n0, n1);
            x[r + e] = v;
        }
    }
};

// the lazy Harvey butterfly (ntt.cpp:160-166) as the policy of pass_slots: two butterflies per call, the form with the twiddles
// in SGPRs where the table is a scalar one
struct HarveyBf {
    u64 two_q;
    u32 n0, n1;
    HP_DEV HarveyBf(u64 nq, u64 two_q_) : two_q(two_q_), n0((u32)nq), n1((u32)(nq >> 32)) {}
    template <bool SC> HP_DEV void pair(u64 &a0, u64 &a1, u64 &b0, u64 &b1, const u64x2 &ta, const u64x2 &tb) const {
        if constexpr (SC) hp_butterfly2_nq_sw(a0, a1, b0, b1, ta.x, ta.y, tb.x, tb.y, two_q, n0, n1);
        else hp_butterfly2_nq(a0, a1, b0, b1, ta.x, ta.y, tb.x, tb.y, two_q, n0, n1);
    }
};

// FLAV (fused drop only): 0 = every option decided at run time; 1..5 = the shapes of the CKKS / BGV pipelines with the options
// fixed at compile time (Barrett prologue, no final multiplication; 1: CKKS, no addend; 2: CKKS, addend on both polynomials;
// 3 / 4: the same with the BGV factors; 5: CKKS, addend on polynomial 0 only = rotations), which takes ~100 uniform branches
// out of the prologue and the store loop
template <int LOGN, bool DROP, int FLAV = 0, bool SMALL = false>
HP_DEV void ntt_fwd_body(const HpNttJob &job, const HpDropArgs *da) {
    using G = Geo<LOGN>;
    using AD = Addr<LOGN, LOGN == 15>;   // (re-checked in round 3 with the general PB form below: N = 16384 / 8192 still spill 28 / 39-46 registers with it)
    __shared__ u32 lds[AD::WORDS];
    __shared__ u64v2 lds_tw[31 * (1 << G::A)];
    TRACE_ENTRY
    const u32 w = hp_xcd_remap(blockIdx.x, job.W);
    HpItem it;
    if (!hp_decode_item(job, w, it)) return;
    // the limb's constants and table pointers through the scalar cache (constant address space): as vector loads they would
    // queue behind the coefficient loads and the first pass could not start before nearly all of those are back
    const cptr_limb lp = (cptr_limb)(job.limbs + __builtin_amdgcn_readfirstlane(it.limb));
    const u64 q = lp->q, two_q = lp->two_q, nq = lp->neg_q;
    const u32 tid = threadIdx.x;
    const HarveyBf bf(nq, two_q);
    AD ad;
    ad.init(tid);
    const u64v2 stg = fwd_stage_issue<LOGN>(lp, tid);

    TRACE_DECL
    TRACE_MARK();
    u64 x[32];
    // load-side work deferred into the first stage: the plain N = 32768 kernel (lane-pair swap) and the compile-time flavours of
    // the fused drop (swap + Barrett / centring prologue); the run-time flavour 0 (hybrid key switch inputs) keeps the eager form
    // (N = 32768 only: -2 % on the launch there, +2 % at N = 8192 where two workgroups per CU hide the load phase anyway)
    constexpr bool LZ_DROP = DROP && FLAV != 0 && G::PB == 0;
    constexpr bool LZ = (!DROP && G::PB == 0) || LZ_DROP;   // registers left as loaded
    load_flight<LOGN, LZ>(it.src, tid, x);
    fwd_stage_write<LOGN>(lds_tw, tid, stg);
    if (DROP) {
        // rescaling.cpp:54-69 / mod_switch.cpp:52-70 while the coefficients are still in flight order:
        // rem = strict_barrett_{q_k}(c) (+ q_k - (q_last mod q_k) if c >= q_last/2) (BGV: * t)
        const u32 k = it.limb;
        const u64 bc = lp->barrett_c, bump = q - da->dc.r[k], half = da->dc.half_q_last;
        const u64 tk = da->dc.t[k], tkh = da->dc.t_h[k];
        const bool bgv = FLAV ? (FLAV == 3 || FLAV == 4) : da->dc.bgv != 0;
        if (!LZ_DROP && (FLAV || !da->raw_input)) {
#pragma unroll
            for (int r = 0; r < 32; ++r) {
                const u64 c = x[r];
                u64 v = SMALL ? hp_strict(c, q) : hp_strict(hp_barrett_lazy_nq(c, bc, (u32)nq, (u32)(nq >> 32)), q);
                if (c >= half) v += bump;
                if (bgv) v = hp_harvey_lazy_nq(v, tk, tkh, (u32)nq, (u32)(nq >> 32));
                x[r] = v;
            }
        }
        if (!FLAV && da->comb) {
            // hybrid key switch, ModDown merged with the rescale: x = rem_k + (P mod q_k) * centre_k(c), c = the strict
            // coefficients modulo q_last of the relinearised last limb (one row per polynomial, read by every limb)
            // Eight registers (four 16-byte loads) at a time with the next four loads in flight.  The loads are inline asm: left
            // to itself the compiler, short of registers beside x, issues the sixteen loads one by one with a full wait after
            // each.  It does not count asm loads, so the waits are explicit (vector loads return in order: "at most four
            // outstanding" means the current four are back); each wait is tied to the registers it guards.
            typedef u64 __attribute__((ext_vector_type(2))) vv;
            const u64 *crow = da->comb + (size_t)it.poly * G::N;
            const u64 pm = da->comb_mul[k], pmh = da->comb_mul_h[k], cbump = q - da->comb_r[k], chalf = da->comb_half;
            const bool odd = (tid & 1u) != 0;
            vv ca[4], cb[4];
            auto issue = [&](vv (&d)[4], int ch) {
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int r = 8 * ch + 2 * i;
                    const u64 *a = (G::PB == 0) ? crow + (tid & ~1u) + ((size_t)(r + (odd ? 1 : 0)) << 10)
                                                : crow + ((size_t)tid << G::PB) + ((size_t)(r >> G::PB) << 10) + (r & ((1 << G::PB) - 1));
                    asm volatile("global_load_dwordx4 %0, %1, off" : "=&v"(d[i]) : "v"(a) : "memory");
                }
            };
            issue(ca, 0);
#pragma unroll
            for (int ch = 0; ch < 4; ++ch) {
                vv(&cur)[4] = (ch & 1) ? cb : ca;
                vv(&nxt)[4] = (ch & 1) ? ca : cb;
                if (ch + 1 < 4) {
                    issue(nxt, ch + 1);
                    asm volatile("s_waitcnt vmcnt(4)" : "+v"(cur[0]), "+v"(cur[1]), "+v"(cur[2]), "+v"(cur[3]) : : "memory");
                } else {
                    asm volatile("s_waitcnt vmcnt(0)" : "+v"(cur[0]), "+v"(cur[1]), "+v"(cur[2]), "+v"(cur[3]) : : "memory");
                }
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    u64 c0 = cur[i].x, c1 = cur[i].y;
                    if (G::PB == 0) {   // lane-pair swap as in load_flight
                        const u64 keep = odd ? c1 : c0, send = odd ? c0 : c1;
                        const u64 recv = from_pair_lane(send);
                        c0 = odd ? recv : keep;
                        c1 = odd ? keep : recv;
                    }
                    const int r = 8 * ch + 2 * i;
                    u64 v0 = hp_strict(hp_barrett_lazy_nq(c0, bc, (u32)nq, (u32)(nq >> 32)), q);
                    u64 v1 = hp_strict(hp_barrett_lazy_nq(c1, bc, (u32)nq, (u32)(nq >> 32)), q);
                    if (c0 >= chalf) v0 += cbump;
                    if (c1 >= chalf) v1 += cbump;
                    x[r] = hp_add_lazy(x[r], hp_harvey_lazy_nq(v0, pm, pmh, (u32)nq, (u32)(nq >> 32)), two_q);
                    x[r + 1] = hp_add_lazy(x[r + 1], hp_harvey_lazy_nq(v1, pm, pmh, (u32)nq, (u32)(nq >> 32)), two_q);
                }
            }
        }
    }
#ifdef HP_TRACE
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#endif
    TRACE_MARK();   // 1: coefficients have arrived
    // pass A: global stages 1..A, wave-uniform twiddles seq[1 .. 2^A - 1]
    if constexpr (LZ_DROP) {
        const u32 k = it.limb;
        const DropPre<G::PB == 0, (FLAV == 3 || FLAV == 4), SMALL> pre{q, lp->barrett_c, q - da->dc.r[k], da->dc.half_q_last, da->dc.t[k], da->dc.t_h[k],
                                                    (u32)nq, (u32)(nq >> 32)};
        fwd_pass<4, G::PB, STab>(x, STab(lp->fwd_ref + 1), 1u, 0u, bf, pre);
    } else if constexpr (LZ) {
        fwd_pass<4, G::PB, STab>(x, STab(lp->fwd_ref + 1), 1u, 0u, bf, SwapPre());
    } else {
        fwd_pass<4, G::PB, STab>(x, STab(lp->fwd_ref + 1), 1u, 0u, bf);
    }
    TRACE_MARK();   // 2
    exchange<LOGN, LAY_A, LAY_B, true>(x, lds, ad);
    TRACE_MARK();   // 3
    // pass B: global stages A+1..A+5, twiddles depend on the 1024-block
    fwd_pass<4, 0>(x, LTab(lds_tw), 1u << G::A, tid >> 5, bf);
    TRACE_MARK();   // 4
    exchange<LOGN, LAY_B, LAY_C, false>(x, lds, ad);
    TRACE_MARK();   // 5
    // pass C: global stages A+6..logN, per-thread twiddles
    fwd_pass<4, 0>(x, BTab(lp->fwd_k + 31 * (1 << G::A)), (u32)G::T, tid, bf);
    TRACE_MARK();   // 6
    // final fold (ntt.cpp:171-175)
    {
        const u32 k = lp->k, fix = lp->fix;
#pragma unroll
        for (int r = 0; r < 32; ++r) x[r] = hp_shift_fold(x[r], q, k, fix);
    }
    if constexpr (DROP && FLAV == 0) {
        // hybrid ModDown (raw rows: the engine's own pipeline, no hehub words to follow): the epilogue's lazy subtraction takes
        // NTT(rem) below 2q, which the fold alone does not give at every modulus (hp_lazy_below_2q, hp_device.h)
        if (da->raw_input) {
#pragma unroll
            for (int r = 0; r < 32; ++r) x[r] = hp_lazy_below_2q(x[r], two_q);
        }
    }
    TRACE_MARK();   // 7: fold done
    exchange<LOGN, LAY_C, LAY_S, false>(x, lds, ad);
    TRACE_MARK();   // 8
    if (!DROP) {
        const size_t off = stream_off(tid);
        if (job.mode == HP_NTT_SPREAD && ((job.pack_mask >> it.limb) & 1u)) store_stream_pack48<LOGN>(it.dst, off, x);
        else store_stream(it.dst, off, x);
    } else {
        // rescaling.cpp:72-74 / mod_switch.cpp:72-76 (+ the += of relinearize, ckks/arith.cpp:70-71):
        // out = ((x - NTT(rem)) * inv) [* (q_last mod t)] [+ addend], all in the lazy representation
        const u32 k = it.limb;
        const DropRows<LOGN, FLAV> io(da, k, it.poly, tid);
        const u64 inv = da->dc.inv[k], invh = da->dc.inv_h[k], ql = da->dc.qlt[k], qlh = da->dc.qlt_h[k];
        const bool bgv = FLAV ? (FLAV == 3 || FLAV == 4) : da->dc.bgv != 0, fin_on = FLAV ? false : da->fin_on != 0;
        const u64 fin = da->fin[k], finh = da->fin_h[k];
        const u32 n0 = (u32)nq, n1 = (u32)(nq >> 32);
        io.run([&](auto add_tag, const V2 &xv, const V2 &av, int s) {
            u64 v0 = hp_harvey_lazy_nq(hp_sub_lazy(xv.x, x[2 * s], two_q), inv, invh, n0, n1);
            u64 v1 = hp_harvey_lazy_nq(hp_sub_lazy(xv.y, x[2 * s + 1], two_q), inv, invh, n0, n1);
            if (bgv) {
                v0 = hp_harvey_lazy_nq(v0, ql, qlh, n0, n1);
                v1 = hp_harvey_lazy_nq(v1, ql, qlh, n0, n1);
            }
            if (decltype(add_tag)::value) {
                v0 = hp_add_lazy(v0, av.x, two_q);
                v1 = hp_add_lazy(v1, av.y, two_q);
            }
            if (fin_on) {
                v0 = hp_harvey_lazy_nq(v0, fin, finh, n0, n1);
                v1 = hp_harvey_lazy_nq(v1, fin, finh, n0, n1);
            }
            return V2{v0, v1};
        }, [](const V2 &v) { return v; });
    }
    TRACE_MARK();   // 9: stores issued
    TRACE_FLUSH();
}

template <int LOGN>
__global__ void __launch_bounds__(Geo<LOGN>::T, Geo<LOGN>::MINW) k_ntt_fwd(HpNttJob job) {
    ntt_fwd_body<LOGN, false>(job, nullptr);
}

// forward NTT with the drop-last-prime prologue/epilogue fused in (HpDropArgs in kernel-argument memory)
template <int LOGN, int FLAV, bool SMALL>
__global__ void __launch_bounds__(Geo<LOGN>::T, Geo<LOGN>::MINW) k_ntt_fwd_drop(HpNttJob job, HpDropArgs da) {
    ntt_fwd_body<LOGN, true, FLAV, SMALL>(job, &da);
}

// ---- inverse kernel ----------------------------------------------------------------------------
// (InvGeo, hp_ntt_tile.h: several limbs of one modulus per workgroup at N <= 8192)
template <int LOGN, bool STRICT, bool PSCAL>
__global__ void __launch_bounds__(InvGeo<LOGN>::TT, Geo<LOGN>::MINW) k_ntt_inv(HpNttJob job) {
    using G = Geo<LOGN>;
    constexpr int LPW = InvGeo<LOGN>::LPW;
    __shared__ u32 lds_all[Addr<LOGN>::WORDS * LPW];
    __shared__ u64v2 lds_tw[31 * 32];
    TRACE_ENTRY
    const u32 sub = threadIdx.x / G::T, tid = threadIdx.x % G::T;   // limb of the workgroup, thread within the limb
    u32 *lds = lds_all + sub * Addr<LOGN>::WORDS;
    HpItem it;
    const bool active = inv_item<LOGN>(job, sub, it);
    // the limb's constants and table pointers through the scalar cache (constant address space): as vector loads they would
    // queue behind the coefficient loads and the first pass could not start before nearly all of those are back
    const cptr_limb lp = (cptr_limb)(job.limbs + __builtin_amdgcn_readfirstlane(it.limb));
    const u64 q = lp->q, two_q = lp->two_q, nq = lp->neg_q;
    const HarveyBf bf(nq, two_q);
    Addr<LOGN> ad;
    ad.init(tid);
    // (the twiddle staging, the stream load and the layout-A store of the inverse kernels stay written out in both files: as
    // helpers of hp_ntt_tile.h each of them changed the instruction streams of the N <= 16384 kernels)
    constexpr int TT = InvGeo<LOGN>::TT, NSTG = InvGeo<LOGN>::NSTG;
    u64v2 stg[NSTG];
#pragma unroll
    for (int i = 0; i < NSTG; ++i) {
        const u32 e = threadIdx.x + (u32)i * TT;
        stg[i] = (e < 31u * 32u) ? ((gptr_u64x2)(lp->inv_k + 31))[e] : u64v2{0, 0};
    }

    TRACE_DECL
    TRACE_MARK();   // 0: entry (constants and staging loads issued)
    u64 x[32];
    {
        const u64 *s = it.src + (((size_t)(tid >> 6)) << 11) + ((tid & 63u) << 1);
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const V2 v = ld_stream(s + ((size_t)r << 7));
            x[2 * r] = v.x;
            x[2 * r + 1] = v.y;
        }
    }
#pragma unroll
    for (int i = 0; i < NSTG; ++i) {
        const u32 e = threadIdx.x + (u32)i * TT;
        if (e < 31u * 32u) lds_tw[e] = stg[i];
    }
#ifdef HP_TRACE
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#endif
    TRACE_MARK();   // 1: coefficients have arrived
    exchange<LOGN, LAY_S, LAY_C, false>(x, lds, ad);
    TRACE_MARK();   // 2
    // pass A': levels 0..4 (pairs 1,2,4,8,16 apart), wave-uniform twiddles
    inv_pass<0, 4>(x, STab(lp->inv_k), 1u, 0u, bf);
    TRACE_MARK();   // 3
    exchange<LOGN, LAY_C, LAY_B, false>(x, lds, ad);
    TRACE_MARK();   // 4
    // The staged twiddles are read by other waves in pass B'; everything before it is wave-local, so this is the first point
    // where the waves have to meet.  (The barrier used to sit right after the loads: a workgroup's vector loads queue in wave
    // order behind each other at the CU's ~17 B/clk, the last wave gets its staging load out ~10 k cycles after the first, and
    // until then the first waves sat at the barrier with their coefficients long there: -5..8 % per launch at N = 32768.)
    __syncthreads();
    // pass B': levels 5..9, twiddles depend on j = tid & 31
    inv_pass<0, 4>(x, LTab(lds_tw), 32u, tid & 31u, bf);
    TRACE_MARK();   // 5
    exchange<LOGN, LAY_B, LAY_A, true>(x, lds, ad);
    TRACE_MARK();   // 6
    // pass C': levels 10..logN-1, per-thread twiddles
    // (twiddle ring of the last pass: 4 slots at N = 32768 / 8192; 3 at N = 16384 and 2 at N <= 4096, where the fourth costs spilled
    // registers -- 9 -> 4 and 19 -> 8 -- and buys nothing: +0.5 % / +3 % on the launch, less scratch traffic in WRITE_SIZE)
    constexpr int RING = LOGN == 14 ? 3 : LOGN <= 12 ? 2 : BTab::depth;
    inv_pass<G::PB, 4, BTab, RING>(x, BTab(lp->inv_k + 31 + 31 * 32), (u32)G::T, tid, bf);
    TRACE_MARK();   // 7
    if constexpr (InvGeo<LOGN>::STREAM_EPILOGUE) {
        // N <= 8192: in layout A a thread owns 2^PB >= 4 consecutive coefficients, so a 16-byte store instruction would write
        // a quarter or half of every cache line it touches: measured 1.9 x the algorithmic write traffic at N = 4096
        // (WRITE_SIZE, rocprofv3).  Fold in place, transpose once more (layout S, as the forward kernel stores), then the
        // psi^-i N^-1 pairs are read and the words written 16 contiguous bytes per lane, 1 KiB per wave instruction.
        const u32 k = lp->k, fix = lp->fix;
#pragma unroll
        for (int r = 0; r < 32; ++r) x[r] = hp_shift_fold(x[r], q, k, fix);
        exchange<LOGN, LAY_A, LAY_S, true>(x, lds, ad);
        if (!active) return;   // (after the last barrier of the kernel)
        const size_t off = (((size_t)(tid >> 6)) << 11) + ((tid & 63u) << 1);
        const BTab sc(lp->inv_ref + G::N);   // pairs of coefficient off + (s << 7) + e: row = s, 128 pairs per row, lane part off + e
        u64 *d = it.dst + off;
        const u64 psc = job.post_scalar, psh = job.post_scalar_h;
#pragma unroll
        for (int s0 = 0; s0 < 16; s0 += 2) {
            u64x2 f[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) f[e] = sc.at((u32)(s0 + (e >> 1)), 128u, (u32)off + (u32)(e & 1));
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int r = 2 * s0 + e;
                u64 v = hp_harvey_lazy_nq(x[r], f[e].x, f[e].y, (u32)nq, (u32)(nq >> 32));
                if (PSCAL) v = hp_harvey_lazy_nq(v, psc, psh, (u32)nq, (u32)(nq >> 32));
                if (STRICT) v = hp_strict(v, q);
                x[r] = v;
            }
            st_stream(d + ((size_t)s0 << 7), V2{x[2 * s0], x[2 * s0 + 1]});
            st_stream(d + ((size_t)(s0 + 1) << 7), V2{x[2 * s0 + 2], x[2 * s0 + 3]});
            __builtin_amdgcn_sched_barrier(0);
        }
        return;
    }
    // fold, multiply by psi^-i * N^-1 (ntt.cpp:214-222), optional scalar + strict reduction, store (layout A)
    {
        const u32 k = lp->k, fix = lp->fix;
        const BTab sc(lp->inv_ref + G::N);   // pair of coefficient (kk << 10) + (tid << PB) + pp: row = kk, 1024 pairs per row
        u64 *d = it.dst + ((size_t)tid << G::PB);
        const u64 psc = job.post_scalar, psh = job.post_scalar_h;
#pragma unroll
        for (int r0 = 0; r0 < 32; r0 += 4) {
            u64x2 f[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int r = r0 + e, kk = r >> G::PB, pp = r & ((1 << G::PB) - 1);
                f[e] = sc.at((u32)kk, 1024u, (tid << G::PB) + (u32)pp);
            }
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int r = r0 + e;
                u64 v = hp_harvey_lazy_nq(hp_shift_fold(x[r], q, k, fix), f[e].x, f[e].y, (u32)nq, (u32)(nq >> 32));
                if (PSCAL) v = hp_harvey_lazy_nq(v, psc, psh, (u32)nq, (u32)(nq >> 32));
                if (STRICT) v = hp_strict(v, q);
                x[r] = v;
            }
            __builtin_amdgcn_sched_barrier(0);
        }
        TRACE_MARK();   // 8: scaled
        if (!active) return;   // (after the last barrier of the kernel)
        if (G::PB == 0) {   // mirror of the forward load: lane pairs assemble 16-byte stores
            const bool odd = (tid & 1u) != 0;
            u64 *dp = it.dst + (tid & ~1u);
#pragma unroll
            for (int p = 0; p < 16; ++p) {
                const u64 recv = from_pair_lane(odd ? x[2 * p] : x[2 * p + 1]);
                V2 v;
                v.x = odd ? recv : x[2 * p];
                v.y = odd ? x[2 * p + 1] : recv;
                st_stream(dp + ((size_t)(2 * p + (odd ? 1 : 0)) << 10), v);
            }
        }
#pragma unroll
        for (int kk = 0; kk < (G::PB == 0 ? 0 : (1 << G::A)); ++kk) {
            if (G::PB == 0) {
            } else {
#pragma unroll
                for (int pp = 0; pp < (1 << G::PB); pp += 2) {
                    V2 v{x[(kk << G::PB) | pp], x[(kk << G::PB) | pp | 1]};
                    st_stream(d + ((size_t)kk << 10) + pp, v);
                }
            }
        }
    }
    TRACE_MARK();   // 9: stores issued
    TRACE_FLUSH();
}

template <int LOGN> hipError_t launch(const HpNttJob &job, hipStream_t stream) {
    if (!job.inverse) {
        k_ntt_fwd<LOGN><<<job.W, Geo<LOGN>::T, 0, stream>>>(job);
        return hipGetLastError();
    }
    constexpr int TT = InvGeo<LOGN>::TT;
    if (job.mode != HP_NTT_BATCH || job.pair_moduli) return hipErrorNotSupported;
    const u32 grid = InvGeo<LOGN>::grid(job);
    if (job.use_post_scalar && job.strict) k_ntt_inv<LOGN, true, true><<<grid, TT, 0, stream>>>(job);
    else if (job.use_post_scalar) return hipErrorNotSupported;
    else if (job.strict) k_ntt_inv<LOGN, true, false><<<grid, TT, 0, stream>>>(job);
    else k_ntt_inv<LOGN, false, false><<<grid, TT, 0, stream>>>(job);
    return hipGetLastError();
}

template <int LOGN> hipError_t launch_drop(const HpNttJob &job, const HpDropArgs &da, hipStream_t stream) {
    bool small;   // (SMALL: the prologue's Barrett quotient is not needed, see HpDropArgs)
    const int flav = hp_drop_flavour_b(da, &small);
    for_index<0, 5>(flav, [&](auto f) {
        constexpr int F = decltype(f)::value;   // (flavour 0 has no SMALL form: hp_drop_flavour_b never asks for it)
        if (small) k_ntt_fwd_drop<LOGN, F, F != 0><<<job.W, Geo<LOGN>::T, 0, stream>>>(job, da);
        else k_ntt_fwd_drop<LOGN, F, false><<<job.W, Geo<LOGN>::T, 0, stream>>>(job, da);
    });
    return hipGetLastError();
}

} // namespace

hipError_t hp_launch_ntt_fast_drop(const HpNttJob &job, const HpDropArgs &da, hipStream_t stream) {
    if (job.W == 0) return hipSuccess;
    return for_logn(job, [&](auto n) { return launch_drop<decltype(n)::value>(job, da, stream); });
}

hipError_t hp_launch_ntt_fast(const HpNttJob &job, hipStream_t stream) {
    if (job.W == 0) return hipSuccess;
    return for_logn(job, [&](auto n) { return launch<decltype(n)::value>(job, stream); });
}
