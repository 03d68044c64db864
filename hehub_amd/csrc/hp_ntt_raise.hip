// hp_ntt_raise.hip -- ModRaise for N = 2^11 .. 2^15: the tiled forward transform of hp_ntt_fast.hip with the centring of a
// coefficient row modulo q_0 and its reduction into the item's modulus done in the LOADS (hp_dev_ckks_mod_raise).
//
// A ciphertext at its last limb is raised to the chain q_0 .. q_{L-1} by reading its strict coefficients c modulo q_0 as the
// centred integers v (c below floor(q_0 / 2): c, else c - q_0) and transforming v modulo every q_m, m >= 1.  All L - 1 items of
// a polynomial read the same row (the job shape of the fused drop: src_kstride 0, items numbered by groups of moduli so that
// the row comes from HBM once per group), and the lifted block u64[L - 1][N] of the three-call form -- inverse transform,
// hp_dev_rns_base_from_single, forward transform -- is never written: per polynomial 1 + (L - 1) rows cross HBM here instead
// of the 3 (L - 1) of its last two calls.
//
// The load-side arithmetic is that of the fused drop's prologue (hp_ntt_fast.hip: DropPre) without the drop's subtraction and
// final multiplication: v = strict(barrett_q(c)), + q - (q_0 mod q) when c >= floor(q_0 / 2); v is below 2q, a lazy word of the
// butterflies.  Its own translation unit over hp_ntt_tile.h, so that no instantiation of hp_ntt_fast.hip changes; the pass
// schedule, geometry, loads, stores and staging are the header's.
#include "hp_ntt_tile.h"

namespace {

// load-side work of the first slot (pass_slots, hp_ntt_tile.h): the lane-pair swap at N = 32768, then centre and reduce
template <bool SWAP> struct RaisePre {
    static constexpr bool on = true;
    u64 q, bc, bump, half;
    u32 n0, n1;
    HP_DEV void operator()(u64 (&x)[32], int r) const {
        if (SWAP) lazy_swap(x, r);
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            const u64 c = x[r + e];
            u64 v = hp_strict(hp_barrett_lazy_nq(c, bc, n0, n1), q);
            if (c >= half) v += bump;
            x[r + e] = v;
        }
    }
};

// the lazy Harvey butterfly as the policy of pass_slots (hp_ntt_fast.hip: HarveyBf; arithmetic stays out of the shared header)
struct HarveyBf {
    u64 two_q;
    u32 n0, n1;
    HP_DEV HarveyBf(u64 nq, u64 two_q_) : two_q(two_q_), n0((u32)nq), n1((u32)(nq >> 32)) {}
    template <bool SC> HP_DEV void pair(u64 &a0, u64 &a1, u64 &b0, u64 &b1, const u64x2 &ta, const u64x2 &tb) const {
        if constexpr (SC) hp_butterfly2_nq_sw(a0, a1, b0, b1, ta.x, ta.y, tb.x, tb.y, two_q, n0, n1);
        else hp_butterfly2_nq(a0, a1, b0, b1, ta.x, ta.y, tb.x, tb.y, two_q, n0, n1);
    }
};

template <int LOGN>
__global__ void __launch_bounds__(Geo<LOGN>::T, Geo<LOGN>::MINW) k_ntt_raise(HpNttJob job, HpRaiseArgs ra) {
    using G = Geo<LOGN>;
    using AD = Addr<LOGN, LOGN == 15>;
    __shared__ u32 lds[AD::WORDS];
    __shared__ u64v2 lds_tw[31 * (1 << G::A)];
    const u32 w = hp_xcd_remap(blockIdx.x, job.W);
    HpItem it;
    if (!hp_decode_item(job, w, it)) return;
    // the limb's constants and table pointers through the scalar cache, as in k_ntt_fwd
    const cptr_limb lp = (cptr_limb)(job.limbs + __builtin_amdgcn_readfirstlane(it.limb));
    const u64 q = lp->q, two_q = lp->two_q, nq = lp->neg_q;
    const u32 tid = threadIdx.x;
    const HarveyBf bf(nq, two_q);
    AD ad;
    ad.init(tid);
    const u64v2 stg = fwd_stage_issue<LOGN>(lp, tid);

    u64 x[32];
    load_flight<LOGN, G::PB == 0>(it.src, tid, x);   // N = 32768: registers left as loaded, sorted by the first stage
    fwd_stage_write<LOGN>(lds_tw, tid, stg);
    // pass A with the centring in its first slot: the first butterflies run while the later loads are still in flight
    const RaisePre<G::PB == 0> pre{q, lp->barrett_c, q - ra.r[it.limb], ra.half, (u32)nq, (u32)(nq >> 32)};
    fwd_pass<4, G::PB, STab>(x, STab(lp->fwd_ref + 1), 1u, 0u, bf, pre);
    exchange<LOGN, LAY_A, LAY_B, true>(x, lds, ad);
    fwd_pass<4, 0>(x, LTab(lds_tw), 1u << G::A, tid >> 5, bf);
    exchange<LOGN, LAY_B, LAY_C, false>(x, lds, ad);
    fwd_pass<4, 0>(x, BTab(lp->fwd_k + 31 * (1 << G::A)), (u32)G::T, tid, bf);
    // final fold (ntt.cpp:171-175), then below 2q at every modulus (hp_lazy_below_2q: the fold alone does not give that)
    {
        const u32 k = lp->k, fix = lp->fix;
#pragma unroll
        for (int r = 0; r < 32; ++r) x[r] = hp_lazy_below_2q(hp_shift_fold(x[r], q, k, fix), two_q);
    }
    exchange<LOGN, LAY_C, LAY_S, false>(x, lds, ad);
    store_stream(it.dst, stream_off(tid), x);
}

} // namespace

hipError_t hp_launch_ntt_raise(const HpNttJob &job, const HpRaiseArgs &ra, hipStream_t stream) {
    if (job.W == 0) return hipSuccess;
    if (job.inverse || job.mode != HP_NTT_BATCH || job.limbs_a || job.L > HP_MAX_LIMBS) return hipErrorNotSupported;
    return for_logn(job, [&](auto n) {
        constexpr int LOGN = decltype(n)::value;
        k_ntt_raise<LOGN><<<job.W, Geo<LOGN>::T, 0, stream>>>(job, ra);
        return hipGetLastError();
    });
}
