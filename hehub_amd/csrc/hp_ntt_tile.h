// hp_ntt_tile.h -- everything of the tiled transforms that is not arithmetic, shared by hp_ntt_fast.hip (exact Harvey
// butterflies, parity level B) and hp_ntt_a.hip (error-free FP64 residue butterflies, parity level A): geometry, twiddle-table
// readers, LDS exchange layouts, the slot schedule of a pass over a butterfly policy, streaming HBM accesses, the forward kernels'
// load, twiddle staging and stores, the inverse kernels' geometry and item decode, the row streams and software pipeline of the
// fused drop epilogue, and the launch dispatch.  The two .hip files keep their butterfly policy, their Pre functors and the
// arithmetic of their prologues and epilogues: no FP64 arithmetic here, it would be compiled under the other file's contraction
// flags.  (The inverse kernels' staging, stream load and layout-A store are written out in both files: see there.)
// See the head of hp_ntt_fast.hip for the schedule.
#pragma once
#include "hp_kernels.h"
#include "hp_ntt_job.h"
#include <type_traits>
#include <utility>

namespace {

template <int LOGN> struct Geo {
    static constexpr int A = LOGN - 10;          // stages of pass A (1..5)
    static constexpr int PB = 5 - A;             // passenger bits of pass A's register index
    static constexpr int T = 1 << (LOGN - 5);    // threads per workgroup
    static constexpr int N = 1 << LOGN;
    static constexpr int MINW = 4;                // waves per SIMD wanted (<= 128 VGPRs)
};

HP_DEV u32 lo32(u64 v) { return (u32)v; }
HP_DEV u32 hi32(u64 v) { return (u32)(v >> 32); }
HP_DEV u64 mk64(u32 lo, u32 hi) { return ((u64)hi << 32) | lo; }

// ---- passes ---------------------------------------------------------------------------------
// A pass runs up to five radix-2 stages on the 5-bit register index.  Its twiddles are numbered by
// "slot" 0..30 in the order they are consumed:
//   forward: stage on register bit b = 4 - floor(log2(slot+1)); the pairs (r, r | 1<<b) that use the
//            slot are those with r >> (b+1) == slot + 1 - 2^(4-b)
//   inverse: stage on register bit b = floor(log2(slot+1));      pairs with (r & (2^b - 1)) == slot + 1 - 2^b
// Twiddle loads run TW_DEPTH slots ahead of their use through a small register ring; scheduling
// barriers keep the compiler from hoisting all 31 loads (124 VGPRs) to the top of the pass, which
// would push the kernel past the 128-VGPR budget of 4 waves per SIMD.
constexpr int TW_DEPTH = 4;     // deeper rings spill (measured)

typedef u64 __attribute__((ext_vector_type(2))) u64v2;
typedef const u64v2 __attribute__((address_space(1))) * gptr_u64x2;
typedef const u64v2 __attribute__((address_space(3))) * lptr_u64x2;
HP_DEV u64x2 gload(gptr_u64x2 p, size_t i) {   // one global_load_dwordx4
    const u64v2 v = p[i];
    return u64x2{v.x, v.y};
}

// Where a pass finds its (w, w') pairs.
//  GTab: a per-modulus table in global memory.  The table pointer comes out of a struct in memory, so the
//        compiler only knows it as a generic (flat) pointer; flat loads bump both vmcnt and lgkmcnt and force
//        full s_waitcnt 0 waits, which would serialise the prefetch ring behind L2 latency -- so it is cast to
//        the global address space and the loads become counted global_load_dwordx4.
//  LTab: a copy of the pass table staged in LDS by the workgroup (the per-1024-block tables of the middle
//        pass: 31 * 2^A pairs forward, 31 * 32 pairs inverse).  Each entry is needed by exactly one half-wave,
//        so from global memory every read would be an L1 miss; from LDS it is a broadcast ds_read_b128.
struct GTab {
    static constexpr bool scalar = false;
    static constexpr int depth = TW_DEPTH;   // slots of L2 latency to cover
    gptr_u64x2 p;
    HP_DEV explicit GTab(const u64x2 *generic) : p((gptr_u64x2)generic) {}
    HP_DEV u64x2 operator()(u32 i) const { const u64v2 v = p[i]; return u64x2{v.x, v.y}; }
    HP_DEV u64x2 at(u32 row, u32 ncls, u32 cls) const { return (*this)(row * ncls + cls); }
};
// BTab: the same table read with BUFFER loads: address = descriptor base (SGPRs) + per-launch scalar offset (SGPR, the slot) + one
//       32-bit lane offset (VGPR, computed once) -- no 64-bit address arithmetic on the vector ALU per slot (the global form
//       costs a v_add_co / v_addc pair per load: 66 instructions per thread in the last pass).
typedef u32 __attribute__((ext_vector_type(4))) v4u32;
struct BTab {
    static constexpr bool scalar = false;
    static constexpr int depth = TW_DEPTH;
    __amdgpu_buffer_rsrc_t rsrc;
    // raw buffer over the whole address range above the table (no bounds clamp wanted), gfx9-family data format word
    HP_DEV explicit BTab(const u64x2 *uniform_base)
        : rsrc(__builtin_amdgcn_make_buffer_rsrc((void *)uniform_base, 0, 0x7fffffff, 0x00020000)) {}
    // entry (row * ncls + cls) of 16-byte pairs: row * ncls is wave-uniform, cls per lane
    HP_DEV u64x2 at(u32 row, u32 ncls, u32 cls) const {
        const v4u32 v = __builtin_amdgcn_raw_buffer_load_b128(rsrc, cls << 4, (row * ncls) << 4, 0);
        return u64x2{((u64)v.y << 32) | v.x, ((u64)v.w << 32) | v.z};
    }
};
// STab: wave-uniform entries of a global table (the first pass of a transform): constant address space, so the
//       loads are scalar (s_load_dwordx4 through the scalar cache) and take no vector-memory slots.
typedef const u64v2 __attribute__((address_space(4))) * cptr_u64x2;
typedef const HpLimb __attribute__((address_space(4))) * cptr_limb;
constexpr int STAB_DEPTH = 4;   // 2 / 8 / 16 measured the same or worse
struct STab {
    static constexpr bool scalar = true;
    static constexpr int depth = STAB_DEPTH;   // held in SGPRs; SMEM returns out of order, so every use waits for all of them
    cptr_u64x2 p;
    HP_DEV explicit STab(const u64x2 *generic) : p((cptr_u64x2)generic) {}
    HP_DEV u64x2 operator()(u32 i) const { const u64v2 v = p[i]; return u64x2{v.x, v.y}; }
    HP_DEV u64x2 at(u32 row, u32 ncls, u32 cls) const { return (*this)(row * ncls + cls); }
};
struct LTab {
    static constexpr bool scalar = false;
    static constexpr int depth = 2;          // LDS latency is short
    lptr_u64x2 p;
    HP_DEV explicit LTab(const u64v2 *shared) : p((lptr_u64x2)shared) {}
    HP_DEV u64x2 operator()(u32 i) const { const u64v2 v = p[i]; return u64x2{v.x, v.y}; }
    HP_DEV u64x2 at(u32 row, u32 ncls, u32 cls) const { return (*this)(row * ncls + cls); }
};

constexpr int ilog2c(int v) { return v <= 1 ? 0 : 1 + ilog2c(v >> 1); }

// BTab / StreamBuf address with 32-bit byte offsets into descriptors without a bounds clamp: the largest offsets are
// (31 rows x 1024 classes + 1023) pairs of 16 bytes for a table and one limb (8 N bytes) for a coefficient row
static_assert((31ull * 1024 + 1024) * 16 < (1ull << 31) && (8ull << 15) < (1ull << 31), "buffer offsets must stay below 2^31");

// register index of the o-th butterfly of slot s (compile-time): forward idx = bits above b, o = bits below b;
// inverse the other way round
template <bool FWD> constexpr int slot_reg(int s, int o) {
    const int lg = ilog2c(s + 1), b = FWD ? 4 - lg : lg, idx = s + 1 - (1 << lg);
    return FWD ? ((idx << (b + 1)) | o) : ((o << (b + 1)) | idx);
}
template <bool FWD> constexpr int slot_bit(int s) { return 1 << (FWD ? 4 - ilog2c(s + 1) : ilog2c(s + 1)); }

// ---- LDS word addresses of the four register layouts ------------------------------------------
// (all already swizzled: addr(i) = i ^ ((i >> 5) & 31))
//
//   layout A ("strided"):   r = (kk << PB) | pp,  i = (kk << 10) | (tid << PB) | pp
//   layout B ("blocked"):   r = m,                i = (blk << 10) | (m << 5) | j,  blk = tid >> 5, j = tid & 31
//   layout C ("contiguous"): r,                   i = (tid << 5) | r
//   layout S ("stream"):    r = (s << 1) | e,     i = (wave << 11) | (s << 7) | (lane << 1) | e
//                           (a lane moves 16 contiguous bytes, a wave 1 KiB per HBM instruction)
// N = 32768 uses a PADDED buffer instead (word address i + (i >> 5), 132 KiB): every register's offset is then an immediate of the
// ds instruction and the 279 v_xor per thread disappear; it is conflict-free for all four layouts at that size only (at N <= 16384
// the strided layout A collides, and the padding would cost the second workgroup per CU its LDS).
// (forward kernels only: the inverse kernel with the padded buffer spills 34 registers and runs 4 % slower)
template <int LOGN, bool PADDED = false> struct Addr {
    using G = Geo<LOGN>;
    static constexpr int LOGN_ = LOGN;
    static constexpr bool PAD = PADDED;
    static constexpr int WORDS = PAD ? G::N + G::N / 32 : G::N;
    u32 a_base;   // ((tid << PB) ^ h) with h = bits 9..5 of (tid << PB)
    u32 b_base;   // (blk << 10) | j
    u32 c_base;   // (tid << 5) | (tid & 31)
    u32 s_base;   // (wave << 11) | ((lane >> 4) << 5) | (((lane & 15) << 1) ^ (lane >> 4))
    HP_DEV void init(u32 tid) {
        const u32 lane = tid & 63u, wave = tid >> 6;
        if (PAD) {   // byte offsets of i + (i >> 5) with the register-dependent part left to lay_addr()
            a_base = ((tid << G::PB) + ((tid << G::PB) >> 5)) << 2;   // (the passenger bits pp < 2^PB <= 32 do not reach bit 5)
            b_base = ((tid >> 5) * 1056u + (tid & 31u)) << 2;
            c_base = (tid * 33u) << 2;
            s_base = (wave * 2112u + 2u * lane + (lane >> 4)) << 2;
            return;
        }
        // all four are BYTE offsets into the exchange buffer (word index * 4): an access then costs one v_xor, the
        // additive part of lay_addr() folds into the ds instruction's immediate offset
        const u32 t = tid << G::PB;
        a_base = (t ^ ((t >> 5) & 31u)) << 2;
        b_base = (((tid >> 5) << 10) | (tid & 31u)) << 2;
        c_base = ((tid << 5) | (tid & 31u)) << 2;
        s_base = ((wave << 11) | ((lane >> 4) << 5) | (((lane & 15u) << 1) ^ (lane >> 4))) << 2;
    }
};

enum { LAY_A = 0, LAY_B = 1, LAY_C = 2, LAY_S = 3 };

// Launder a thread-constant through an empty asm so the compiler treats it as a fresh value:
// the 32 LDS addresses derived from it are then recomputed (one v_xor each) in every round of
// an exchange instead of being kept live in 32 VGPRs across rounds.
HP_DEV u32 opaque(u32 v) {
    asm volatile("" : "+v"(v));
    return v;
}

template <int LAY, class AD> HP_DEV u32 lay_base(const AD &ad) {
    if (LAY == LAY_A) return ad.a_base;
    if (LAY == LAY_B) return ad.b_base;
    if (LAY == LAY_C) return ad.c_base;
    return ad.s_base;
}

template <int LOGN, int LAY, bool PAD> HP_DEV u32 lay_addr(u32 base, int r) {
    using G = Geo<LOGN>;
    if (PAD) {
        if (LAY == LAY_A) return base + ((u32)(r >> G::PB) * 1056u + (u32)(r & ((1 << G::PB) - 1))) * 4u;   // i = (kk << 10) | (tid << PB) | pp
        if (LAY == LAY_B) return base + (u32)r * (33u * 4u);                         // i = (blk << 10) | (r << 5) | j
        if (LAY == LAY_C) return base + (u32)r * 4u;                                 // i = (tid << 5) | r
        return base + ((u32)(r >> 1) * 132u + (u32)(r & 1)) * 4u;                    // i = (wave << 11) | (s << 7) | (lane << 1) | e
    }
    if (LAY == LAY_A) return (base ^ ((u32)(r & ((1 << G::PB) - 1)) << 2)) + ((u32)((r >> G::PB) << 10) << 2);
    if (LAY == LAY_B) return (base ^ ((u32)r << 2)) + ((u32)(r << 5) << 2);
    if (LAY == LAY_C) return base ^ ((u32)r << 2);
    return (base ^ ((u32)((r & 1) | (((r >> 1) & 7) << 2)) << 2)) + ((u32)((r >> 1) << 7) << 2);
}

// Between the write and the read phase of an exchange round.  Workgroup-wide: s_barrier.  Wave-local: the hardware
// executes one wave's LDS instructions in order, so no wait is needed -- but the COMPILER must not move a thread's reads
// above its own writes (different addresses for the thread, the same words for its wave): memory clobber + scheduling
// barrier.  Measured cost: none.
template <bool WG> HP_DEV void exch_fence() {
    if (WG) {
        __syncthreads();
    } else {
        asm volatile("" ::: "memory");
        __builtin_amdgcn_sched_barrier(0);
    }
}

// word of the exchange buffer at a byte offset
HP_DEV u32 &lds_w(u32 *lds, u32 byte_off) { return *reinterpret_cast<u32 *>(reinterpret_cast<char *>(lds) + byte_off); }

// Transpose the workgroup's coefficients from register layout FROM to layout TO through LDS, one
// 32-bit half at a time.  WG: the exchange crosses waves (needs s_barrier); otherwise it is
// confined to the wave's own 2048-word region and relies on in-order LDS execution per wave.
template <int LOGN, int FROM, int TO, bool WG, class AD>
HP_DEV void exchange(u64 (&x)[32], u32 *lds, const AD &ad) {
    static_assert(AD::LOGN_ == LOGN, "address set of another ring degree");
    constexpr bool PAD = AD::PAD;
    u32 keep[32];
    {
        const u32 fb = opaque(lay_base<FROM>(ad));
#pragma unroll
        for (int r = 0; r < 32; ++r) {
            lds_w(lds, lay_addr<LOGN, FROM, PAD>(fb, r)) = lo32(x[r]);
            keep[r] = hi32(x[r]);
        }
    }
    exch_fence<WG>();
    u32 nlo[32];
    {
        const u32 tb = opaque(lay_base<TO>(ad));
#pragma unroll
        for (int r = 0; r < 32; ++r) nlo[r] = lds_w(lds, lay_addr<LOGN, TO, PAD>(tb, r));
    }
    exch_fence<WG>();
    {
        const u32 fb = opaque(lay_base<FROM>(ad));
#pragma unroll
        for (int r = 0; r < 32; ++r) lds_w(lds, lay_addr<LOGN, FROM, PAD>(fb, r)) = keep[r];
    }
    exch_fence<WG>();
    {
        const u32 tb = opaque(lay_base<TO>(ad));
#pragma unroll
        for (int r = 0; r < 32; ++r) x[r] = mk64(nlo[r], lds_w(lds, lay_addr<LOGN, TO, PAD>(tb, r)));
    }
}

constexpr int HP_EPI_DEPTH = 4;   // rows of the fused drop epilogue whose operand loads are in flight

struct alignas(16) V2 {
    u64 x, y;
};

// Streaming accesses to coefficient data are marked non-temporal so that the once-read, once-written
// limbs do not push the twiddle tables (re-read by every workgroup) out of L2: +3.5..5 % on every
// transform shape (HP_TEMPORAL_DATA restores plain accesses for A/B runs).
HP_DEV V2 ld_stream(const u64 *p) {
    typedef u64 __attribute__((ext_vector_type(2))) vv;
    const vv v = __builtin_nontemporal_load(reinterpret_cast<const vv *>(p));
    return V2{v.x, v.y};
}
HP_DEV void st_stream(u64 *p, const V2 &v) {
    typedef u64 __attribute__((ext_vector_type(2))) vv;
    __builtin_nontemporal_store(vv{v.x, v.y}, reinterpret_cast<vv *>(p));
}

// A coefficient row as a buffer: 16 bytes per lane at (lane byte offset, wave-uniform byte offset), non-temporal like ld_stream / st_stream
struct StreamBuf {
    __amdgpu_buffer_rsrc_t rsrc;
    // the row address is the same for the whole workgroup; say so (readfirstlane), or the compiler keeps the descriptor in VGPRs
    // and wraps every access in a loop over its distinct values
    HP_DEV static u64 *uniform(const u64 *row) {
        const u64 a = reinterpret_cast<u64>(row);
        const u32 lo = (u32)__builtin_amdgcn_readfirstlane((u32)a), hi = (u32)__builtin_amdgcn_readfirstlane((u32)(a >> 32));   // (the builtin returns int)
        return reinterpret_cast<u64 *>(((u64)hi << 32) | lo);
    }
    HP_DEV explicit StreamBuf(const u64 *row) : rsrc(__builtin_amdgcn_make_buffer_rsrc(uniform(row), 0, 0x7fffffff, 0x00020000)) {}
    HP_DEV V2 load(u32 voff, u32 soff) const {
        const v4u32 v = __builtin_amdgcn_raw_buffer_load_b128(rsrc, voff, soff, 2);
        return V2{((u64)v.y << 32) | v.x, ((u64)v.w << 32) | v.z};
    }
    // Stores take the row offset in the LANE offset and no scalar offset.  With an SGPR soffset the assembler assumes that a
    // 16-byte buffer store has read its data by the time the next instruction issues and pads nothing; on gfx950 it has not: a
    // VALU instruction right behind the store that overwrites a data register changed what the last lanes of each 16-lane pass
    // stored (found as rare wrong words in lanes 12-15, 28-31, ... of one row).  Without soffset the hazard is known and padded.
    HP_DEV void store(u32 voff, const V2 &v) const {
        __builtin_amdgcn_raw_buffer_store_b128(v4u32{(u32)v.x, (u32)(v.x >> 32), (u32)v.y, (u32)(v.y >> 32)}, rsrc, voff, 0, 2);
    }
};

// value held by the neighbouring lane (lane ^ 1): DPP quad_perm [1,0,3,2], no LDS involved
HP_DEV u64 from_pair_lane(u64 v) {
    const u32 lo = (u32)__builtin_amdgcn_update_dpp(0, (int)(u32)v, 0xB1, 0xF, 0xF, true);
    const u32 hi = (u32)__builtin_amdgcn_update_dpp(0, (int)(u32)(v >> 32), 0xB1, 0xF, 0xF, true);
    return ((u64)hi << 32) | lo;
}

// load-side work deferred into the first stage of a forward pass (see pass_slots): the lane-pair swap of N = 32768
HP_DEV void lazy_swap(u64 (&x)[32], int r) {
    const bool odd = (threadIdx.x & 1u) != 0;
    const u64 vx = x[r], vy = x[r + 1];
    const u64 keep = odd ? vy : vx, send = odd ? vx : vy;
    const u64 recv = from_pair_lane(send);
    x[r] = odd ? recv : keep;
    x[r + 1] = odd ? keep : recv;
}
struct NoPre {
    static constexpr bool on = false;
    HP_DEV void operator()(u64 (&)[32], int) const {}
};
struct SwapPre {
    static constexpr bool on = true;
    HP_DEV void operator()(u64 (&x)[32], int r) const { lazy_swap(x, r); }
};

// ---- the slot schedule of a pass, over a butterfly policy --------------------------------------
// One slot (or, in the last stage of a pass where every butterfly has its own twiddle, two slots) of a pass;
// recursion over the slot number keeps every register index a compile-time constant.
// Bf: the arithmetic, `template <bool SCALAR_TAB> void pair(a0, a1, b0, b1, twA, twB) const` = two butterflies (a0, a1) with
// twiddle pair twA and (b0, b1) with twB; it lives in the .hip file that owns the arithmetic (HarveyBf, F64Bf).
// Pre (first pass of a forward kernel): work that belongs to the LOADS is done here, per register pair (r, r + 1) = one 16-byte
// load, right before the first butterfly that touches it -- so the first stage runs while the later loads are still in flight
// instead of after all sixteen (SwapPre above; DropPre, ConvPre, DropPreA, DropPre2A in the .hip files).
// The scheduling barriers are placed by measurement: one misplaced barrier costs spills (128-VGPR budget).
template <bool FWD, int S, int S0, int S1, int D, class Tab, class Bf, class Pre = NoPre>
HP_DEV void pass_slots(u64 (&x)[32], u64x2 (&ring)[D], const Tab &tbl, u32 ncls, u32 cls, const Bf &bf, const Pre &pre = Pre()) {
    if constexpr (S < S1) {
        constexpr int cnt = 1 << (4 - ilog2c(S + 1));   // butterflies that use this slot's twiddle
        constexpr int bit = slot_bit<FWD>(S);
        const u64x2 tw = ring[(S - S0) % D];
        if constexpr (S + D < S1) ring[(S - S0) % D] = tbl.at((u32)(S + D), ncls, cls);
        if constexpr (cnt >= 2) {
#pragma unroll
            for (int o = 0; o < cnt; o += 2) {
                const int ra = slot_reg<FWD>(S, o), rb = slot_reg<FWD>(S, o + 1);
                if constexpr (Pre::on && S == 0) {
                    static_assert(!Pre::on || (FWD && S0 == 0), "load-side work: first slot of a forward pass");
                    pre(x, ra);          // rb == ra + 1: one 16-byte load
                    pre(x, ra | bit);
                }
                bf.template pair<Tab::scalar>(x[ra], x[ra | bit], x[rb], x[rb | bit], tw, tw);
                if (o & 2) __builtin_amdgcn_sched_barrier(0);
            }
            if constexpr (cnt == 2) { if constexpr (S & 1) __builtin_amdgcn_sched_barrier(0); }
            pass_slots<FWD, S + 1, S0, S1, D, Tab, Bf, Pre>(x, ring, tbl, ncls, cls, bf, pre);
        } else {
            static_assert(S + 1 < S1, "single-butterfly slots come in pairs");
            const u64x2 tw2 = ring[(S + 1 - S0) % D];
            if constexpr (S + 1 + D < S1) ring[(S + 1 - S0) % D] = tbl.at((u32)(S + 1 + D), ncls, cls);
            constexpr int ra = slot_reg<FWD>(S, 0), rb = slot_reg<FWD>(S + 1, 0);
            bf.template pair<Tab::scalar>(x[ra], x[ra | bit], x[rb], x[rb | bit], tw, tw2);
            if constexpr (((S - 15) & 2) != 0) __builtin_amdgcn_sched_barrier(0);
            pass_slots<FWD, S + 2, S0, S1, D, Tab, Bf>(x, ring, tbl, ncls, cls, bf);
        }
    }
}

template <bool FWD, int S0, int S1, int D, class Tab, class Bf, class Pre = NoPre>
HP_DEV void run_pass(u64 (&x)[32], const Tab tbl, u32 ncls, u32 cls, const Bf &bf, const Pre &pre = Pre()) {
    u64x2 ring[D];
#pragma unroll
    for (int s = S0; s < S0 + D; ++s)
        if (s < S1) ring[(s - S0) % D] = tbl.at((u32)s, ncls, cls);
    pass_slots<FWD, S0, S0, S1, D, Tab, Bf, Pre>(x, ring, tbl, ncls, cls, bf, pre);
}

// forward: stages on register bits BHI..BLO (descending)
template <int BHI, int BLO, class Tab, class Bf, class Pre = NoPre>
HP_DEV void fwd_pass(u64 (&x)[32], const Tab tbl, u32 ncls, u32 cls, const Bf &bf, const Pre &pre = Pre()) {
    static_assert(BHI == 4, "forward passes start at register bit 4");
    run_pass<true, 0, (1 << (5 - BLO)) - 1, Tab::depth, Tab, Bf, Pre>(x, tbl, ncls, cls, bf, pre);
}

// inverse: stages on register bits BLO..BHI (ascending); D: depth of the twiddle ring
template <int BLO, int BHI, class Tab, int D = Tab::depth, class Bf>
HP_DEV void inv_pass(u64 (&x)[32], const Tab tbl, u32 ncls, u32 cls, const Bf &bf) {
    static_assert(BHI == 4, "inverse passes end at register bit 4");
    run_pass<false, (1 << BLO) - 1, 31, D, Tab, Bf>(x, tbl, ncls, cls, bf);
}

// ---- forward kernel ----------------------------------------------------------------------------
#define HP_LOAD_ORDER(t) (((t) >> 1) | (((t) & 1) << 3))
// load, layout A: thread reads 2^PB consecutive coefficients at 2^A places 1024 apart
template <int LOGN, bool LZ = false>
HP_DEV void load_flight(const u64 *src, u32 tid, u64 (&x)[32]) {
    using G = Geo<LOGN>;
    if constexpr (G::PB == 0) {
        // N = 32768: a thread owns one column (tid) of 32 rows 1024 apart.  Two neighbouring lanes
        // fetch 16 bytes (both their columns) of alternate rows and trade halves with one DPP swap,
        // so every HBM instruction still moves 16 bytes per lane.
        const bool odd = (tid & 1u) != 0;
        const u64 *sp = src + (tid & ~1u);
        // issue order 0, 8, 1, 9, ...: the first stage pairs register r with r + 16, i.e. load p with load p + 8, so its
        // butterflies can start as soon as the first two loads are back instead of after nine
#pragma unroll
        for (int t = 0; t < 16; ++t) {
            const int p = HP_LOAD_ORDER(t);
            const V2 v = ld_stream(sp + ((size_t)(2 * p + (odd ? 1 : 0)) << 10));
            if (LZ) { x[2 * p] = v.x; x[2 * p + 1] = v.y; continue; }   // sorted by lazy_swap in the first pass
            const u64 keep = odd ? v.y : v.x, send = odd ? v.x : v.y;
            const u64 recv = from_pair_lane(send);
            x[2 * p] = odd ? recv : keep;
            x[2 * p + 1] = odd ? keep : recv;
        }
    } else {
        const u64 *s = src + ((size_t)tid << G::PB);
#pragma unroll
        for (int tk = 0; tk < (1 << G::A); ++tk) {
            // same idea as above: the first stage pairs place kk with kk + 2^(A-1)
            const int kk = (tk >> 1) | ((tk & 1) << (G::A - 1));
#pragma unroll
            for (int pp = 0; pp < (1 << G::PB); pp += 2) {
                const V2 v = ld_stream(s + ((size_t)kk << 10) + pp);
                x[(kk << G::PB) | pp] = v.x;
                x[(kk << G::PB) | pp | 1] = v.y;
            }
        }
    }
}

// stage the forward middle pass's twiddles in LDS (31 * 2^A pairs, one per thread): the load is issued first, the LDS write after
// the coefficient loads are in flight; it becomes visible through the barriers of the A->B exchange
// (lp: the limb's constants, HpLimb or HpLimbA; the table pointer is read from it by the threads that stage, not before the branch)
template <int LOGN, class LP> HP_DEV u64v2 fwd_stage_issue(LP lp, u32 tid) {
    u64v2 stg = {0, 0};
    if (tid < 31u * (1u << Geo<LOGN>::A)) stg = ((gptr_u64x2)lp->fwd_k)[tid];
    return stg;
}
template <int LOGN> HP_DEV void fwd_stage_write(u64v2 *lds_tw, u32 tid, const u64v2 &stg) {
    if (tid < 31u * (1u << Geo<LOGN>::A)) lds_tw[tid] = stg;
}

// word offset of a thread's 16 bytes in row 0 of layout S (row s is (s << 7) words further)
HP_DEV size_t stream_off(u32 tid) { return (((size_t)(tid >> 6)) << 11) + ((tid & 63u) << 1); }

// store, layout S: 16 bytes per lane, a wave writes 1 KiB of consecutive words per instruction
HP_DEV void store_stream(u64 *dst, size_t off, const u64 (&x)[32]) {
    u64 *d = dst + off;
#pragma unroll
    for (int s = 0; s < 16; ++s) {
        V2 v{x[2 * s], x[2 * s + 1]};
        st_stream(d + ((size_t)s << 7), v);
    }
}
// HP_PACK48 (hp_device.h): low words as 8 bytes per lane, high 16 bits of the two words as 4 bytes per lane
template <int LOGN> HP_DEV void store_stream_pack48(u64 *dst, size_t off, const u64 (&x)[32]) {
    typedef u32 __attribute__((ext_vector_type(2))) v2u;
    u32 *lo = reinterpret_cast<u32 *>(dst) + off;
    u32 *hi = reinterpret_cast<u32 *>(dst) + Geo<LOGN>::N + (off >> 1);
#pragma unroll
    for (int s = 0; s < 16; ++s) {
        __builtin_nontemporal_store(v2u{lo32(x[2 * s]), lo32(x[2 * s + 1])}, reinterpret_cast<v2u *>(lo + ((size_t)s << 7)));
        __builtin_nontemporal_store((hi32(x[2 * s]) & 0xffffu) | (hi32(x[2 * s + 1]) << 16), hi + ((size_t)s << 6));
    }
}
// HP_PACK40 (hp_device.h): low words as 8 bytes per lane, bits 32..39 of the two words as 2 bytes per lane
template <int LOGN> HP_DEV void store_stream_pack40(u64 *dst, size_t off, const u64 (&x)[32]) {
    typedef u32 __attribute__((ext_vector_type(2))) v2u;
    u32 *lo = reinterpret_cast<u32 *>(dst) + off;
    unsigned short *hi = reinterpret_cast<unsigned short *>(reinterpret_cast<char *>(dst) + 4 * (size_t)Geo<LOGN>::N + off);
#pragma unroll
    for (int s = 0; s < 16; ++s) {
        __builtin_nontemporal_store(v2u{lo32(x[2 * s]), lo32(x[2 * s + 1])}, reinterpret_cast<v2u *>(lo + ((size_t)s << 7)));
        __builtin_nontemporal_store((unsigned short)((hi32(x[2 * s]) & 0xffu) | ((hi32(x[2 * s + 1]) & 0xffu) << 8)), hi + ((size_t)s << 6));
    }
}

// ---- fused drop epilogue: rows x, addend and out of the thread's item, and the pipeline over their 16 rows ------------------
// The three streams through buffer descriptors: one lane offset for all of them, the row step (s << 7 words) in an SGPR for the
// loads, in the instruction's immediate / one 32-bit add for the stores -- no 64-bit address arithmetic on the vector ALU.
// has_add is wave-uniform; said explicitly (readfirstlane) so that the run-time flavours branch on an SGPR instead of masking lanes:
// flavour 0 asks add_mask, flavour 5 (rotations / conjugations, ckks/arith.cpp:75-93) adds the moved c0 to polynomial 0 only,
// flavours 2 / 4 / 6 / 7 always add.
template <int LOGN, int FLAV> struct DropRows {
    using G = Geo<LOGN>;
    u32 voff;
    bool has_add;
    StreamBuf xs, as, d;
    HP_DEV DropRows(const HpDropArgs *da, u32 k, u32 p2, u32 tid)
        : voff(((((tid >> 6)) << 11) + ((tid & 63u) << 1)) << 3),
          has_add(FLAV == 2 || FLAV == 4 || FLAV == 6 || FLAV == 7 || (FLAV == 5 && __builtin_amdgcn_readfirstlane((p2 & 1u) == 0 ? 1 : 0) != 0) ||
                  (FLAV == 0 && __builtin_amdgcn_readfirstlane((da->addend && ((da->add_mask >> (p2 & 1)) & 1u)) ? 1 : 0) != 0)),
          xs(da->x + ((size_t)p2 * da->L + k) * G::N),
          as(has_add ? da->addend + ((size_t)(p2 >> 1) * da->add_ct_stride + (size_t)(p2 & 1) * da->add_poly_stride + k) * G::N : da->x),
          d(da->out + ((size_t)p2 * da->out_stride + k) * G::N) {}

    // The 16 rows are software-pipelined by hand: the operand loads run HP_EPI_DEPTH rows ahead of their use (ring in
    // registers, the twiddle ring is dead by now), otherwise every row waits for its own two loads with
    // vmcnt(0) -- which also drains the stores of the previous row -- and the epilogue costs 32 exposed round trips.
    // row(add_tag, x_row, add_row, s) -> the result of row s (registers 2 s, 2 s + 1 of the transform); words(result) -> the words
    // stored (level A: the canonical residues of its doubles), evaluated after the store's offset as both files always had it
    template <bool ADD, class Row, class Words> HP_DEV void pipeline(const Row &row, const Words &words) const {
        constexpr int EPI_DEPTH = HP_EPI_DEPTH;
        V2 xr[EPI_DEPTH], ar[EPI_DEPTH];
#pragma unroll
        for (int s = 0; s < EPI_DEPTH; ++s) {
            xr[s] = xs.load(voff, (u32)s << 10);
            if (ADD) ar[s] = as.load(voff, (u32)s << 10);
        }
#pragma unroll
        for (int s = 0; s < 16; ++s) {
            const V2 xv = xr[s % EPI_DEPTH];
            V2 av{0, 0};
            if (ADD) av = ar[s % EPI_DEPTH];
            __builtin_amdgcn_sched_barrier(0);
            if (s + EPI_DEPTH < 16) {
                xr[s % EPI_DEPTH] = xs.load(voff, (u32)(s + EPI_DEPTH) << 10);
                if (ADD) ar[s % EPI_DEPTH] = as.load(voff, (u32)(s + EPI_DEPTH) << 10);
            }
            __builtin_amdgcn_sched_barrier(0);
            const V2 out = row(std::bool_constant<ADD>{}, xv, av, s);
            d.store(voff + ((u32)s << 10), words(out));
        }
    }
    // one copy of the row loop per value of has_add where it is only known at run time (flavours 0 and 5): the loop body
    // then has no branch on it
    template <class Row, class Words> HP_DEV void run(const Row &row, const Words &words) const {
        if constexpr (FLAV == 2 || FLAV == 4 || FLAV == 6 || FLAV == 7) pipeline<true>(row, words);
        else if constexpr (FLAV == 1 || FLAV == 3) pipeline<false>(row, words);
        else if (has_add) pipeline<true>(row, words);
        else pipeline<false>(row, words);
    }
};

// ---- inverse kernels -------------------------------------------------------------------------------
// The middle pass of the inverse stages 31 x 32 twiddle pairs (15.5 KiB) in LDS whatever N is.  With one limb per workgroup
// that stage caps the occupancy of the small sizes (N = 4096: 16 + 15.5 KiB per two waves -> 5 workgroups = 2.5 waves per
// SIMD, VALUBusy 42 %).  So for N <= 8192 a workgroup transforms LPW limbs OF ONE MODULUS side by side and shares the stage:
// 512 threads, 4 N LPW + 15.5 KiB = 80 KiB of LDS, two workgroups = four waves per SIMD on a CU.
template <int LOGN> struct InvGeo {
    static constexpr int LPW = LOGN >= 14 ? 1 : (512 >> (LOGN - 5));   // limbs per workgroup: 2^11 -> 8, 2^12 -> 4, 2^13 -> 2
    static constexpr int TT = Geo<LOGN>::T * LPW;                      // threads per workgroup
    static constexpr bool STREAM_EPILOGUE = LOGN <= 13;                // see the end of k_ntt_inv
    static constexpr int NSTG = (31 * 32 + TT - 1) / TT;               // staged twiddle pairs per thread
    static u32 grid(const HpNttJob &job) { return hp_inv_grid(job, LPW); }
};

// the item of sub-limb `sub` of a workgroup; false: a group past the last polynomial, which re-reads the last one and stores nothing
// (the numbering itself: hp_inv_item, hp_ntt_job.h)
template <int LOGN> HP_DEV bool inv_item(const HpNttJob &job, u32 sub, HpItem &it) {
    return hp_inv_item(job, blockIdx.x, sub, InvGeo<LOGN>::LPW, Geo<LOGN>::N, it);
}

// ---- launch dispatch -------------------------------------------------------------------------------
// f(std::integral_constant<int, LOGN>) for the ring degrees the tiled kernels are built for
template <class F> hipError_t for_logn(const HpNttJob &job, F f) {
    switch (job.logn) {
    case 11: return f(std::integral_constant<int, 11>{});
    case 12: return f(std::integral_constant<int, 12>{});
    case 13: return f(std::integral_constant<int, 13>{});
    case 14: return f(std::integral_constant<int, 14>{});
    case 15: return f(std::integral_constant<int, 15>{});
    default: return hipErrorNotSupported;
    }
}
// f(std::integral_constant<int, I>) for the I of LO .. HI that equals i; false: none does
template <int LO, int HI, class F> bool for_index(int i, F f) {
    if constexpr (LO <= HI) {
        if (i == LO) { f(std::integral_constant<int, LO>{}); return true; }
        return for_index<LO + 1, HI>(i, f);
    }
    return false;
}

// Phase tracing for kernel tuning (variant builds only, -DHP_TRACE): shader-clock stamps of wave 0
// of every 16th workgroup at the phase boundaries.  Each .hip file says HP_TRACE_STORAGE(reader) once, at file scope before its
// kernels: its own g_trace and the exported reader (hp_debug_trace, hp_debug_trace_a).
#ifdef HP_TRACE
#ifdef HP_TRACE_ALL
#define HP_TRACE_SEL (blockIdx.x < 2048 * 16)
#define HP_TRACE_IDX (blockIdx.x)
#else
#define HP_TRACE_SEL ((blockIdx.x & 15) == 0 && (blockIdx.x >> 4) < 2048)
#define HP_TRACE_IDX (blockIdx.x >> 4)
#endif
#define HP_TRACE_SLOTS 12
#define HP_TRACE_STORAGE(reader) \
    namespace { __device__ u64 g_trace[2 * 2048 * 16 * HP_TRACE_SLOTS]; } \
    extern "C" int reader(u64 *out, size_t words) { return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(g_trace), words * sizeof(u64)); }
#define TRACE_DECL u64 tr__[HP_TRACE_SLOTS]; int tri__ = 0; tr__[10] = ((u64)__builtin_amdgcn_s_getreg(63492) << 32) | (u32)__builtin_amdgcn_s_getreg((31 << 11) | 20); tr__[11] = t_entry__;
#define TRACE_ENTRY __builtin_amdgcn_sched_barrier(0); const u64 t_entry__ = __builtin_amdgcn_s_memtime(); __builtin_amdgcn_sched_barrier(0);
#define TRACE_MARK() do { __builtin_amdgcn_sched_barrier(0); tr__[tri__++] = __builtin_amdgcn_s_memtime(); __builtin_amdgcn_sched_barrier(0); } while (0)
#ifdef HP_TRACE_WAVES   // every wave of every 16th workgroup: record (blockIdx >> 4) * 16 + wave
#define TRACE_FLUSH() do { if ((threadIdx.x & 63u) == 0 && HP_TRACE_SEL && (threadIdx.x >> 6) < 16) { \
        for (int i__ = 0; i__ < HP_TRACE_SLOTS; i__++) g_trace[(HP_TRACE_IDX * 16 + (threadIdx.x >> 6)) * HP_TRACE_SLOTS + i__] = (i__ < tri__ || i__ >= 10) ? tr__[i__] : 0; } } while (0)
#else
#define TRACE_FLUSH() do { if ((threadIdx.x == 0 || threadIdx.x == blockDim.x - 64) && HP_TRACE_SEL) { \
        for (int i__ = 0; i__ < HP_TRACE_SLOTS; i__++) g_trace[(HP_TRACE_IDX * 2 + (threadIdx.x != 0)) * HP_TRACE_SLOTS + i__] = (i__ < tri__ || i__ >= 10) ? tr__[i__] : 0; } } while (0)
#endif
#else
#define HP_TRACE_STORAGE(reader)
#define TRACE_DECL
#define TRACE_ENTRY
#define TRACE_MARK() do { } while (0)
#define TRACE_FLUSH() do { } while (0)
#endif

} // namespace
