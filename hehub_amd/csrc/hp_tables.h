// hp_tables.h -- host-side construction of per-modulus constants and twiddle
// tables for the HIP kernels.  Values follow hehub's NTTFactors
// (src/fhe/common/ntt.cpp:41-105) and mod_arith.cpp:49-62; the *layouts* are
// the engine's own (reference order for the simple kernels, kernel order for
// the register/LDS-tiled ones).
#pragma once
#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

namespace hp {

typedef uint64_t u64;
typedef unsigned __int128 u128;

struct Pair {
    u64 w, wh;
};

struct ModConsts {
    u64 q, two_q, neg_q, mqinv, r64, r64h, barrett_c;
    uint32_t k, fix;
};

// scalar helpers (host)
u64 harvey_quotient(u64 b, u64 q);                 // floor(b * 2^64 / q)
u64 mul_mod(u64 a, u64 b, u64 q);
u64 pow_mod(u64 q, u64 base, u64 e);
u64 inverse_mod_prime(u64 elem, u64 prime);        // mod_arith.cpp:136-149
u64 minus_q_inv_mod_2to64(u64 q);
u64 two_to_64_mod(u64 q);
unsigned bit_rev(unsigned x, int bits);
int log_modulus(u64 q);                             // (u64)(log2(q) + 0.5)

ModConsts make_consts(u64 q);

// The fold that ends hehub's lazy transforms (ntt.cpp:171-175 forward, :215-219 inverse): x -= ((x >> kb) - fix) q with
// kb = round(log2 q), fix = (q >= 2^kb).  Each of the logn butterfly stages raises the largest word by less than 2q (a stage writes
// x_l + t and x_l + 2q - t with t = mul_mod_harvey_lazy(..) in [0, 2q) whatever the u64 operand), so for input words below x_in
// the fold sees x < x_in + 2q logn, m = x >> kb <= m_max.  With delta = |q - 2^kb| the folded word is (x mod 2^kb) + m delta for
// fix = 0 -- never below zero -- and (x mod 2^kb) + q - m delta for fix = 1, which goes below zero (hehub's word is then the
// wrapped u64, not congruent to x modulo q) once m delta exceeds q: no wrap is guaranteed where m_max delta < 2^kb.
struct FoldBound {
    bool wraps;      // some input below x_in may give a word that is not x modulo q (a wrapped fold, or a stage sum past 2^64)
    u128 m_delta;    // m_max delta: below 2^kb, the fold neither wraps (fix = 1) nor leaves a word at or above 2^(kb+1) (fix = 0)
    u128 word_end;   // where it does not wrap: every folded word is below this (the forward transform's output word)
};
FoldBound lazy_fold_bound(const ModConsts &c, u128 x_in, size_t logn);
// Parity level A serves q (hp_ctx.cpp ensure_plan_a): its FP64 kernels compute true residues, so hehub's fold must not wrap for any
// input a pipeline of the chain hands the transform -- a caller's lazy word (< 2q) or a strict row of another modulus (< cmax, the
// key switch's digit rows: their words may exceed 2q, they stay inside the pipeline).  And level A takes lazy words only (< 2q, the
// range guard), so hehub's forward words of a caller's lazy row -- words hehub hands back to the caller -- must stay below 2q.
bool level_a_modulus(const ModConsts &c, u64 cmax, size_t logn);

// Returns "" on success, otherwise the message hehub throws for the same input
// ("2N doesn't divide (modulus - 1)" / "NTT not supporting primes with bit size > 59 currently.").
std::string check_ntt_modulus(u64 q, size_t logn);
u64 unity_root_2n(u64 q, size_t logn);              // ntt.cpp:26-39

// Reference-order tables.
//   fwd_ref[i]            = psi^bitrev(i, logn)                       i in [0, N)
//   inv_ref[2^l - 1 + i]  = psi^-(bitrev(i, l) * 2^(logn - l))         l in [0, logn)
//   inv_ref[N + i]        = strict(psi^-i * N^-1)                      i in [0, N)
void build_fwd_ref(u64 q, size_t logn, std::vector<Pair> &out);   // N entries
void build_inv_ref(u64 q, size_t logn, std::vector<Pair> &out);   // 2N entries

// Kernel-order tables for the fast (register + LDS exchange) transforms,
// logn in [11, 15]; layouts documented in hp_ntt_fast.hip.
void build_fwd_fast(const std::vector<Pair> &fwd_ref, size_t logn, std::vector<Pair> &out);
void build_inv_fast(const std::vector<Pair> &inv_ref, size_t logn, std::vector<Pair> &out);

// Parity level A (hp_ntt_a.hip): any of the tables above with every pair (w, w') replaced by the bit patterns of the IEEE doubles
// (w, RN(w / q)); same layout.  q < 2^50 (every w < q is a double exactly).
void pairs_to_f64(const std::vector<Pair> &in, u64 q, std::vector<Pair> &out);
u64 f64_bits(double v);

} // namespace hp
