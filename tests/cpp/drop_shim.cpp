// drop_shim.cpp -- C entry points around hehub_amd/csrc/hp_drop.cpp so the CPU test-suite can check every constant of the fused
// drop launches without a GPU.  Test infrastructure only.
#include "../../hehub_amd/csrc/hp_drop.h"
#include "../../hehub_amd/csrc/hp_tables.h"

#include <cstring>
#include <vector>

using namespace hpi;

namespace {

std::vector<hp::ModConsts> chain_of(const uint64_t *moduli, size_t count) {
    std::vector<hp::ModConsts> c;
    for (size_t i = 0; i < count; i++) c.push_back(hp::make_consts(moduli[i]));
    return c;
}

HpDropArgs blank() { return drop_args(nullptr, 0, Addend(), nullptr, 0); }

// HpDropArgs as DS_WORDS u64: 18 scalars, then the 12 per-limb arrays (tests/test_host_drop_consts.py names them in this order)
void dump(const HpDropArgs &da, uint64_t *out) {
    const uint64_t head[18] = {da.dc.q_last, da.dc.half_q_last, (uint64_t)da.dc.bgv, (uint64_t)da.small_rem, (uint64_t)da.raw_input, da.out_stride,
                               (uint64_t)da.fin_on, da.comb_half, da.q2_last, da.half_q2_last, da.L, da.add_poly_stride, da.add_ct_stride,
                               da.add_mask, (uint64_t)(uintptr_t)da.x, (uint64_t)(uintptr_t)da.addend, (uint64_t)(uintptr_t)da.out,
                               (uint64_t)(uintptr_t)da.comb};
    std::memcpy(out, head, sizeof(head));
    const uint64_t *rows[12] = {da.dc.r, da.dc.inv, da.dc.inv_h, da.dc.t, da.dc.t_h, da.dc.qlt, da.dc.qlt_h, da.fin, da.fin_h, da.comb_r,
                                da.comb_mul, da.comb_mul_h};
    for (int i = 0; i < 12; i++) std::memcpy(out + 18 + i * HP_MAX_LIMBS, rows[i], HP_MAX_LIMBS * sizeof(uint64_t));
}

} // namespace

extern "C" {

int ds_max_limbs() { return HP_MAX_LIMBS; }

void ds_a_pair(uint64_t v, uint64_t q, uint64_t *out2) { a_pair(v, q, out2[0], out2[1]); }

void ds_drop_args(uint64_t x, size_t L, uint64_t add, size_t ps, size_t cs, unsigned mask, size_t shift, uint64_t o, size_t out_stride, uint64_t *out) {
    const Addend a = Addend((const u64 *)(uintptr_t)add, ps, cs, mask).from(shift);
    dump(drop_args((const u64 *)(uintptr_t)x, L, a, (u64 *)(uintptr_t)o, out_stride), out);
}

// one drop of the last of `L` moduli, limbs [k0, k1): level B, or that block taken to level A
void ds_drop(const uint64_t *moduli, size_t L, size_t k0, size_t k1, int bgv, uint64_t t, int level_a, uint64_t *out) {
    const std::vector<hp::ModConsts> c = chain_of(moduli, L);
    HpDropArgs da = blank();
    drop_consts(c.data(), L, k0, k1, bgv != 0, t, da.dc);
    da.small_rem = drop_small_rem(c.data(), L, k0, k1);
    if (level_a) drop_consts_to_a(c.data(), k0, k1, da.dc);
    dump(da, out);
}

void ds_post_scalar(uint64_t t, uint64_t q_last, int level_a, uint64_t *out2) { drop_post_scalar(t, q_last, level_a != 0, out2[0], out2[1]); }

// moduli: L + 1; mx6 = {A, A_h, K, K_h, prev_q, prev_half}
void ds_two_drop(const uint64_t *moduli, size_t L, int bgv, uint64_t t1, uint64_t t2, uint64_t *out, uint64_t *mx6) {
    const std::vector<hp::ModConsts> c = chain_of(moduli, L + 1);
    HpDropArgs da = blank();
    HpInvMixArgs mx;
    std::memset(&mx, 0, sizeof(mx));
    two_drop_consts(c.data(), L, bgv != 0, t1, t2, da, mx);
    dump(da, out);
    const uint64_t v[6] = {mx.A, mx.A_h, mx.K, mx.K_h, mx.prev_q, mx.prev_half};
    std::memcpy(mx6, v, sizeof(v));
}

// out4L = pinv[L], pinv_h[L], p_mod_q[L], p_mod_q_h[L]; returns 0 when some q_i divides P
int ds_hks_limbs(const uint64_t *mext, size_t L, size_t k, uint64_t *out4L) {
    HksLimbConsts h;
    if (!hks_limb_consts(mext, L, k, h)) return 0;
    for (size_t i = 0; i < L; i++) {
        out4L[i] = h.pinv[i]; out4L[L + i] = h.pinv_h[i]; out4L[2 * L + i] = h.p_mod_q[i]; out4L[3 * L + i] = h.p_mod_q_h[i];
    }
    return 1;
}

void ds_hks_down(const uint64_t *mext, size_t L, size_t k, size_t i0, size_t cnt, int level_a, uint64_t *out) {
    HksLimbConsts h;
    hks_limb_consts(mext, L, k, h);
    HpDropArgs da = blank();
    hks_down_consts(h, i0, cnt, da);
    if (level_a) hks_down_consts_a(mext, i0, cnt, da);
    dump(da, out);
}

// the kernel flavour of a launch with these fields set (everything else zero): out2 = {level B flavour, its SMALL flag}; returns level A's
int ds_flavours(int fin_on, int raw_input, int comb, int addend, unsigned add_mask, int bgv, int small_rem, int *out2) {
    static const u64 row[1] = {0};
    HpDropArgs da = blank();
    da.fin_on = fin_on; da.raw_input = raw_input; da.comb = comb ? row : nullptr; da.addend = addend ? row : nullptr;
    da.add_mask = add_mask; da.dc.bgv = bgv; da.small_rem = small_rem;
    bool small = false;
    out2[0] = hp_drop_flavour_b(da, &small);
    out2[1] = small ? 1 : 0;
    return hp_drop_flavour_a(da);
}

void ds_hks_down_rescale(const uint64_t *mext, size_t L, size_t k, uint64_t comb, int level_a, uint64_t *out) {
    HksLimbConsts h;
    hks_limb_consts(mext, L, k, h);
    HpDropArgs da = blank();
    hks_down_rescale_consts(h, mext, L, (const u64 *)(uintptr_t)comb, da);
    if (level_a) hks_down_rescale_consts_a(mext, L, da);
    dump(da, out);
}
}
