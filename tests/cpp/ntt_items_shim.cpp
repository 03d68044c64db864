// ntt_items_shim.cpp -- C entry points around the work-item numbering of the transform launches (hehub_amd/csrc/hp_ntt_job.h,
// hp_device.h) so the CPU test-suite can enumerate every item of a launch without a GPU.  Test infrastructure only.
// Compiled as HIP, host side only (the headers need hip_runtime.h): tests/test_host_ntt_items.py has the command.
//
// The jobs the test hands in have src = dst = NULL and logn = 1: an item's pointers are then row * n words from zero, a row index
// once divided out, and nothing is ever dereferenced.
#include "../../hehub_amd/csrc/hp_ntt_job.h"

namespace {

uint64_t row_of(const u64 *p, size_t n) { return (uint64_t)((uintptr_t)p / (sizeof(u64) * n)); }

} // namespace

extern "C" {

unsigned ni_sizeof_job() { return (unsigned)sizeof(HpNttJob); }
unsigned ni_max_limbs() { return HP_MAX_LIMBS; }

unsigned ni_spread_items(unsigned L, unsigned P, unsigned k0, unsigned k1) { return hp_spread_items(L, P, k0, k1); }
unsigned ni_hks_items(unsigned L, unsigned nd, unsigned k, unsigned P) { return hp_hks_items(L, nd, k, P); }
unsigned ni_inv_grid(const HpNttJob *job, unsigned LPW) { return hp_inv_grid(*job, LPW); }

// out[b] = hp_xcd_remap(b, W) for b < W
void ni_xcd_remap(unsigned W, uint32_t *out) {
    for (u32 b = 0; b < W; b++) out[b] = hp_xcd_remap(b, W);
}

// the forward kernels' prologue for every workgroup b < job->W: w = hp_xcd_remap(b, W), hp_decode_item(job, w)
//   -> out[4 b ..] = {src row, dst row, limb, poly}; returns how many items decoded (W unless the mode is unknown)
unsigned ni_decode(const HpNttJob *job, uint64_t *out) {
    const size_t n = (size_t)1 << job->logn;
    unsigned ok = 0;
    for (u32 b = 0; b < job->W; b++) {
        HpItem it = {nullptr, nullptr, ~0u, ~0u};
        if (!hp_decode_item(*job, hp_xcd_remap(b, job->W), it)) continue;
        ok++;
        out[4 * (size_t)b + 0] = row_of(it.src, n);
        out[4 * (size_t)b + 1] = row_of(it.dst, n);
        out[4 * (size_t)b + 2] = it.limb;
        out[4 * (size_t)b + 3] = it.poly;
    }
    return ok;
}

// the tiled inverse kernels' prologue for every (workgroup b < grid, sub-limb s < LPW):
//   -> out[5 (b LPW + s) ..] = {active, src row, dst row, limb, poly}
void ni_inv_items(const HpNttJob *job, unsigned LPW, unsigned grid, uint64_t *out) {
    const size_t n = (size_t)1 << job->logn;
    for (u32 b = 0; b < grid; b++)
        for (u32 s = 0; s < LPW; s++) {
            HpItem it = {nullptr, nullptr, ~0u, ~0u};
            uint64_t *o = out + 5 * ((size_t)b * LPW + s);
            o[0] = hp_inv_item(*job, b, s, LPW, n, it) ? 1 : 0;
            o[1] = row_of(it.src, n);
            o[2] = row_of(it.dst, n);
            o[3] = it.limb;
            o[4] = it.poly;
        }
}

// out[2 b ..] = (unit, w) of workgroup b < units * W (hp_hks.hip: the hoisted and the diagonal inner products)
void ni_xcd_units(unsigned units, unsigned W, uint32_t *out) {
    for (u32 b = 0; b < units * W; b++) hp_xcd_unit(b, units, W, out[2 * (size_t)b], out[2 * (size_t)b + 1]);
}
}
