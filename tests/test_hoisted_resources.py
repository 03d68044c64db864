"""Register budget of the hoisted-rotation inner product (hp_hks.hip: k_hks_inner_hoisted), read from the metadata of the built library
like tests/test_kernel_resources.py (CPU tier: hipcc cross-compiles, nothing runs).  The kernel holds the carry-save accumulators of
k_hks_inner plus the gather's indices; a spill in its loop would put scratch traffic next to the scattered digit reads it exists to
keep in L2."""
import pytest

from kernel_budget import meta, needs_llvm, no_scratch, one  # noqa: F401  (meta: the fixture)

pytestmark = needs_llvm


@pytest.mark.parametrize("pt", [1, 2])
def test_hoisted_inner_product_is_built_and_does_not_spill(meta, pt):
    no_scratch(*one(meta, rf"k_hks_inner_hoisted<{pt}>"))


def test_hoisted_inner_product_keeps_the_occupancy_of_the_plain_one(meta):
    """two ciphertexts per thread must not cost a wave per SIMD against k_hks_inner<2> (512 VGPRs per SIMD lane: waves = 512 // vgprs)"""
    for pt in (1, 2):
        _, plain = one(meta, rf"k_hks_inner<{pt}>")
        _, hoisted = one(meta, rf"k_hks_inner_hoisted<{pt}>")
        assert 512 // hoisted["vgpr_count"] >= min(8, 512 // plain["vgpr_count"]), (pt, plain, hoisted)
