"""Register budget of the plain-modulus ModDown conversion (hp_hks.hip: k_hks_moddown_t<K>, K = 1..8), read from the metadata of the
built library like tests/test_hoisted_resources.py (CPU tier: hipcc cross-compiles, nothing runs).  The kernel is k_hks_moddown<K> with
two multiplications more per coefficient and a by-value block of constants; it must be there for every K, must not use scratch, and must
not cost a wave per SIMD against k_hks_moddown<K> of the SAME build -- the figure is read from that compile, not written down here."""
import pytest

from kernel_budget import meta, needs_llvm, no_scratch, one, waves  # noqa: F401  (meta: the fixture)

pytestmark = needs_llvm

KS = list(range(1, 9))


@pytest.mark.parametrize("K", KS)
def test_every_instantiation_is_built_and_uses_no_scratch(meta, K):
    no_scratch(*one(meta, rf"\bk_hks_moddown_t<{K}>"), sgpr=False)


@pytest.mark.parametrize("K", KS)
def test_occupancy_is_that_of_the_ckks_conversion(meta, K):
    _, plain = one(meta, rf"\bk_hks_moddown<{K}>")
    name, bgv = one(meta, rf"\bk_hks_moddown_t<{K}>")
    print(f"K={K}: k_hks_moddown {plain['vgpr_count']} VGPRs, {plain['sgpr_count']} SGPRs ({waves(plain)} waves); "
          f"k_hks_moddown_t {bgv['vgpr_count']} VGPRs, {bgv['sgpr_count']} SGPRs ({waves(bgv)} waves)")
    assert waves(bgv) >= waves(plain), (name, plain, bgv)
