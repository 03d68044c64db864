"""Register budget of the BFV kernels (hp_bfv.hip: k_bfv_lift<K>, k_bfv_scale<K>, k_bfv_decrypt_round<K>; K = 1..8 exactly, 16 for
the widths 9..16), read from the metadata of the built library like tests/test_hks_bgv_resources.py (CPU tier: hipcc cross-compiles,
nothing runs).  Every instantiation must be there and none may use scratch or spill, vector or scalar registers -- that is why the
scaling is two kernels.  The
VGPR / SGPR counts and the waves per SIMD they leave are printed for DESIGN.md; no occupancy threshold is fixed in advance."""
import pytest

from kernel_budget import meta, needs_llvm, no_scratch, one  # noqa: F401  (meta: the fixture)

pytestmark = needs_llvm

KERNELS = ["k_bfv_lift", "k_bfv_scale", "k_bfv_decrypt_round"]
KS = list(range(1, 9)) + [16]


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("kernel", KERNELS)
def test_every_instantiation_is_built_and_uses_no_scratch(meta, kernel, K):
    no_scratch(*one(meta, rf"\b{kernel}<{K}>"))


def test_the_reduction_kernel_is_built_and_uses_no_scratch(meta):
    no_scratch(*one(meta, r"\bk_bfv_canonical\b"), sgpr=False)
