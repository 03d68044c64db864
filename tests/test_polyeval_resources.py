"""Register budget of the ciphertext linear-combination kernel (hp_lincomb.hip: k_ct_lincomb), read from the metadata of the built
library like tests/test_dot_resources.py (CPU tier: hipcc cross-compiles, nothing runs).  The kernel keeps eight carry-save
accumulators (four rounds x two words, 64 VGPRs) across its loop over the terms, next to the four 16-byte loads of a term: a spill
there would put scratch traffic inside a streaming loop.  Only the absence of spills and of a private segment is asserted; the VGPR
count and the occupancy it leaves (512 // vgpr_count waves per SIMD) are a finding, recorded in DESIGN 4.7j."""
from kernel_budget import meta, needs_llvm, no_scratch, some  # noqa: F401  (meta: the fixture)

pytestmark = needs_llvm


def test_lincomb_kernel_is_built_and_does_not_spill(meta):
    """the kernel is not a template; any instantiation a later change adds is held to the same"""
    for name, r in some(meta, r"\bk_ct_lincomb\b").items():
        no_scratch(name, r)
