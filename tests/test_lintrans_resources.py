"""Register budget of the accumulate kernel of the diagonal linear transform (hp_hks.hip: k_hks_inner_lintrans), read from the metadata
of the built library like tests/test_hoisted_resources.py (CPU tier: hipcc cross-compiles, nothing runs).  The kernel holds TWO sets of
carry-save accumulators per output pair -- the digit sum of the current rotation and the weighted sum over the rotations -- and keeps
both across a loop of scattered loads: a spill there would put scratch traffic inside that loop.  Only the absence of spills is
asserted; the occupancy the two sets leave (512 // vgpr_count waves per SIMD) is a finding, recorded in DESIGN 4.7a."""
from kernel_budget import meta, needs_llvm, no_scratch, some  # noqa: F401  (meta: the fixture)

pytestmark = needs_llvm


def test_lintrans_accumulate_kernel_is_built_and_does_not_spill(meta):
    """the kernel is not a template (one ciphertext per thread at every batch); any instantiation a later change adds is held to the same"""
    for name, r in some(meta, r"\bk_hks_inner_lintrans\b").items():
        no_scratch(name, r)
