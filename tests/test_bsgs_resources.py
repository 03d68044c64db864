"""Register budgets of the kernels hp_dev_ckks_lintrans_bsgs_hks adds (hp_hks.hip), read from the metadata of the built library by the
method of tests/test_lintrans_resources.py (CPU tier: hipcc cross-compiles, nothing runs).  The pre-sum kernel keeps GT giants x two
halves x two words of carry-save accumulators (8 VGPRs each) across a loop of loads; the giant and baby flavours of the accumulate
kernel are k_hks_inner_lintrans with a compile-time branch.  A spill would put scratch traffic inside those loops: only its absence
is asserted.  The counts and the occupancy they leave (512 // vgpr_count waves per SIMD) are findings, recorded in DESIGN 4.7b."""
import re

from kernel_budget import meta, needs_llvm, no_scratch, some  # noqa: F401  (meta: the fixture)

pytestmark = needs_llvm


def test_presum_kernel_is_built_and_does_not_spill(meta):
    for name, r in sorted(some(meta, r"\bk_hks_bsgs_presum\b").items()):
        no_scratch(name, r)


def test_every_flavour_of_the_accumulate_kernel_is_built_and_does_not_spill(meta):
    """flat (0), giant (1), baby (2): one instantiation each"""
    found = some(meta, r"\bk_hks_inner_lintrans\b")
    flavours = sorted(int(f) for k in found for f in re.findall(r"k_hks_inner_lintrans<(\d+)>", k))
    assert flavours == [0, 1, 2], sorted(found)
    for name, r in sorted(found.items()):
        no_scratch(name, r)
