"""Register budget of the discrete Gaussian instantiations of the sampling kernels (hp_sample.hip: k_sample_signed<4> and
k_gauss_spread, the Gaussian twin of k_sample_spread under a name of its own), read from the metadata of the built library like
tests/test_sample_resources.py (CPU tier: hipcc cross-compiles, nothing runs).  The 30 table entries are literals of the unrolled compare chain: were the table in memory, or the chain's operands
spilled, the kernel would show scratch, LDS or a register count above what leaves eight waves per SIMD."""
import pytest

from kernel_budget import in_registers, meta, needs_llvm, one  # noqa: F401  (meta: the fixture)

pytestmark = needs_llvm

KERNELS = [r"\bk_sample_signed<4u?>", r"\bk_gauss_spread\("]


@pytest.mark.parametrize("pattern", KERNELS)
def test_gaussian_kernels_keep_block_and_table_in_registers(meta, pattern):
    in_registers(meta, pattern)


def test_the_instantiations_that_were_there_are_still_there(meta):
    for pattern in (r"\bk_sample_signed<2u?>", r"\bk_sample_signed<3u?>", r"\bk_sample_spread<2u?>", r"\bk_sample_spread<3u?>"):
        one(meta, pattern)
