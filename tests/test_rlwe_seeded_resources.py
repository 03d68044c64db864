"""Register budget of the seeded-ciphertext kernels (hp_sample.hip), read from the metadata of the built library like
tests/test_sample_resources.py (CPU tier: hipcc cross-compiles, nothing runs; metadata only, never disassembly).  Every instantiation is
there exactly once, keeps everything in registers (no scratch, no spills, no LDS) and fits the sampling kernels' budget of eight waves per
SIMD: VGPR <= 64, SGPR <= 96.  The fused kernel k_enc_seeded holds the 8 words of a beside the block; it loads its operands in two
halves of 12 words, which is what keeps all four instantiations inside the 64 registers -- the cap is NOT raised."""
import re

import pytest

from kernel_budget import in_registers, meta, needs_llvm  # noqa: F401  (meta: the fixture)

pytestmark = needs_llvm

KERNELS = [r"\bk_sample_spread<2u?>", r"\bk_sample_spread<3u?>", r"\bk_enc_seeded<true, true>", r"\bk_enc_seeded<true, false>",
           r"\bk_enc_seeded<false, true>", r"\bk_enc_seeded<false, false>", r"\bk_enc_pk_fin\(", r"\bk_sample_canonical\("]


@pytest.mark.parametrize("pattern", KERNELS)
def test_kernels_are_present_once_and_keep_everything_in_registers(meta, pattern):
    in_registers(meta, pattern)


def test_no_other_instantiation_exists(meta):
    names = [k for k in meta if re.search(r"\bk_(sample_spread|enc_seeded|enc_pk_fin)\b", k)]
    assert len(names) == 7, sorted(names)
