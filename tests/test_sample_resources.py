"""Register budget of the sampling kernels (hp_sample.hip), read from the metadata of the built library like
tests/test_hks_bgv_resources.py (CPU tier: hipcc cross-compiles, nothing runs).  A ChaCha20 block is 16 state words and 16 working words
per lane; the kernels are VALU-bound, so they must be there in every instantiation, keep the whole block in registers (no scratch, no
spills, no LDS) and leave eight waves per SIMD."""
import pytest

from kernel_budget import disassembly, in_registers, meta, needs_llvm  # noqa: F401  (meta: the fixture)

pytestmark = needs_llvm

KERNELS = [r"\bk_sample_uniform<false>", r"\bk_sample_uniform<true>", r"\bk_sample_signed<2u?>", r"\bk_sample_signed<3u?>"]


@pytest.mark.parametrize("pattern", KERNELS)
def test_sampling_kernels_keep_the_block_in_registers(meta, pattern):
    in_registers(meta, pattern)


def test_rotations_are_single_instructions():
    """__builtin_rotateleft32 becomes v_alignbit_b32: the 32 rotations of a double round (the ten double rounds stay a loop)"""
    text = disassembly()
    start = text.index("k_sample_signedILj3E")
    body = text[start:text.index("s_endpgm", start)]
    assert body.count("v_alignbit_b32") >= 32, body.count("v_alignbit_b32")
