"""Register budget of the sampling kernels (hp_sample.hip), read from the metadata of the built library like
tests/test_hks_bgv_resources.py (CPU tier: hipcc cross-compiles, nothing runs).  A ChaCha20 block is 16 state words and 16 working words
per lane; the kernels are VALU-bound, so they must be there in every instantiation, keep the whole block in registers (no scratch, no
spills, no LDS) and leave eight waves per SIMD."""
import os
import re
import shutil
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

pytestmark = pytest.mark.skipif(
    not (os.path.exists("/opt/rocm/lib/llvm/bin/clang-offload-bundler") and shutil.which("objcopy") and shutil.which("c++filt")),
    reason="needs the ROCm LLVM tools")

KERNELS = [r"\bk_sample_uniform<false>", r"\bk_sample_uniform<true>", r"\bk_sample_signed<2u?>", r"\bk_sample_signed<3u?>"]


@pytest.fixture(scope="module")
def meta():
    from hehub_amd.build import build_lib
    from kernel_meta import kernel_meta
    return kernel_meta(build_lib())


@pytest.mark.parametrize("pattern", KERNELS)
def test_sampling_kernels_keep_the_block_in_registers(meta, pattern):
    found = {k: v for k, v in meta.items() if re.search(pattern, k)}
    assert len(found) == 1, (pattern, sorted(found))
    name, r = next(iter(found.items()))
    print(name, {k: r.get(k) for k in ("vgpr_count", "sgpr_count", "vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size",
                                       "group_segment_fixed_size")})
    assert r["vgpr_spill_count"] == 0 and r.get("sgpr_spill_count", 0) == 0 and r["private_segment_fixed_size"] == 0, (name, r)
    assert r.get("group_segment_fixed_size", 0) == 0, (name, r)
    assert r["vgpr_count"] <= 64 and r["sgpr_count"] <= 96, (name, r)   # eight waves per SIMD


def test_rotations_are_single_instructions():
    """__builtin_rotateleft32 becomes v_alignbit_b32: the 32 rotations of a double round (the ten double rounds stay a loop)"""
    from hehub_amd.build import build_lib
    from kernel_meta import disassembly

    text = disassembly(build_lib())
    start = text.index("k_sample_signedILj3E")
    body = text[start:text.index("s_endpgm", start)]
    assert body.count("v_alignbit_b32") >= 32, body.count("v_alignbit_b32")
