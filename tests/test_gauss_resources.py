"""Register budget of the discrete Gaussian instantiations of the sampling kernels (hp_sample.hip: k_sample_signed<4> and
k_gauss_spread, the Gaussian twin of k_sample_spread under a name of its own), read from the metadata of the built library like
tests/test_sample_resources.py (CPU tier: hipcc cross-compiles, nothing runs).  The 30 table entries are literals of the unrolled compare chain: were the table in memory, or the chain's operands
spilled, the kernel would show scratch, LDS or a register count above what leaves eight waves per SIMD."""
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

KERNELS = [r"\bk_sample_signed<4u?>", r"\bk_gauss_spread\("]


@pytest.fixture(scope="module")
def meta():
    from hehub_amd.build import build_lib
    from kernel_meta import kernel_meta
    return kernel_meta(build_lib())


@pytest.mark.parametrize("pattern", KERNELS)
def test_gaussian_kernels_keep_block_and_table_in_registers(meta, pattern):
    found = {k: v for k, v in meta.items() if re.search(pattern, k)}
    assert len(found) == 1, (pattern, sorted(found))
    name, r = next(iter(found.items()))
    print(name, {k: r.get(k) for k in ("vgpr_count", "sgpr_count", "vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size",
                                       "group_segment_fixed_size")})
    assert r["vgpr_spill_count"] == 0 and r.get("sgpr_spill_count", 0) == 0 and r["private_segment_fixed_size"] == 0, (name, r)
    assert r.get("group_segment_fixed_size", 0) == 0, (name, r)
    assert r["vgpr_count"] <= 64 and r["sgpr_count"] <= 96, (name, r)   # eight waves per SIMD


def test_the_instantiations_that_were_there_are_still_there(meta):
    for pattern in (r"\bk_sample_signed<2u?>", r"\bk_sample_signed<3u?>", r"\bk_sample_spread<2u?>", r"\bk_sample_spread<3u?>"):
        assert len([k for k in meta if re.search(pattern, k)]) == 1, pattern
