"""Register budget of the hoisted-rotation inner product (hp_hks.hip: k_hks_inner_hoisted), read from the metadata of the built library
like tests/test_kernel_resources.py (CPU tier: hipcc cross-compiles, nothing runs).  The kernel holds the carry-save accumulators of
k_hks_inner plus the gather's indices; a spill in its loop would put scratch traffic next to the scattered digit reads it exists to
keep in L2."""
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


@pytest.fixture(scope="module")
def meta():
    from hehub_amd.build import build_lib
    from kernel_meta import kernel_meta
    return kernel_meta(build_lib())


@pytest.mark.parametrize("pt", [1, 2])
def test_hoisted_inner_product_is_built_and_does_not_spill(meta, pt):
    found = {k: v for k, v in meta.items() if re.search(rf"k_hks_inner_hoisted<{pt}>", k)}
    assert len(found) == 1, sorted(found)
    (name, r), = found.items()
    assert r["vgpr_spill_count"] == 0 and r["private_segment_fixed_size"] == 0, (name, r)
    assert r.get("sgpr_spill_count", 0) == 0, (name, r)


def test_hoisted_inner_product_keeps_the_occupancy_of_the_plain_one(meta):
    """two ciphertexts per thread must not cost a wave per SIMD against k_hks_inner<2> (512 VGPRs per SIMD lane: waves = 512 // vgprs)"""
    for pt in (1, 2):
        (plain,) = [v for k, v in meta.items() if re.search(rf"k_hks_inner<{pt}>", k)]
        (hoisted,) = [v for k, v in meta.items() if re.search(rf"k_hks_inner_hoisted<{pt}>", k)]
        assert 512 // hoisted["vgpr_count"] >= min(8, 512 // plain["vgpr_count"]), (pt, plain, hoisted)
