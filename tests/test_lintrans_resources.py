"""Register budget of the accumulate kernel of the diagonal linear transform (hp_hks.hip: k_hks_inner_lintrans), read from the metadata
of the built library like tests/test_hoisted_resources.py (CPU tier: hipcc cross-compiles, nothing runs).  The kernel holds TWO sets of
carry-save accumulators per output pair -- the digit sum of the current rotation and the weighted sum over the rotations -- and keeps
both across a loop of scattered loads: a spill there would put scratch traffic inside that loop.  Only the absence of spills is
asserted; the occupancy the two sets leave (512 // vgpr_count waves per SIMD) is a finding, recorded in DESIGN 4.7a."""
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


def test_lintrans_accumulate_kernel_is_built_and_does_not_spill(meta):
    """the kernel is not a template (one ciphertext per thread at every batch); any instantiation a later change adds is held to the same"""
    found = {k: v for k, v in meta.items() if re.search(r"\bk_hks_inner_lintrans\b", k)}
    assert found, sorted(k for k in meta if "hks" in k)
    for name, r in found.items():
        print(f"{name}: {r['vgpr_count']} VGPRs, {512 // r['vgpr_count']} waves per SIMD")
        assert r["vgpr_spill_count"] == 0 and r["private_segment_fixed_size"] == 0, (name, r)
        assert r.get("sgpr_spill_count", 0) == 0, (name, r)
