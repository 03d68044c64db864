"""Register budgets of the kernels hp_dev_ckks_lintrans_bsgs_hks adds (hp_hks.hip), read from the metadata of the built library by the
method of tests/test_lintrans_resources.py (CPU tier: hipcc cross-compiles, nothing runs).  The pre-sum kernel keeps GT giants x two
halves x two words of carry-save accumulators (8 VGPRs each) across a loop of loads; the giant and baby flavours of the accumulate
kernel are k_hks_inner_lintrans with a compile-time branch.  A spill would put scratch traffic inside those loops: only its absence
is asserted.  The counts and the occupancy they leave (512 // vgpr_count waves per SIMD) are findings, recorded in DESIGN 4.7b."""
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


def report(found):
    for name, r in sorted(found.items()):
        print(f"{name}: {r['vgpr_count']} VGPRs, {512 // r['vgpr_count']} waves per SIMD")
        assert r["vgpr_spill_count"] == 0 and r["private_segment_fixed_size"] == 0, (name, r)
        assert r.get("sgpr_spill_count", 0) == 0, (name, r)


def test_presum_kernel_is_built_and_does_not_spill(meta):
    found = {k: v for k, v in meta.items() if re.search(r"\bk_hks_bsgs_presum\b", k)}
    assert found, sorted(k for k in meta if "hks" in k)
    report(found)


def test_every_flavour_of_the_accumulate_kernel_is_built_and_does_not_spill(meta):
    """flat (0), giant (1), baby (2): one instantiation each"""
    found = {k: v for k, v in meta.items() if re.search(r"\bk_hks_inner_lintrans\b", k)}
    flavours = sorted(int(f) for k in found for f in re.findall(r"k_hks_inner_lintrans<(\d+)>", k))
    assert flavours == [0, 1, 2], sorted(found)
    report(found)
