"""Register budget of the ciphertext linear-combination kernel (hp_lincomb.hip: k_ct_lincomb), read from the metadata of the built
library like tests/test_dot_resources.py (CPU tier: hipcc cross-compiles, nothing runs).  The kernel keeps eight carry-save
accumulators (four rounds x two words, 64 VGPRs) across its loop over the terms, next to the four 16-byte loads of a term: a spill
there would put scratch traffic inside a streaming loop.  Only the absence of spills and of a private segment is asserted; the VGPR
count and the occupancy it leaves (512 // vgpr_count waves per SIMD) are a finding, recorded in DESIGN 4.7j."""
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


def test_lincomb_kernel_is_built_and_does_not_spill(meta):
    """the kernel is not a template; any instantiation a later change adds is held to the same"""
    found = {k: v for k, v in meta.items() if re.search(r"\bk_ct_lincomb\b", k)}
    assert found, sorted(k for k in meta if "lincomb" in k)
    for name, r in found.items():
        print(f"{name}: {r['vgpr_count']} VGPRs, {r.get('sgpr_count')} SGPRs, {512 // r['vgpr_count']} waves per SIMD")
        assert r["vgpr_spill_count"] == 0 and r["private_segment_fixed_size"] == 0, (name, r)
        assert r.get("sgpr_spill_count", 0) == 0, (name, r)
