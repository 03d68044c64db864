"""Register budget of the BFV kernels (hp_bfv.hip: k_bfv_lift<K>, k_bfv_scale<K>, k_bfv_decrypt_round<K>; K = 1..8 exactly, 16 for
the widths 9..16), read from the metadata of the built library like tests/test_hks_bgv_resources.py (CPU tier: hipcc cross-compiles,
nothing runs).  Every instantiation must be there and none may use scratch or spill, vector or scalar registers -- that is why the
scaling is two kernels.  The
VGPR / SGPR counts and the waves per SIMD they leave are printed for DESIGN.md; no occupancy threshold is fixed in advance."""
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

KERNELS = ["k_bfv_lift", "k_bfv_scale", "k_bfv_decrypt_round"]
KS = list(range(1, 9)) + [16]


@pytest.fixture(scope="module")
def meta():
    from hehub_amd.build import build_lib
    from kernel_meta import kernel_meta
    return kernel_meta(build_lib())


def one(meta, pattern):
    found = {k: v for k, v in meta.items() if re.search(pattern, k)}
    assert len(found) == 1, (pattern, sorted(found))
    return next(iter(found.items()))


def waves(r):
    """waves per SIMD the register counts leave: 512 VGPRs per lane and 800 SGPRs per SIMD, at most 8 waves"""
    return min(8, 512 // max(r["vgpr_count"], 1), 800 // max(r["sgpr_count"], 1))


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("kernel", KERNELS)
def test_every_instantiation_is_built_and_uses_no_scratch(meta, kernel, K):
    name, r = one(meta, rf"\b{kernel}<{K}>")
    print(f"{kernel}<{K}>: {r['vgpr_count']} VGPRs, {r['sgpr_count']} SGPRs, {waves(r)} waves per SIMD, "
          f"scratch {r['private_segment_fixed_size']} B, spills {r['vgpr_spill_count']} vector / {r.get('sgpr_spill_count', 0)} scalar")
    assert r["vgpr_spill_count"] == 0 and r["private_segment_fixed_size"] == 0 and r.get("sgpr_spill_count", 0) == 0, (name, r)


def test_the_reduction_kernel_is_built_and_uses_no_scratch(meta):
    name, r = one(meta, r"\bk_bfv_canonical\b")
    assert r["vgpr_spill_count"] == 0 and r["private_segment_fixed_size"] == 0, (name, r)
