"""Register budget of the plain-modulus ModDown conversion (hp_hks.hip: k_hks_moddown_t<K>, K = 1..8), read from the metadata of the
built library like tests/test_hoisted_resources.py (CPU tier: hipcc cross-compiles, nothing runs).  The kernel is k_hks_moddown<K> with
two multiplications more per coefficient and a by-value block of constants; it must be there for every K, must not use scratch, and must
not cost a wave per SIMD against k_hks_moddown<K> of the SAME build -- the figure is read from that compile, not written down here."""
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

KS = list(range(1, 9))


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
def test_every_instantiation_is_built_and_uses_no_scratch(meta, K):
    name, r = one(meta, rf"\bk_hks_moddown_t<{K}>")
    assert r["vgpr_spill_count"] == 0 and r["private_segment_fixed_size"] == 0, (name, r)


@pytest.mark.parametrize("K", KS)
def test_occupancy_is_that_of_the_ckks_conversion(meta, K):
    _, plain = one(meta, rf"\bk_hks_moddown<{K}>")
    name, bgv = one(meta, rf"\bk_hks_moddown_t<{K}>")
    print(f"K={K}: k_hks_moddown {plain['vgpr_count']} VGPRs, {plain['sgpr_count']} SGPRs ({waves(plain)} waves); "
          f"k_hks_moddown_t {bgv['vgpr_count']} VGPRs, {bgv['sgpr_count']} SGPRs ({waves(bgv)} waves)")
    assert waves(bgv) >= waves(plain), (name, plain, bgv)
