"""Register budget of the seeded-ciphertext kernels (hp_sample.hip), read from the metadata of the built library like
tests/test_sample_resources.py (CPU tier: hipcc cross-compiles, nothing runs; metadata only, never disassembly).  Every instantiation is
there exactly once, keeps everything in registers (no scratch, no spills, no LDS) and fits the sampling kernels' budget of eight waves per
SIMD: VGPR <= 64, SGPR <= 96.  The fused kernel k_enc_seeded holds the 8 words of a beside the block; it loads its operands in two
halves of 12 words, which is what keeps all four instantiations inside the 64 registers -- the cap is NOT raised."""
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

KERNELS = [r"\bk_sample_spread<2u?>", r"\bk_sample_spread<3u?>", r"\bk_enc_seeded<true, true>", r"\bk_enc_seeded<true, false>",
           r"\bk_enc_seeded<false, true>", r"\bk_enc_seeded<false, false>", r"\bk_enc_pk_fin\(", r"\bk_sample_canonical\("]


@pytest.fixture(scope="module")
def meta():
    from hehub_amd.build import build_lib
    from kernel_meta import kernel_meta
    return kernel_meta(build_lib())


@pytest.mark.parametrize("pattern", KERNELS)
def test_kernels_are_present_once_and_keep_everything_in_registers(meta, pattern):
    found = {k: v for k, v in meta.items() if re.search(pattern, k)}
    assert len(found) == 1, (pattern, sorted(found))
    name, r = next(iter(found.items()))
    print(name, {k: r.get(k) for k in ("vgpr_count", "sgpr_count", "vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size",
                                       "group_segment_fixed_size")})
    assert r["vgpr_spill_count"] == 0 and r.get("sgpr_spill_count", 0) == 0 and r["private_segment_fixed_size"] == 0, (name, r)
    assert r.get("group_segment_fixed_size", 0) == 0, (name, r)
    assert r["vgpr_count"] <= 64 and r["sgpr_count"] <= 96, (name, r)   # eight waves per SIMD


def test_no_other_instantiation_exists(meta):
    names = [k for k in meta if re.search(r"\bk_(sample_spread|enc_seeded|enc_pk_fin)\b", k)]
    assert len(names) == 7, sorted(names)
