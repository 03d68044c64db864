"""Register budget of the ModRaise transform (hp_ntt_raise.hip: k_ntt_raise), read from the metadata of the built library like
tests/test_polyeval_resources.py (CPU tier: hipcc cross-compiles, nothing runs).  The kernel is the tiled forward transform with a
Barrett reduction and a centring in its loads: every tiled ring degree is built, and like k_ntt_fwd it must hold four waves per
SIMD (at most 128 VGPRs) without a spill or a private segment -- scratch traffic in its first pass would sit in front of every
butterfly.  N = 32768 keeps the one-workgroup-per-CU geometry of the other N = 32768 transforms."""
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


def test_every_tiled_size_is_built_and_none_spills(meta):
    for logn in range(11, 16):
        found = {k: v for k, v in meta.items() if re.search(rf"\bk_ntt_raise<{logn}>", k)}
        assert len(found) == 1, (logn, sorted(k for k in meta if "raise" in k))
        (name, r), = found.items()
        print(f"{name}: {r['vgpr_count']} VGPRs, {r.get('sgpr_count')} SGPRs, LDS {r['group_segment_fixed_size']}")
        assert r["vgpr_spill_count"] == 0 and r["private_segment_fixed_size"] == 0, (name, r)
        assert r.get("sgpr_spill_count", 0) == 0, (name, r)
        assert r["vgpr_count"] <= 128, (name, r)
    (name, r), = {k: v for k, v in meta.items() if re.search(r"\bk_ntt_raise<15>", k)}.items()
    assert 140 * 1024 <= r["group_segment_fixed_size"] <= 160 * 1024, (name, r)


def test_no_other_instantiation(meta):
    """the call launches these five and nothing else of its own: the composed form runs the existing kernels"""
    assert len([k for k in meta if "k_ntt_raise" in k]) == 5
