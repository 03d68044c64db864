"""Register budget of the ModRaise transform (hp_ntt_raise.hip: k_ntt_raise), read from the metadata of the built library like
tests/test_polyeval_resources.py (CPU tier: hipcc cross-compiles, nothing runs).  The kernel is the tiled forward transform with a
Barrett reduction and a centring in its loads: every tiled ring degree is built, and like k_ntt_fwd it must hold four waves per
SIMD (at most 128 VGPRs) without a spill or a private segment -- scratch traffic in its first pass would sit in front of every
butterfly.  N = 32768 keeps the one-workgroup-per-CU geometry of the other N = 32768 transforms."""
from kernel_budget import meta, needs_llvm, no_scratch, one  # noqa: F401  (meta: the fixture)

pytestmark = needs_llvm


def test_every_tiled_size_is_built_and_none_spills(meta):
    for logn in range(11, 16):
        name, r = one(meta, rf"\bk_ntt_raise<{logn}>")
        no_scratch(name, r)
        assert r["vgpr_count"] <= 128, (name, r)
    name, r = one(meta, r"\bk_ntt_raise<15>")
    assert 140 * 1024 <= r["group_segment_fixed_size"] <= 160 * 1024, (name, r)


def test_no_other_instantiation(meta):
    """the call launches these five and nothing else of its own: the composed form runs the existing kernels"""
    assert len([k for k in meta if "k_ntt_raise" in k]) == 5
