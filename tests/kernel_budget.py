"""What tests/test_kernel_resources.py and the tests/test_<feature>_resources.py files read the shipped kernels' budgets from: the
metadata and the disassembly of the built library (tools/kernel_meta.py), unbundled once per pytest process, and the handful of
assertions every one of them repeats."""
import functools
import os
import re
import shutil
import sys
import tempfile

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import kernel_meta  # noqa: E402

needs_llvm = pytest.mark.skipif(
    not (os.path.exists(f"{kernel_meta.LLVM}/clang-offload-bundler") and shutil.which("objcopy") and shutil.which("c++filt")),
    reason="needs the ROCm LLVM tools")


@functools.lru_cache(maxsize=None)
def _objects(lib, mtime):
    tmp = tempfile.TemporaryDirectory()          # returned with the paths: it lives as long as the cache entry
    return tmp, kernel_meta.code_objects(lib, tmp.name)


def _built():
    from hehub_amd.build import build_lib
    lib = build_lib()
    return lib, os.path.getmtime(lib)


@functools.lru_cache(maxsize=None)
def _meta(lib, mtime):
    return kernel_meta.objects_meta(_objects(lib, mtime)[1])


@functools.lru_cache(maxsize=None)
def _disassembly(lib, mtime):
    return kernel_meta.objects_disassembly(_objects(lib, mtime)[1])


def disassembly():
    """llvm-objdump -d of every code object of the built library"""
    return _disassembly(*_built())


@pytest.fixture(scope="module")
def meta():
    """{demangled kernel name: its metadata record} of the built library"""
    return _meta(*_built())


def some(meta, pattern):
    found = {k: v for k, v in meta.items() if re.search(pattern, k)}
    assert found, pattern
    return found


def one(meta, pattern):
    found = {k: v for k, v in meta.items() if re.search(pattern, k)}
    assert len(found) == 1, (pattern, sorted(found))
    return next(iter(found.items()))


def no_scratch(name, r, sgpr=True, lds=None):
    """no spilled vector register, no private segment; no spilled scalar register unless sgpr=False; lds bytes exactly, if given.
    Prints the record and the occupancy it leaves: the figures DESIGN.md quotes are read from `pytest -s`."""
    print(f"{name}: {r}, {waves(r)} waves per SIMD")
    assert r["vgpr_spill_count"] == 0 and r["private_segment_fixed_size"] == 0, (name, r)
    assert not sgpr or r.get("sgpr_spill_count", 0) == 0, (name, r)
    assert lds is None or r.get("group_segment_fixed_size", 0) == lds, (name, r)


def in_registers(meta, pattern):
    """the budget the sampling, seeded-ciphertext and discrete Gaussian kernels of hp_sample.hip share: there exactly once, no
    scratch, no spills, no LDS, eight waves per SIMD"""
    name, r = one(meta, pattern)
    no_scratch(name, r, lds=0)
    assert r["vgpr_count"] <= 64 and r["sgpr_count"] <= 96, (name, r)   # eight waves per SIMD


def waves(r):
    """waves per SIMD the register counts leave: 512 VGPRs per lane and 800 SGPRs per SIMD, at most 8 waves"""
    return min(8, 512 // max(r["vgpr_count"], 1), 800 // max(r["sgpr_count"], 1))
