"""The polynomial-evaluation entry points at the C boundary (CPU tier: nothing is launched): include/hehub_amd.h declares
hp_dev_ckks_lincomb and hp_dev_ckks_eval_plan_hks with these argument counts, hehub_amd/capi.py carries the plan's three structs
field for field, and a plan of hehub_amd/polyeval.py marshals to those structs (exported, typed as the header types them, refusing a
NULL context: every call, tests/test_capi_symbols.py).  What they compute: tests/test_gpu_lincomb.py and tests/test_gpu_polyeval.py."""
import ctypes as C
import os
import re

import abi

ROOT = abi.ROOT
COUNTS = {"hp_dev_ckks_lincomb": 11, "hp_dev_ckks_eval_plan_hks": 14}


def test_header_declares_the_calls():
    assert {name: len(abi.parameter_names(name)) for name in COUNTS} == COUNTS


def test_header_says_what_is_out_of_scope():
    m = re.search(r"Out of scope:(.*?)\*/", abi.header_text(), flags=re.S)
    assert m
    for what in ("tree-mode", "node", "sharded", "host layers", "encoding", "odd/even", "dead elements"):
        assert what in m.group(1), what


def test_ctypes_structs_have_the_header_layout(tmp_path):
    """sizeof and offsetof of the three plan structs, from a C program compiled against the header"""
    import subprocess

    from hehub_amd import capi

    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "hehub_amd.h"\n'
                   'int main(void) { printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu\\n", sizeof(hp_eval_term), offsetof(hp_eval_term, coef), '
                   'sizeof(hp_eval_form), offsetof(hp_eval_form, term), offsetof(hp_eval_form, cst), sizeof(hp_eval_step), '
                   'offsetof(hp_eval_step, products), offsetof(hp_eval_step, x), offsetof(hp_eval_step, y), offsetof(hp_eval_step, z), '
                   'offsetof(hp_eval_term, elem)); return 0; }\n')
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", f"-I{os.path.join(ROOT, 'include')}", str(src), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    T, F, S = capi.EvalTerm, capi.EvalForm, capi.EvalStep
    assert got == [C.sizeof(T), T.coef.offset, C.sizeof(F), F.term.offset, F.cst.offset, C.sizeof(S), S.products.offset, S.x.offset,
                   S.y.offset, S.z.offset, T.elem.offset]


def test_engine_has_the_front_end_methods():
    from hehub_amd.engine import Engine

    for method in ("ckks_lincomb", "ckks_poly_eval_hks"):
        assert callable(getattr(Engine, method))


def test_a_plan_marshals_to_the_structs():
    """residues of the integer constants (negative ones included) modulo the level's moduli, NULL for 1 and for 0"""
    import params as P
    from hehub_amd.polyeval import build_plan

    q = P.P40[:6]
    plan = build_plan([0.5, -0.25, 0.0, 0.125, 1.0, -1.0], "chebyshev", q, 1 << 40, 1 << 40, n1=4)
    steps, keep = plan.marshal()
    assert len(steps) == len(plan.steps) and keep
    for dst, s in zip(steps, plan.steps):
        assert (dst.level, dst.products) == (s.level, len(s.products))
        pairs = [(dst.z, s.z)] + [(dst.x[t], fx) for t, (fx, _) in enumerate(s.products)] + [(dst.y[t], fy) for t, (_, fy) in enumerate(s.products)]
        for got, form in pairs:
            assert got.terms == len(form.terms)
            for j, (e, c) in enumerate(form.terms):
                assert got.term[j].elem == e and bool(got.term[j].coef) == (c is not None)
                if c is not None:
                    assert [got.term[j].coef[m] for m in range(s.level)] == [c % q[m] for m in range(s.level)]
            assert bool(got.cst) == (form.cst is not None)
            if form.cst is not None:
                assert [got.cst[m] for m in range(s.level)] == [form.cst % q[m] for m in range(s.level)]
