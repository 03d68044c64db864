"""Record tests/golden/ref_digests.json: the digests of the compiled reference's results for every call that
tests/test_oracle_vs_reference.py, tests/test_moduli_edges.py and the CPU part of tests/test_gpu_elem_tiles.py make
(tests/golden/ref_record.py).  Run where oracle/_ref/libhehub_ref.so is built:

    python tests/golden/make_ref_digests.py"""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

if __name__ == "__main__":
    env = dict(os.environ, HP_RECORD_REF_DIGESTS="1")
    sys.exit(subprocess.call([sys.executable, "-m", "pytest", "-q", "-p", "no:cacheprovider", "-m", "not gpu",
                             os.path.join(ROOT, "tests", "test_oracle_vs_reference.py"),
                             os.path.join(ROOT, "tests", "test_moduli_edges.py"), os.path.join(ROOT, "tests", "test_gpu_elem_tiles.py")],
                             env=env, cwd=ROOT))
