"""Record tests/golden/ref_digests.json: the digests of the compiled reference's results for every call that
tests/test_oracle_vs_reference.py and tests/test_moduli_edges.py make (tests/golden/ref_record.py).  Run where oracle/_ref/libhehub_ref.so is built:

    python tests/golden/make_ref_digests.py"""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

if __name__ == "__main__":
    env = dict(os.environ, HP_RECORD_REF_DIGESTS="1")
    sys.exit(subprocess.call([sys.executable, "-m", "pytest", "-q", "-p", "no:cacheprovider", os.path.join(ROOT, "tests", "test_oracle_vs_reference.py"),
                             os.path.join(ROOT, "tests", "test_moduli_edges.py")],
                             env=env, cwd=ROOT))
