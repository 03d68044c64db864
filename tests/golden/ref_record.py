"""The compiled reference as recorded results, for tests/test_oracle_vs_reference.py and tests/test_moduli_edges.py where the reference cannot be built.

Every call the tests make on the reference (`ref.<method>(*args)`) is keyed by a digest of the method name and its arguments; the
value is a digest of what the reference returned (or the name of the exception it raised).  `Recorder` wraps the real reference and
writes tests/golden/ref_digests.json (tests/golden/make_ref_digests.py); `Replayer` answers each call with the oracle's result after
checking it against the recorded digest, so a test's `orc.f(x) == ref.f(x)` still pins the oracle to the reference word for word."""
from __future__ import annotations

import hashlib
import json
import os

import numpy as np

DIGESTS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "ref_digests.json")


def _feed(h, x):
    if isinstance(x, np.ndarray):
        h.update(f"a{x.dtype.str}{x.shape}".encode())
        h.update(np.ascontiguousarray(x).tobytes())
    elif isinstance(x, (list, tuple)):
        h.update(f"l{len(x)}(".encode())
        for v in x:
            _feed(h, v)
        h.update(b")")
    elif isinstance(x, (bool, np.bool_)):
        h.update(f"b{bool(x)}".encode())
    elif isinstance(x, (int, np.integer)):
        h.update(f"i{int(x)}".encode())
    elif isinstance(x, str):
        h.update(f"s{len(x)}:{x}".encode())
    elif x is None:
        h.update(b"n")
    else:
        raise TypeError(f"no digest for {type(x).__name__}")


def digest(*parts) -> str:
    h = hashlib.sha256()
    for p in parts:
        _feed(h, p)
    return h.hexdigest()[:24]


def _key(name, args, kwargs):
    return digest(name, list(args), sorted(kwargs.items()))


class Recorder:
    """the real reference; every call's result digest is kept and written by save()"""

    def __init__(self, real):
        self._real, self.table = real, {}

    def __getattr__(self, name):
        f = getattr(self._real, name)

        def call(*args, **kwargs):
            k = _key(name, args, kwargs)
            try:
                out = f(*args, **kwargs)
            except Exception as e:
                self.table[k] = "raise:" + type(e).__name__
                raise
            self.table[k] = digest(out)
            return out
        return call

    def save(self, path=DIGESTS):
        with open(path, "w") as f:
            json.dump({"what": "digests of the compiled reference's results for the calls of tests/test_oracle_vs_reference.py "
                               "and tests/test_moduli_edges.py "
                               "(tests/golden/ref_record.py, tests/golden/make_ref_digests.py)",
                       "calls": dict(sorted(self.table.items()))}, f, indent=0)
            f.write("\n")


class Replayer:
    """the oracle's results, each checked against the reference's recorded digest for the same call"""

    def __init__(self, orc, path=DIGESTS):
        self._orc = orc
        with open(path) as f:
            self.table = json.load(f)["calls"]

    def __getattr__(self, name):
        f = getattr(self._orc, name)

        def call(*args, **kwargs):
            k = _key(name, args, kwargs)
            assert k in self.table, f"no recorded reference result for {name} (tests/golden/make_ref_digests.py)"
            want = self.table[k]
            try:
                out = f(*args, **kwargs)
            except Exception as e:
                assert want == "raise:" + type(e).__name__, f"{name}: the oracle raised {e!r}, the reference gave {want}"
                raise
            assert digest(out) == want, f"{name}: the oracle's result differs from the recorded reference result"
            return out
        return call
