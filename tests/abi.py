"""include/hehub_amd.h, parsed once for every test of the C boundary: prototypes() is the header's side of the ctypes table in
hehub_amd/capi.py.  A feature's test imports this and asserts what is its own (parameter names, orders, phrases); that every
declared symbol is exported, typed as the header types it and refuses a NULL context is asserted table-wide in
tests/test_capi_symbols.py."""
import ctypes as C
import functools
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "hehub_amd.h")

# what capi.py may hold for a type class of the header; "ptr" is anything with a `*`.  The comparison is by identity of the ctypes
# class, so types that ctypes makes one class on the platform are not told apart: on LP64 Linux c_size_t, c_uint64 and c_ulong
# are all c_ulong, and a size_t / uint64_t mix-up (no ABI difference there) passes.
CTYPES = {"int": C.c_int, "size_t": C.c_size_t, "uint64_t": C.c_uint64, "uint32_t": C.c_uint32, "unsigned": C.c_uint,
          "unsigned long": C.c_ulong, "void": None}


def header_text():
    """the header as written, comments included"""
    return open(HEADER).read()


@functools.lru_cache(maxsize=None)
def _stripped():
    return re.sub(r"^\s*#.*$", "", re.sub(r"/\*.*?\*/", "", header_text(), flags=re.S), flags=re.M)


def type_class(decl):
    return "ptr" if "*" in decl else " ".join(w for w in decl.split() if w != "const")


@functools.lru_cache(maxsize=None)
def prototypes():
    """{name: (return type class, [(type class, parameter name), ...])} of every function the header declares"""
    found = {}
    for m in re.finditer(r"(?:^|[;{}])\s*([\w\s*]+?)\s*\b(hp_[a-z0-9_]+)\s*\(([^()]*)\)\s*(?=;)", _stripped()):
        ret, name, params = m.groups()
        assert name not in found, name
        params = [p.strip() for p in params.split(",") if p.strip() not in ("", "void")]
        found[name] = (type_class(ret), [(type_class(p[:re.search(r"\w+$", p).start()]), re.search(r"\w+$", p).group()) for p in params])
    return found


def parameter_names(name):
    return [p for _, p in prototypes()[name][1]]


def parameter_list_text(name):
    """the text between the prototype's parentheses, blanks normalised"""
    return " ".join(re.search(r"\b%s\s*\(([^()]*)\)\s*;" % name, _stripped()).group(1).split())


def agrees(ctype, cls):
    """whether a restype / argtypes entry of capi.py is what the header's type class asks for"""
    if cls == "ptr":
        return ctype in (C.c_void_p, C.c_char_p) or (isinstance(ctype, type) and issubclass(ctype, C._Pointer))
    return cls in CTYPES and ctype is CTYPES[cls]


def null_context_call(lib, name, fill=0):
    """call name with a NULL context, NULL for every other pointer and fill for every value"""
    return getattr(lib, name)(*[None if cls == "ptr" else fill for cls, _ in prototypes()[name][1]])
