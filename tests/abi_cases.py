"""What the tests of the cohort stack's C ABI entry points share (tests/test_*_abi_cpu.py): where the header is, which ``oai_*`` names it
declares, the three checks of a new symbol, the check of a refusal, and the check of the package-level re-exports.  No tests and no
fixtures: each of those files keeps its own names, its own words and its own argument checks."""
import ctypes as C
import functools
import os
import re

from oai_analysis_2_amd import _lib, build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIG = 1 << 30                                                             # a workspace size no argument check can find too small


@functools.lru_cache(maxsize=None)
def header():
    """(the raw text of include/oai_hip.h, the ``oai_*`` names it declares outside its comments)."""
    raw = open(os.path.join(ROOT, "include", "oai_hip.h"), encoding="utf-8").read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    return raw, frozenset(re.findall(r"\b(oai_[a-z0-9_]+)\s*\(", text))


def check_symbols(names):
    """Every name is declared in the header, exported by the built library and bound in ``_lib.SIGNATURES``; returns the header's text."""
    raw, declared = header()
    lib = C.CDLL(build.build_library(verbose=False))
    for name in names:
        assert name in declared, f"{name} is not declared in include/oai_hip.h"
        assert hasattr(lib, name), f"{name} declared in include/oai_hip.h but not exported"
        assert name in _lib.SIGNATURES
    return raw


def section(raw, title):
    """The header from ``title`` on."""
    return raw[raw.index(title):]


def refused(lib, rc, *words):
    """The call failed, and the library's message holds every one of ``words``."""
    msg = lib.oai_last_error()
    assert rc != 0 and all(w in msg for w in words), (rc, msg)


def check_reexported(names):
    """The package exports each name, and it is the object that ``stats`` holds."""
    import oai_analysis_2_amd as pkg
    from oai_analysis_2_amd import stats
    for name in names:
        assert getattr(pkg, name) is getattr(stats, name)
