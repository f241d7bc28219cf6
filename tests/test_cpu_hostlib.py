"""tests/hostlib.py's builder on a source of its own in a temporary directory: it compiles and loads, leaves an up-to-date library alone, and rebuilds
-- through a temporary name, by one rename -- when something the library depends on is newer."""
import ctypes
import os
import shutil
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hostlib                                  # noqa: E402

SOURCE = """#include "answer.h"
extern "C" int answer(void) { return ANSWER + EXTRA; }
"""


def _fresh_build(src, hdr):
    """What a new process does: no cached handle.  (A dependency that does not exist is skipped.)"""
    hostlib._LIBS.pop("hostlibtest", None)
    return hostlib.build("hostlibtest", [src], extra_flags=("-DEXTRA=0",), extra_deps=[hdr, hdr + ".missing"])


def test_build_compiles_once_and_again_when_a_dependency_is_newer(tmp_path):
    src, hdr, so = str(tmp_path / "answer.cpp"), str(tmp_path / "answer.h"), str(tmp_path / "libhostlibtest.so")
    open(src, "w").write(SOURCE)
    open(hdr, "w").write("#define ANSWER 42\n")
    try:
        L = _fresh_build(src, hdr)
        assert L.answer() == 42
        assert hostlib.build("hostlibtest", [src]) is L, "one handle per name"
        first = os.stat(so)

        assert _fresh_build(src, hdr).answer() == 42
        same = os.stat(so)
        assert (same.st_ino, same.st_mtime_ns) == (first.st_ino, first.st_mtime_ns), "nothing changed, yet the library was rebuilt"

        open(hdr, "w").write("#define ANSWER 43\n")
        os.utime(hdr, ns=(first.st_mtime_ns + 10**9, first.st_mtime_ns + 10**9))
        _fresh_build(src, hdr)
        assert os.stat(so).st_ino != first.st_ino, "a newer dependency, yet the library was not replaced by a new file"
        assert sorted(os.listdir(str(tmp_path))) == ["answer.cpp", "answer.h", "libhostlibtest.so"], "a temporary file was left behind"
        # (this process's loader answers the old path with the library it has already mapped: the new file is read through a copy)
        shutil.copy(so, so + ".copy")
        assert ctypes.CDLL(so + ".copy").answer() == 43, "the rebuilt library does not hold the new dependency"
    finally:
        hostlib._LIBS.pop("hostlibtest", None)
