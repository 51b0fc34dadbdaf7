"""What holds for every native library alike, checked once over ``_lib.LIBRARIES`` without a GPU: the header, the binding's
record and the built file name the same entry points and no other library's, the ABI version, a missing file is an error,
and the build knows each library's sources, version script and headers."""
import os
import re
import shutil
import subprocess

import pytest

from cough_detector_amd import _lib
from cough_detector_amd import build as cbuild

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("amd", "loop", "data", "segments", "score", "draws", "soft", "warp", "pitch")
COUNTS = dict(zip(NAMES, (53, 3, 5, 6, 5, 5, 6, 5, 4)))
# beside its own sources, version script and header: the shared headers and sources a library compiles
ALSO_COMPILES = {"amd": (), "loop": ("train_common.h",), "data": (), "segments": (), "score": (),
                 "draws": ("augment_kernel.h", "philox.h"), "soft": ("train_common.h", "train_std.hip"),
                 "warp": ("philox.h",), "pitch": ("cough_amd_warp.h", "philox.h")}


def _tag(name):
    return "" if name == "amd" else "_" + name


def _header(name):
    return open(os.path.join(ROOT, "include", f"cough_amd{_tag(name)}.h")).read()


def _exported(path):
    # binutils' nm, or the llvm-nm that ships next to hipcc
    nm = shutil.which("nm") or os.path.join(os.path.dirname(os.path.realpath(cbuild._hipcc())), "..", "lib", "llvm", "bin", "llvm-nm")
    out = subprocess.run([nm, "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    return {line.split()[-1] for line in out.splitlines() if line.strip()}


def _module_name(name, what):
    """The module-level name of a record's ``load`` / ``check`` / ``SYMBOLS`` / ``LIB_PATH``: bare for the main library."""
    if name == "amd":
        return what
    return f"{what}_{name}" if what.islower() else f"{name.upper()}_{what}"


def test_the_table_lists_the_nine_libraries_in_order():
    assert tuple(_lib.LIBRARIES) == tuple(cbuild.UNITS) == tuple(cbuild.LIBS) == NAMES


@pytest.mark.parametrize("name", NAMES)
def test_header_record_and_file_name_the_same_entry_points(name):
    rec, text = _lib.LIBRARIES[name], _header(name)
    declared = set(re.findall(r"^(?:int|size_t|const char\*|void) (cough_[a-z_0-9]+)\s*\(", text, flags=re.M))
    assert declared == set(rec.symbols) == set(rec.prototypes), declared ^ set(rec.symbols)
    assert len(rec.symbols) == len(set(rec.symbols)) == COUNTS[name]
    assert rec.symbols[0] == rec.abi_symbol == f"cough_{name}_abi_version" and rec.error_symbol == f"cough_{name}_last_error"
    assert rec.error_symbol in rec.symbols[1:3]
    assert os.path.basename(rec.path) == rec.soname == f"libcough_amd{_tag(name)}.so"
    assert _exported(rec.path) == declared, sorted(_exported(rec.path) ^ declared)
    # the module-level names are this record
    assert getattr(_lib, _module_name(name, "SYMBOLS")) is rec.symbols and getattr(_lib, _module_name(name, "LIB_PATH")) == rec.path
    assert getattr(_lib, _module_name(name, "load")) == rec.load and getattr(_lib, _module_name(name, "check")) == rec.check
    lib = rec.load()
    for s in rec.symbols:
        assert hasattr(lib, s), s
    assert getattr(lib, rec.abi_symbol)() == rec.abi == (5 if name == "amd" else 1)
    assert f"#define COUGH_{name.upper()}_ABI_VERSION {rec.abi}\n" in text
    assert isinstance(getattr(lib, rec.error_symbol)(), bytes)
    # no other library binds or exports one of them, and no header written before this one so much as mentions them
    for other in NAMES:
        if other != name:
            assert not declared & set(_lib.LIBRARIES[other].symbols), other
            for s in declared:
                assert not hasattr(_lib.LIBRARIES[other].load(), s), (other, s)
    for earlier in NAMES[:NAMES.index(name)]:
        text = _header(earlier)
        for s in declared:
            assert s not in text, (earlier, s)


@pytest.mark.parametrize("name", NAMES)
def test_a_missing_library_is_an_error(name, monkeypatch):
    rec = _lib.LIBRARIES[name]
    monkeypatch.setattr(rec, "handle", None)
    monkeypatch.setattr(rec, "path", os.path.join(ROOT, "no_such_dir", rec.soname))
    with pytest.raises(RuntimeError, match=r"is missing: the HIP extension is not built\. Run `python -m cough_detector_amd\.build`"):
        getattr(_lib, _module_name(name, "load"))()


@pytest.mark.parametrize("name", NAMES)
def test_the_build_covers_the_library(name, monkeypatch):
    sources = tuple(u if isinstance(u, str) else u[0] for u in cbuild.UNITS[name])
    assert len(cbuild.SOURCES) == 12 and cbuild.UNITS["amd"] is cbuild.SOURCES and cbuild.LIB == cbuild.LIBS["amd"]
    assert cbuild.SOFT_SHARED_SOURCES == ("train.hip", "train_small.hip", "train_std.hip")
    assert set(cbuild.SOFT_SHARED_SOURCES) <= set(cbuild.SOURCES)         # the step code exists once
    if name == "soft":
        assert cbuild.UNITS[name] == ("soft.hip",) + tuple((s, cbuild.SOFT_FLAGS, "_soft") for s in cbuild.SOFT_SHARED_SOURCES)
    elif name != "amd":
        assert cbuild.UNITS[name] == (name + ".hip",) and name + ".hip" not in cbuild.SOURCES
    assert os.path.basename(cbuild.LIBS[name]) == f"libcough_amd{_tag(name)}.so" == _lib.LIBRARIES[name].soname
    assert os.path.dirname(cbuild.LIBS[name]) == os.path.dirname(cbuild.LIB) and os.path.exists(cbuild.LIBS[name])
    own = sources + (f"exports{_tag(name)}.map",)
    for s in own + tuple(s for s in ALSO_COMPILES[name] if not s.startswith("cough_amd")):
        assert os.path.exists(os.path.join(cbuild.CSRC, s)), s
    # the staleness check: every file at time 1 is up to date; a source, version script or header at time 2 is not
    newer = []
    monkeypatch.setattr(cbuild.os.path, "getmtime", lambda p: 2.0 if os.path.basename(p) in newer else 1.0)
    assert not cbuild.is_stale()
    for dep in own + (f"cough_amd{_tag(name)}.h", "common.h", "build.py") + ALSO_COMPILES[name]:
        newer[:] = [dep]
        assert cbuild.is_stale(), dep
    newer[:] = []
    assert not cbuild.is_stale()
    monkeypatch.setitem(cbuild.LIBS, name, os.path.join(ROOT, "no_such_dir", f"libcough_amd{_tag(name)}.so"))
    assert cbuild.is_stale()
