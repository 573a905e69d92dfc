"""The C-ABI library loads and exports every symbol include/cwt.h (the drop-in boundary) and
include/cwt_debug.h (test / measurement hooks) declare (no GPU needed), the ctypes prototypes
cover exactly that set, and the boundary header holds no debug hook."""
import os
import re

import pytest

from few_shot_seg_cwt_amd import _lib, build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header_functions(names=("cwt.h", "cwt_debug.h")):
    fns = set()
    for n in names:
        src = open(os.path.join(ROOT, "include", n)).read()
        src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
        fns |= set(re.findall(r"\b(cwt_[a-z0-9_]+)\s*\(", src))
    return sorted(fns)


def test_boundary_header_has_no_debug_hooks():
    boundary = header_functions(("cwt.h",))
    assert not [f for f in boundary if f.startswith("cwt_debug_") or "masked" in f], boundary
    assert set(header_functions(("cwt_debug.h",))).isdisjoint(boundary)


@pytest.fixture(scope="module")
def lib():
    build.build(verbose=False)
    return _lib.load_library()


def test_header_declares_functions():
    fns = header_functions()
    assert "cwt_extract_features" in fns and "cwt_inner_adapt" in fns and "cwt_attention_fwd" in fns
    assert len(fns) >= 20


def test_library_exports_every_header_symbol(lib):
    for fn in header_functions():
        assert hasattr(lib, fn), fn


def test_ctypes_prototypes_match_header():
    assert sorted(_lib.SIGNATURES) == header_functions()


def test_version_and_error_calls_without_gpu(lib):
    assert b"gfx950" in lib.cwt_version()
    assert lib.cwt_last_error() is not None
    # argument validation happens before any device call
    assert lib.cwt_extract_features(None, None, None, 1, 473, None, None) == 1001
    assert b"ctx" in lib.cwt_last_error()
    assert lib.cwt_attention_saved_floats(1, 3600, 512, 4) > 0


def test_code_object_targets_gfx950():
    so = open(_lib.LIB_PATH, "rb").read()
    assert b"gfx950" in so


C_PROGRAM = r"""
#include <stdio.h>
#include <string.h>
#include "cwt.h"
#include "cwt_debug.h"
int main(void) {
  const char* v = cwt_version();
  if (!v || !strstr(v, "gfx950")) return 2;
  /* argument validation precedes any device call: no GPU needed */
  if (cwt_extract_features(NULL, NULL, NULL, 1, 473, NULL, NULL) != 1001) return 3;
  if (!strstr(cwt_last_error(), "ctx")) return 4;
  if (cwt_attention_saved_floats(1, 3600, 512, 4) == 0) return 5;
  printf("ok %s\n", v);
  return 0;
}
"""


def test_header_is_plain_c_and_links(lib, tmp_path):
    """include/cwt.h compiles as C99 (no C++ or torch types in the signatures) and a C program
    links against libcwt.so and calls it -- the boundary a cgo / JNI / N-API stub would bind."""
    import shutil
    import subprocess
    if shutil.which("gcc") is None:
        pytest.skip("gcc not available")
    src = tmp_path / "abi.c"
    src.write_text(C_PROGRAM)
    exe = tmp_path / "abi"
    libdir = os.path.dirname(_lib.LIB_PATH)
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src),
                        "-L", libdir, "-lcwt", f"-Wl,-rpath,{libdir}", "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    env = dict(os.environ, LD_LIBRARY_PATH="/opt/rocm/lib:" + os.environ.get("LD_LIBRARY_PATH", ""))
    r = subprocess.run([str(exe)], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0 and r.stdout.startswith("ok"), (r.returncode, r.stdout, r.stderr)


def test_library_provenance_is_the_tree(lib):
    """The library's compiled-in source hash is the tree's (build.source_hash), and a library
    whose hash differs is refused at load instead of being run (build provenance)."""
    from few_shot_seg_cwt_amd import _lib as L
    assert build.built_hash() == build.source_hash()
    assert lib.cwt_version().decode().endswith("src=" + build.source_hash())
    with pytest.raises(L.CwtError, match="stale"):
        L.check_provenance("libcwt 0.2 (gfx950) src=0000000000000000", "libcwt.so")


def test_build_lists_cover_every_source_file():
    """Every .hip / .h / .inc under csrc/ is in build.SOURCES or build.HEADERS, and nothing else is: a
    file missing from the lists would be left out of source_hash, and a stale library would load."""
    listed = build.SOURCES + build.HEADERS
    assert len(set(listed)) == len(listed), sorted(f for f in set(listed) if listed.count(f) > 1)
    on_disk = {f for f in os.listdir(build.CSRC) if f.endswith((".hip", ".h", ".inc"))}
    assert on_disk == set(listed), (sorted(on_disk - set(listed)), sorted(set(listed) - on_disk))
