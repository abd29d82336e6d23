"""Scene edits without a GPU (docs/SCENE_EDITS.md): the eight entry points exist where a caller looks for them, and the host half of
an edit -- the derivation functions of csrc/host/scene_upload.hpp, which atn_upload_scene and the edit calls share -- leaves the state
a fresh upload of the edited description gives (tests/cxx/scene_edit_host_test.cpp, also under the host sanitizers)."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

EDIT_SYMBOLS = ["atn_update_materials", "atn_update_lights", "atn_update_texture", "atn_update_rendering_config",
                "atn_mgpu_update_materials", "atn_mgpu_update_lights", "atn_mgpu_update_texture", "atn_mgpu_update_rendering_config"]


def test_edit_symbols_in_header_binding_and_library():
    """Every edit entry point is declared in include/aten_amd.h, listed in _lib.SYMBOLS (build() checks that list against the
    library) and exported by the built libaten_amd.so."""
    from aten_amd import build
    from aten_amd._lib import SYMBOLS
    header = open(os.path.join(ROOT, "include", "aten_amd.h")).read()
    for s in EDIT_SYMBOLS:
        assert re.search(r"\bint %s\(atn_(ctx|mgpu)\*" % s, header), s
        assert s in SYMBOLS, s
    nm =shutil.which("nm") or shutil.which("llvm-nm") or "/opt/rocm/llvm/bin/llvm-nm"
    out = subprocess.run([nm, "-D", "--defined-only", build.HIP_LIB], capture_output=True, text=True, check=True).stdout
    exported = set(line.split()[-1] for line in out.splitlines() if line.split())
    assert not [s for s in EDIT_SYMBOLS if s not in exported]


def _build_host_test(exe, extra=()):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    lib_dir = os.path.join(ROOT, "aten_amd")
    from aten_amd._hostlib import hostlib
    hostlib()                                                           # (builds libaten_amd_scene.so if it is missing)
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-std=c++17", "-O1", "-w", "-I", os.path.join(ROOT, "include")] + list(extra)
                          + [os.path.join(ROOT, "tests", "cxx", "scene_edit_host_test.cpp"), "-L", lib_dir, "-laten_amd_scene",
                             "-Wl,-rpath," + lib_dir, "-o", exe])


@pytest.mark.parametrize("sanitized", [False, True], ids=["plain", "asan_ubsan"])
def test_host_derivation_of_edits(tmp_path, sanitized):
    """tests/cxx/scene_edit_host_test.cpp: for a hand-made scene and a list of edits -- every material-set crossing, alpha through
    baseColor.w and through the albedo texture, stencil types, light type changes, an NPR target light, the config -- the state
    after the host half of the edit equals build_host_image's for the edited description (arrays byte for byte, scalars field for
    field), and a refused edit changes nothing and is refused by the upload with the same message.  Once more as a stand-alone
    program under -fsanitize=address,undefined (host code only, on the CPU)."""
    exe = str(tmp_path / "scene_edit_host_test")
    flags = ["-g", "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined"] if sanitized else []
    _build_host_test(exe, flags)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stdout + out.stderr
