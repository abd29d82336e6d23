"""DevScene::shadow_plain without a GPU (docs/TRACE_RAY_COST.md): the decision function of csrc/host/scene_upload.hpp for the light
lists a scene can have, and that a light edit decides it again (tests/cxx/shadow_plain_host_test.cpp, also under the host
sanitizers)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _build_host_test(exe, extra=()):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    lib_dir = os.path.join(ROOT, "aten_amd")
    from aten_amd._hostlib import hostlib
    hostlib()                                                           # (builds libaten_amd_scene.so if it is missing)
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-std=c++17", "-O1", "-w", "-I", os.path.join(ROOT, "include")] + list(extra)
                          + [os.path.join(ROOT, "tests", "cxx", "shadow_plain_host_test.cpp"), "-L", lib_dir, "-laten_amd_scene",
                             "-Wl,-rpath," + lib_dir, "-o", exe])


@pytest.mark.parametrize("sanitized", [False, True], ids=["plain", "asan_ubsan"])
def test_host_decision_of_the_plain_shadow_flag(tmp_path, sanitized):
    """Empty, IBL only, directional only, IBL + point, an area light with and without an object, the attribute on an area light; an
    edit of the lights decides again and a refused edit changes nothing.  Once more as a stand-alone program under
    -fsanitize=address,undefined (host code only, on the CPU)."""
    exe = str(tmp_path / "shadow_plain_host_test")
    flags = ["-g", "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined"] if sanitized else []
    _build_host_test(exe, flags)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stdout + out.stderr
