"""Node-wide SVGF's entry points (docs/MGPU_SVGF.md): declared in the header, listed in the binding, exported by the built library;
the display tail keeps no node-wide form.  No GPU."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MGPU_SVGF_SYMBOLS = ("atn_mgpu_svgf_render", "atn_mgpu_svgf_set_motion_depth", "atn_mgpu_svgf_reset", "atn_mgpu_svgf_set_atrous_iterations",
                     "atn_mgpu_svgf_set_dilate_temporal_weight", "atn_mgpu_svgf_download", "atn_mgpu_svgf_output_device")


def _exported():
    so = os.environ.get("ATEN_AMD_LIB") or os.path.join(ROOT, "aten_amd", "libaten_amd.so")
    out = subprocess.check_output(["nm", "-D", "--defined-only", so]).decode()
    return {l.split()[-1] for l in out.splitlines() if l.strip()}


def test_the_seven_entry_points_are_declared_listed_and_exported():
    from aten_amd import _lib
    header = open(os.path.join(ROOT, "include", "aten_amd.h")).read()
    names = _exported()
    for s in MGPU_SVGF_SYMBOLS:
        ret = "void*" if s.endswith("_device") else "int"
        assert "%s %s(atn_mgpu* mg" % (ret, s) in header, s
        assert s in _lib.SYMBOLS, s
        assert s in names, s
    assert len(set(MGPU_SVGF_SYMBOLS)) == 7


def test_the_display_tail_has_no_node_wide_form():
    from aten_amd import _lib
    assert not [n for n in _exported() if n.startswith("atn_mgpu_taa")]
    assert not [n for n in _lib.SYMBOLS if n.startswith("atn_mgpu_taa")]


def test_the_exchange_kernels_have_kernel_time_ids_behind_the_single_context_ones():
    """ATN_K_COUNT -- the length of the arrays a caller hands to atn_get_kernel_times -- stays what it was; the exchange's two
    classes follow it and are reported by atn_mgpu_get_kernel_times only."""
    from aten_amd import _lib
    header = open(os.path.join(ROOT, "include", "aten_amd.h")).read()
    assert "ATN_K_COUNT = 11," in header
    assert "ATN_K_SVGF_PACK = 11, ATN_K_SVGF_UNPACK = 12" in header and "ATN_K_MGPU_COUNT = 13" in header
    assert len(_lib.K_NAMES) == 11
    assert _lib.MGPU_K_NAMES[:11] == _lib.K_NAMES and _lib.MGPU_K_NAMES[11:] == ["svgf_pack", "svgf_unpack"]
