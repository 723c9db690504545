"""Rendering mode 6 (MBOIT) without a GPU: the header defines the mode and declares lv_mboit_resolve_buffers in C99, the HIP library
and the host layer export the new entry points, lv_stats carries the degenerate-pixel counter, and the host layer lists the
reference's ten MBOIT states apart from getTestModes."""
import ctypes as C
import os
import re
import subprocess

from linevis_amd import build as lv_build, capi, host_api


def _exports(lib):
    out = subprocess.check_output(["nm", "-D", "--defined-only", lib], text=True)
    return {line.split()[-1] for line in out.splitlines() if line.strip()}


def test_header_defines_mode_6_and_declares_the_resolve_entry_point(tmp_path):
    text = open(capi.HEADER_PATH).read()
    assert re.search(r"#define LV_RENDERING_MODE_MBOIT 6\b", text)
    assert "int lv_mboit_resolve_buffers(" in text
    for key in ("mboit_num_moments", "mboit_overestimation", "mboit_moment_bias", "mboit_use_power_moments", "mboit_pixel_format"):
        assert key in text, key
    src = tmp_path / "mboit.c"
    src.write_text('#include <stddef.h>\n#include "linevis_hip.h"\n'
                   'int resolve(lv_ctx* ctx, const uint32_t* e, const uint64_t* off, float* moments, uint8_t* out) {\n'
                   '  int m = LV_RENDERING_MODE_MBOIT;\n'
                   '  lv_stats s;\n'
                   '  s.mboit_degenerate_pixels = 0u;\n'
                   '  (void)m; (void)s;\n'
                   '  return lv_mboit_resolve_buffers(ctx, e, 3u, off, 2u, 1u, -0.5f, 1.5f, moments, out);\n'
                   '}\n')
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-c", "-I", os.path.dirname(capi.HEADER_PATH),
                           str(src), "-o", str(tmp_path / "mboit.o")])
    assert capi.MODE_MBOIT == 6
    assert "lv_mboit_resolve_buffers" in capi.SYMBOLS
    assert capi.Stats._fields_[-1] == ("mboit_degenerate_pixels", C.c_uint32)


def test_libraries_export_the_new_symbols():
    assert "lv_mboit_resolve_buffers" in _exports(lv_build.LIB)
    host = lv_build.build_host()
    assert {"lvh_test_modes_mboit_count", "lvh_test_mode_mboit", "lvh_renderer_mboit_state"} <= _exports(host)


def test_mboit_test_modes_are_the_reference_states_and_not_in_get_test_modes():
    states = host_api.get_test_modes_mboit()
    names, maps = [], []
    for n in ("4", "8"):
        names += ["MBOIT (%s Moments, %s)" % (n, v) for v in ("No Sync", "Spinlock", "Unordered Interlock", "Ordered Interlock",
                                                               "Render Targets")]
        maps += [{"numMoments": n, "syncMode": "0", "useRenderTargets": "false"},
                 {"numMoments": n, "syncMode": "2", "useRenderTargets": "false"},
                 {"numMoments": n, "syncMode": "1", "useOrderedFragmentShaderInterlock": "false", "useRenderTargets": "false"},
                 {"numMoments": n, "syncMode": "1", "useOrderedFragmentShaderInterlock": "true", "useRenderTargets": "false"},
                 {"numMoments": n, "useRenderTargets": "true"}]
    assert [s[0] for s in states] == names
    assert all(s[1] == 6 for s in states)
    assert [s[3] for s in states] == maps
    assert all(m[1] != 6 for m in host_api.get_test_modes(True))
    assert all(m[1] != 6 for m in host_api.get_test_modes_mlab())


def test_cli_offers_the_mboit_mode():
    from linevis_amd import __main__ as cli
    text = open(cli.__file__).read()
    assert '"mboit": capi.MODE_MBOIT' in text
    assert '"mboit"]' in text
