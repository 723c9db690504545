"""Rendering mode 3 (MLAB) without a GPU: the header defines the mode and declares lv_mlab_resolve_buffers in C99, the HIP library
and the host layer export the new entry points, and the host layer lists the reference's four MLAB states apart from getTestModes."""
import os
import re
import subprocess

from linevis_amd import build as lv_build, capi, host_api


def _exports(lib):
    out = subprocess.check_output(["nm", "-D", "--defined-only", lib], text=True)
    return {line.split()[-1] for line in out.splitlines() if line.strip()}


def test_header_defines_mode_3_and_declares_the_fold_entry_point(tmp_path):
    text = open(capi.HEADER_PATH).read()
    assert re.search(r"#define LV_RENDERING_MODE_MLAB 3\b", text)
    assert "int lv_mlab_resolve_buffers(" in text
    assert "mlab_num_layers" in text
    src = tmp_path / "mlab.c"
    src.write_text('#include <stddef.h>\n#include "linevis_hip.h"\n'
                   'int fold(lv_ctx* ctx, const uint32_t* e, const uint64_t* off, uint8_t* out) {\n'
                   '  int m = LV_RENDERING_MODE_MLAB;\n'
                   '  (void)m;\n'
                   '  return lv_mlab_resolve_buffers(ctx, e, 3u, off, 2u, 1u, out);\n'
                   '}\n')
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-c", "-I", os.path.dirname(capi.HEADER_PATH),
                           str(src), "-o", str(tmp_path / "mlab.o")])
    assert capi.MODE_MLAB == 3
    assert "lv_mlab_resolve_buffers" in capi.SYMBOLS


def test_libraries_export_the_new_symbols():
    assert "lv_mlab_resolve_buffers" in _exports(lv_build.LIB)
    host = lv_build.build_host()
    assert {"lvh_test_modes_mlab_count", "lvh_test_mode_mlab", "lvh_renderer_mlab_state"} <= _exports(host)


def test_mlab_test_modes_are_the_reference_states_and_not_in_get_test_modes():
    states = host_api.get_test_modes_mlab()
    assert [s[0] for s in states] == ["MLAB (No Sync)", "MLAB (Spinlock)", "MLAB (Unordered Interlock)", "MLAB (Ordered Interlock)"]
    assert all(s[1] == 3 for s in states)
    assert [s[3] for s in states] == [{"syncMode": "0"}, {"syncMode": "2"},
                                     {"syncMode": "1", "useOrderedFragmentShaderInterlock": "false"},
                                     {"syncMode": "1", "useOrderedFragmentShaderInterlock": "true"}]
    assert all(m[1] != 3 for m in host_api.get_test_modes(True))


def test_cli_offers_the_mlab_mode():
    from linevis_amd import __main__ as cli
    text = open(cli.__file__).read()
    assert '"mlab": capi.MODE_MLAB' in text
