"""Rendering mode 10 (Atomic Loop 64) without a GPU: the header defines the mode, documents the option and declares the two entry
points in C99, the libraries export them, the Python layers bind them and the host plugin forwards its keys."""
import os
import re
import subprocess

from linevis_amd import build as lv_build, capi, host_api


def _exports(lib):
    out = subprocess.check_output(["nm", "-D", "--defined-only", lib], text=True)
    return {line.split()[-1] for line in out.splitlines() if line.strip()}


def test_header_defines_mode_10_and_declares_the_entry_points(tmp_path):
    text = open(capi.HEADER_PATH).read()
    assert re.search(r"#define LV_RENDERING_MODE_ATOMIC_LOOP_64 10\b", text)
    assert "int lv_atomic_loop_get_buffers(" in text and "int lv_atomic_loop_resolve_buffers(" in text
    assert "int lv_atomic_loop_get_num_layers(" in text
    assert "atomic_loop_num_layers" in text and "AtomicLoop64Gather.glsl" in text
    src = tmp_path / "al64.c"
    src.write_text('#include <stddef.h>\n#include "linevis_hip.h"\n'
                   'int both(lv_ctx* ctx, const uint64_t* keys, const uint64_t* off, uint8_t* out, uint64_t* slots, uint64_t* tail) {\n'
                   '  int rc = lv_set_option(ctx, "atomic_loop_num_layers", "4");\n'
                   '  if (rc) return rc;\n'
                   '  rc = lv_atomic_loop_resolve_buffers(ctx, keys, 3u, off, 2u, 1u, out, NULL, NULL);\n'
                   '  if (rc) return rc;\n'
                   '  rc = lv_render(ctx, LV_RENDERING_MODE_ATOMIC_LOOP_64, 0u, 0u, 2u, 1u, out);\n'
                   '  if (rc) return rc;\n'
                   '  return lv_atomic_loop_get_buffers(ctx, slots, tail, 2u);\n'
                   '}\n')
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-c", "-I", os.path.dirname(capi.HEADER_PATH),
                           str(src), "-o", str(tmp_path / "al64.o")])
    assert capi.MODE_ATOMIC_LOOP_64 == 10
    assert {"lv_atomic_loop_get_buffers", "lv_atomic_loop_resolve_buffers"} <= set(capi.SYMBOLS)


def test_libraries_export_the_new_symbols():
    assert {"lv_atomic_loop_get_buffers", "lv_atomic_loop_resolve_buffers", "lv_atomic_loop_get_num_layers"} <= _exports(lv_build.LIB)
    host = lv_build.build_host()
    assert "lvh_renderer_atomic_loop_state" in _exports(host)
    assert hasattr(host_api.HeadlessLineRenderer, "atomic_loop_state")
    assert hasattr(capi.Context, "atomic_loop_buffers") and hasattr(capi.Context, "atomic_loop_resolve")


def test_host_plugin_forwards_the_keys():
    """HipAtomicLoop64Renderer: numLayers from the state and the settings, atomic_loop_num_layers and the PPLL tile / fragment keys
    to the C ABI, mode 10 from the factory.  Without a GPU no plugin can be created, so this reads the source and is only a
    smoke check; what the plugin does with the keys is tested on the GPU (test_gpu_atomic_loop.py, test_host_plugin)."""
    host = os.path.join(os.path.dirname(lv_build.__file__), "host")
    text = open(os.path.join(host, "LineRenderer.cpp")).read()
    body = text[text.index("void HipAtomicLoop64Renderer::setNewState"):text.index("void HipPerPixelLinkedListLineRenderer::computeStatistics")]
    assert 'getValueOpt("numLayers", numLayers)' in body
    assert 'setOption("atomic_loop_num_layers", std::to_string(numLayers))' in body
    assert "renderMode(LV_RENDERING_MODE_ATOMIC_LOOP_64)" in body
    for key in ("atomic_loop_num_layers", "ppll_tile_width", "ppll_tile_height", "ppll_fragment_source", "ppll_fragment_colour",
                "ppll_prism_rasteriser"):
        assert '"%s"' % key in body[body.index("::setNewSettings"):], key
    assert re.search(r"RENDERING_MODE_ATOMIC_LOOP_64 = 10\b", open(os.path.join(host, "LineRenderer.hpp")).read())
    factory = open(os.path.join(host, "HeadlessLineRenderer.cpp")).read()
    assert "new HipAtomicLoop64Renderer(" in factory


def test_cli_offers_the_mode():
    from linevis_amd import __main__ as cli
    assert '"al64": capi.MODE_ATOMIC_LOOP_64' in open(cli.__file__).read()
