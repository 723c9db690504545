"""Rendering modes 5 (depth complexity) and 9 (depth peeling) without a GPU: the header defines the modes, documents the options and
declares the entry points in C99, the libraries export them, the Python layers bind them and the host plugins forward their keys."""
import os
import re
import subprocess

from linevis_amd import build as lv_build, capi, host_api

ENTRY_POINTS = {"lv_depth_complexity_get_buffers", "lv_depth_complexity_get_stats", "lv_depth_peeling_get_buffers",
                "lv_depth_peeling_resolve_buffers"}


def _exports(lib):
    out = subprocess.check_output(["nm", "-D", "--defined-only", lib], text=True)
    return {line.split()[-1] for line in out.splitlines() if line.strip()}


def test_header_defines_the_modes_and_declares_the_entry_points(tmp_path):
    text = open(capi.HEADER_PATH).read()
    assert re.search(r"#define LV_RENDERING_MODE_DEPTH_COMPLEXITY 5\b", text)
    assert re.search(r"#define LV_RENDERING_MODE_DEPTH_PEELING 9\b", text)
    for name in ENTRY_POINTS:
        assert "int %s(" % name in text, name
    for word in ("depth_peeling_max_layers", "depth_complexity_max_colour", "DepthPeelingGather.glsl", "DepthComplexityResolve.glsl",
                 "FRONT_TO_BACK_PREMUL_ALPHA", "BACK_TO_FRONT_PREMUL_ALPHA", "2000", "only an explicit value"):
        assert word in text, word
    src = tmp_path / "peel.c"
    src.write_text('#include <stddef.h>\n#include "linevis_hip.h"\n'
                   'int all(lv_ctx* ctx, const uint32_t* entries, const uint64_t* off, uint8_t* out, float* accum, uint32_t* words) {\n'
                   '  lv_depth_complexity_stats s;\n'
                   '  int rc = lv_set_option(ctx, "depth_peeling_max_layers", "3");\n'
                   '  if (rc) return rc;\n'
                   '  rc = lv_set_option(ctx, "depth_complexity_max_colour", "0");\n'
                   '  if (rc) return rc;\n'
                   '  rc = lv_depth_peeling_resolve_buffers(ctx, entries, 3u, off, 2u, 1u, out, NULL, NULL);\n'
                   '  if (rc) return rc;\n'
                   '  rc = lv_render(ctx, LV_RENDERING_MODE_DEPTH_PEELING, 0u, 0u, 2u, 1u, out);\n'
                   '  if (rc) return rc;\n'
                   '  rc = lv_depth_peeling_get_buffers(ctx, accum, words, words + 2, 2u);\n'
                   '  if (rc) return rc;\n'
                   '  rc = lv_render(ctx, LV_RENDERING_MODE_DEPTH_COMPLEXITY, 0u, 0u, 2u, 1u, out);\n'
                   '  if (rc) return rc;\n'
                   '  rc = lv_depth_complexity_get_buffers(ctx, words, 2u);\n'
                   '  if (rc) return rc;\n'
                   '  rc = lv_depth_complexity_get_stats(ctx, &s);\n'
                   '  return rc ? rc : (int)(s.total + s.used_locations + s.max + s.min + s.buffer_size);\n'
                   '}\n')
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-c", "-I", os.path.dirname(capi.HEADER_PATH),
                           str(src), "-o", str(tmp_path / "peel.o")])
    assert capi.MODE_DEPTH_COMPLEXITY == 5 and capi.MODE_DEPTH_PEELING == 9
    assert ENTRY_POINTS <= set(capi.SYMBOLS)


def test_unsupported_mode_message_lists_the_modes():
    text = open(os.path.join(lv_build.CSRC, "lv_render.hip")).read()
    message = text[text.index('"unsupported rendering mode %d'):]
    message = message[:message.index("mode);")]
    assert "5 = depth complexity" in message and "9 = depth peeling" in message


def test_option_keys_are_parsed():
    text = open(os.path.join(lv_build.CSRC, "lv_api.hip")).read()
    assert 'k == "depth_peeling_max_layers"' in text and 'k == "depth_complexity_max_colour"' in text


def test_libraries_export_the_new_symbols():
    assert ENTRY_POINTS <= _exports(lv_build.LIB)
    host = lv_build.build_host()
    assert {"lvh_renderer_depth_peeling_state", "lvh_renderer_depth_complexity_state"} <= _exports(host)
    assert hasattr(host_api.HeadlessLineRenderer, "depth_peeling_state") and hasattr(host_api.HeadlessLineRenderer, "depth_complexity_state")
    for name in ("depth_complexity_buffers", "depth_complexity_stats", "depth_peeling_buffers", "depth_peeling_resolve"):
        assert hasattr(capi.Context, name), name


def test_host_plugins_forward_the_keys():
    """HipDepthPeelingRenderer / HipDepthComplexityRenderer: their key and the PPLL tile / fragment keys to the C ABI, modes 9 and 5
    from the factory.  Without a GPU no plugin can be created, so this reads the source and is only a smoke check; what the plugins do
    with the keys is tested on the GPU (test_host_plugin of test_gpu_depth_peeling.py and test_gpu_depth_complexity.py)."""
    host = os.path.join(os.path.dirname(lv_build.__file__), "host")
    text = open(os.path.join(host, "LineRenderer.cpp")).read()
    hpp = open(os.path.join(host, "LineRenderer.hpp")).read()
    factory = open(os.path.join(host, "HeadlessLineRenderer.cpp")).read()
    for cls, key, member, mode, number in (("HipDepthPeelingRenderer", "depth_peeling_max_layers", "maxLayers", "DEPTH_PEELING", 9),
                                           ("HipDepthComplexityRenderer", "depth_complexity_max_colour", "maxColour", "DEPTH_COMPLEXITY", 5)):
        body = text[text.index("void %s::setNewState" % cls):]
        assert 'setOption("%s", std::to_string(%s))' % (key, member) in body
        assert "renderMode(LV_RENDERING_MODE_%s)" % mode in body
        for k in (key, "ppll_tile_width", "ppll_tile_height", "ppll_fragment_source", "ppll_fragment_colour", "ppll_prism_rasteriser"):
            assert '"%s"' % k in body[body.index("::setNewSettings"):], k
        assert re.search(r"RENDERING_MODE_%s = %d\b" % (mode, number), hpp)
        assert "new %s(" % cls in factory


def test_cli_offers_the_modes_by_the_reference_names():
    from linevis_amd import __main__ as cli
    text = open(cli.__file__).read()
    assert '"Depth Peeling": capi.MODE_DEPTH_PEELING' in text and '"Depth Complexity Renderer": capi.MODE_DEPTH_COMPLEXITY' in text
