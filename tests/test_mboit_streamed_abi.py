"""mboit_fragment_storage = streamed without a GPU: the header documents the option and declares lv_mboit_get_moments in C99, the
library exports it, capi.py binds it, and the host layer passes the key through its settings."""
import os
import re
import subprocess

from linevis_amd import build as lv_build, capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_names_the_option_and_declares_the_read_back(tmp_path):
    text = open(capi.HEADER_PATH).read()
    assert "mboit_fragment_storage" in text and '"pool"' in text and '"streamed"' in text
    assert re.search(r"int lv_mboit_get_moments\(lv_ctx\* ctx, float\* out, uint64_t capacity_floats\);", text)
    for word in ("131071", "ppll_expected_avg_depth_complexity", "LV_KERNEL_PPLL_RASTER"):
        assert word in text, word
    src = tmp_path / "streamed.c"
    src.write_text('#include <stddef.h>\n#include "linevis_hip.h"\n'
                   'typedef int (*get_moments_fn)(lv_ctx*, float*, uint64_t);\n'
                   'get_moments_fn address(void) { return &lv_mboit_get_moments; }\n'
                   'int moments(lv_ctx* ctx, float* out) {\n'
                   '  if (lv_set_option(ctx, "mboit_fragment_storage", "streamed") != LV_OK) return LV_E_INVALID;\n'
                   '  return lv_mboit_get_moments(ctx, out, (uint64_t)5u);\n'
                   '}\n')
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-c", "-I", os.path.dirname(capi.HEADER_PATH),
                           str(src), "-o", str(tmp_path / "streamed.o")])


def test_library_exports_and_capi_binds_the_read_back():
    out = subprocess.check_output(["nm", "-D", "--defined-only", lv_build.LIB], text=True)
    assert "lv_mboit_get_moments" in {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert "lv_mboit_get_moments" in capi.SYMBOLS
    L = capi.load()
    assert L.lv_mboit_get_moments.argtypes is not None and len(L.lv_mboit_get_moments.argtypes) == 3
    assert callable(capi.Context.mboit_moments)


def test_host_layer_passes_the_key_through():
    text = open(os.path.join(ROOT, "linevis_amd", "host", "LineRenderer.cpp")).read()
    body = text[text.index("bool HipMBOITRenderer::setNewSettings"):]
    body = body[:body.index("\n}\n")]
    assert '"mboit_moment_bias", "mboit_fragment_storage"' in body
    state = text[text.index("void HipMBOITRenderer::setNewState"):text.index("void HipMBOITRenderer::render")]
    assert "mboit_fragment_storage" not in state   # the reference's states do not carry the key


def test_probe_offers_the_storage_option():
    text = open(os.path.join(ROOT, "tools", "probe_mboit.py")).read()
    assert "mboit_fragment_storage" in text and "mboit_c4_streamed.json" in text
