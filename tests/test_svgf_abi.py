"""lv_svgf_denoise_buffers without a GPU: the header declares it in C99 and states the rules for what SVGF.glsl leaves open, the HIP
library exports it and the Python binding knows it."""
import os
import subprocess

from linevis_amd import build as lv_build, capi


def test_header_declares_the_entry_point_and_states_the_rules(tmp_path):
    text = open(capi.HEADER_PATH).read()
    assert "int lv_svgf_denoise_buffers(" in text
    doc = " ".join(text[:text.index("int lv_svgf_denoise_buffers(")].rsplit("/*", 1)[1].split())
    for rule in ("not finite or outside the int range", "never converted to int", "non-finite depth fwidth drops the depth term",
                 "fetches outside the image return 0", "return the other operand of a NaN", "LV_E_INVALID"):
        assert rule in doc, rule
    src = tmp_path / "svgf.c"
    src.write_text('#include <stddef.h>\n#include "linevis_hip.h"\n'
                   'int denoise(lv_ctx* ctx, const float* noisy, const float* nd, const float* ff, float* ch, float* mh, float* ndh,\n'
                   '            float* out) {\n'
                   '  return lv_svgf_denoise_buffers(ctx, 37u, 27u, noisy, nd, ff, ch, mh, ndh, out);\n'
                   '}\n')
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-c", "-I", os.path.dirname(capi.HEADER_PATH),
                           str(src), "-o", str(tmp_path / "svgf.o")])
    assert "lv_svgf_denoise_buffers" in capi.SYMBOLS


def test_library_exports_the_symbol():
    out = subprocess.check_output(["nm", "-D", "--defined-only", lv_build.LIB], text=True)
    assert "lv_svgf_denoise_buffers" in {line.split()[-1] for line in out.splitlines() if line.strip()}
