"""The spatial-hashing denoiser's C-ABI without a GPU: the header declares the four entry points in C99 and documents the option keys
and the rules the build owns, the HIP library exports the symbols and the Python binding knows them."""
import os
import re
import subprocess

from linevis_amd import build as lv_build, capi

ENTRY_POINTS = ("lv_spatial_hashing_denoise_buffers", "lv_spatial_hashing_reset", "lv_spatial_hashing_get_cells",
                "lv_spatial_hashing_get_stats")
KEYS = ("spatial_hashing_s_p", "spatial_hashing_s_min_exp", "spatial_hashing_s_nd", "spatial_hashing_num_cells",
        "spatial_hashing_atomics_mode")


def test_header_declares_the_entry_points_and_documents_the_keys(tmp_path):
    text = open(capi.HEADER_PATH).read()
    flat = " ".join(re.sub(r"\n \*", " ", text).split())     # comment text without the line leaders
    for name in ENTRY_POINTS:
        assert "int %s(" % name in text, name
        assert name in capi.SYMBOLS, name
    for key in KEYS:
        assert key in flat, key
    assert '"SVGF" | "Spatial Hashing"' in flat
    for rule in ("Uint Quantized Atomic Add", "No Atomics", "dropped and counted (no eviction)", "more than half of its cells are occupied",
                 "2^28", "lv_spatial_hashing_reset", "(checksum << 32) | hash", "(sum << 28) | count"):
        assert rule in flat, rule
    for name, number in (("LV_KERNEL_SH_WRITE", 9), ("LV_KERNEL_SH_READ", 10), ("LV_KERNEL_SH_TAIL", 11)):
        assert re.search(r"#define %s %d\b" % (name, number), text)
        assert getattr(capi, name[3:]) == number
    src = tmp_path / "sh.c"
    src.write_text('#include <stddef.h>\n#include "linevis_hip.h"\n'
                   'int denoise(lv_ctx* ctx, const float* noisy, const float* n, const float* p, const float* cam, float* rd, float* out) {\n'
                   '  uint64_t stats[4], count = 0;\n'
                   '  int rc = lv_spatial_hashing_denoise_buffers(ctx, 24u, 16u, noisy, n, p, cam, rd, out);\n'
                   '  if (!rc) rc = lv_spatial_hashing_get_stats(ctx, 1, stats);\n'
                   '  if (!rc) rc = lv_spatial_hashing_get_cells(ctx, 1, NULL, NULL, 0, &count);\n'
                   '  if (!rc) rc = lv_spatial_hashing_reset(ctx, 1);\n'
                   '  return rc ? rc : LV_KERNEL_SH_WRITE + LV_KERNEL_SH_READ + LV_KERNEL_SH_TAIL;\n'
                   '}\n')
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-c", "-I", os.path.dirname(capi.HEADER_PATH),
                           str(src), "-o", str(tmp_path / "sh.o")])


def test_library_exports_the_symbols():
    out = subprocess.check_output(["nm", "-D", "--defined-only", lv_build.LIB], text=True)
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    for name in ENTRY_POINTS:
        assert name in exported, name


def test_python_binding_has_the_wrappers():
    for method in ("spatial_hashing_denoise", "spatial_hashing_reset", "spatial_hashing_cells", "spatial_hashing_stats"):
        assert callable(getattr(capi.Context, method))
