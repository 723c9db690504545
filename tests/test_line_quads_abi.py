"""The second line primitive at the boundaries, without a GPU: the option line_primitive_mode, its two values and the read-back entry
point in the header and in the binding; the header as C99; the host layer forwards the key for rendering modes 5, 8 and 10 only, and
the data set's settings path (the command line's key = value pairs) reaches LineData's line primitive mode."""
import os
import re
import subprocess

from linevis_amd import capi, host_api

SYMBOL = "lv_line_quads_get_fragments"
TUBE, QUADS = "Tube (Programmable Pull)", "Quads (Programmable Pull)"


def test_header_names_the_option_its_values_and_the_entry_point(tmp_path):
    text = open(capi.HEADER_PATH).read()
    m = re.search(r"^ \*   line_primitive_mode: ", text, flags=re.M)
    assert m
    doc = text[m.start():m.start() + 3000]
    for needle in ('"%s" (default' % TUBE, '"%s"' % QUADS, "LV_E_INVALID", "modes 2, 3, 6 and 9", "modes 1 and 11 ignore", "use_ribbons",
                   "rotating_helicity_bands", "RTAO (Prebaker)", "capsule_entry", "lbvh", "(2a, 2b, 2b + 1), (2a, 2b + 1, 2a + 1)",
                   "xc = clamp(x, -1, 1)", "sqrt(fma(-xc, xc, 1))", "((shiftSign * lineWidth) * 0.5)", "fwidth"):
        assert needle in doc, needle
    assert re.search(r"\bint %s\s*\(lv_ctx\* ctx, uint64_t capacity, uint32_t\* pixel, uint32_t\* segment, uint32_t\* triangle, "
                     r"float\* depth,\s*float\* rgba, uint64_t\* out_count\);" % SYMBOL, text)
    assert SYMBOL in capi.SYMBOLS and hasattr(capi.load(), SYMBOL)       # the library exports the symbol
    src = tmp_path / "quads.c"
    src.write_text('#include "linevis_hip.h"\n'
                   'int (*get_frags)(lv_ctx*, uint64_t, uint32_t*, uint32_t*, uint32_t*, float*, float*, uint64_t*) = %s;\n' % SYMBOL)
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-c", "-I", os.path.dirname(capi.HEADER_PATH),
                           str(src), "-o", str(tmp_path / "quads.o")])


def test_host_layer_forwards_the_key_for_modes_5_8_and_10_only():
    modes = (capi.MODE_DEFERRED, capi.MODE_PPLL, capi.MODE_MLAB, capi.MODE_DEPTH_COMPLEXITY, capi.MODE_MBOIT, capi.MODE_WBOIT,
             capi.MODE_DEPTH_PEELING, capi.MODE_ATOMIC_LOOP_64, capi.MODE_RAY_TRACER)
    assert sorted(int(m) for m in modes) == [1, 2, 3, 5, 6, 8, 9, 10, 11]
    assert [int(m) for m in modes if host_api.forwards_line_primitive_mode(m)] == [5, 8, 10]
    assert not host_api.forwards_line_primitive_mode(0) and not host_api.forwards_line_primitive_mode(4)


def test_settings_path_reaches_the_line_primitive_mode():
    """LineData::setNewSettings: the key a command line's key = value pair or a plugin's setNewSettings carries"""
    from linevis_amd import scenes
    tr = scenes.normalize(scenes.random_curves(n_lines=3, points_per_line=5, seed=3))
    flow = host_api.LineDataFlow().set_trajectories(tr.positions, tr.attributes, tr.line_offsets)
    try:
        flow.set_new_settings({"line_primitive_mode": QUADS})
        assert flow.line_primitive_mode == QUADS
        flow.set_new_settings({"line_primitive_mode": "no such mode"})
        assert flow.line_primitive_mode == QUADS
        flow.set_new_settings({"line_primitive_mode_index": 2})
        assert flow.line_primitive_mode == TUBE
    finally:
        flow.set_new_settings({"line_primitive_mode": TUBE})       # (the mode is a static member, as in the reference)
