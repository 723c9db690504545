"""lv_set_trajectories_with_bands without a GPU: the header declares it in C99, the library exports it, and the host layer's
LineData::getTrajectoryArrays hands over the ribbon directions, the helicity attribute and maxHelicity it was given (whatever the
use_ribbons / rotating_helicity_bands switches say: toggling them must not need a new upload)."""
import os
import subprocess

import numpy as np

from linevis_amd import build as lv_build, capi, host_api, scenes


def test_header_compiles_as_c99_with_the_band_struct(tmp_path):
    src = tmp_path / "bands.c"
    src.write_text('#include <stddef.h>\n#include "linevis_hip.h"\n'
                   'int set_bands(lv_ctx* ctx, const float* pos, const float* rib, const float* hel, const uint32_t* off) {\n'
                   '  lv_trajectory_bands b;\n'
                   '  b.ribbon_directions = rib;\n'
                   '  b.helicity = hel;\n'
                   '  b.max_helicity = 0.0f;\n'
                   '  return lv_set_trajectories_with_bands(ctx, pos, NULL, off, 1u, &b);\n'
                   '}\n')
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-c", "-I", os.path.dirname(capi.HEADER_PATH),
                           str(src), "-o", str(tmp_path / "bands.o")])
    assert "lv_set_trajectories_with_bands" in capi.SYMBOLS


def test_library_exports_the_band_entry_point():
    out = subprocess.check_output(["nm", "-D", "--defined-only", lv_build.LIB], text=True)
    names = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert {"lv_set_trajectories", "lv_set_trajectories_with_bands"} <= names


def _curves():
    tr = scenes.normalize(scenes.random_curves(n_lines=7, points_per_line=13, seed=5))
    return tr, (tr.attributes[0] if np.ndim(tr.attributes) == 2 else tr.attributes).astype(np.float32)


def test_host_layer_hands_over_the_ribbon_directions():
    tr, att = _curves()
    rib = scenes.twisted_ribbons(tr).ribbon_directions
    flow = host_api.LineDataFlow().set_trajectories(tr.positions, att, tr.line_offsets, ribbon_directions=rib)
    for use_ribbons in (True, False):
        flow.set_new_settings(dict(use_ribbons=use_ribbons))
        a = flow.trajectory_arrays_bands()
        assert a is not None and a["helicity"] is None
        assert np.array_equal(a["positions"], tr.positions.astype(np.float32))
        assert np.array_equal(a["line_offsets"], tr.line_offsets) and np.array_equal(a["attribute"], att)
        assert a["ribbon_directions"].tobytes() == rib.tobytes()


def test_host_layer_hands_over_the_helicity_attribute_and_its_maximum():
    tr, att = _curves()
    hel = np.linspace(-0.03, 0.02, len(tr.positions)).astype(np.float32)
    flow = host_api.LineDataFlow().set_trajectories_multi(tr.positions, np.stack([att, hel]), ["Velocity Magnitude", "Helicity"],
                                                          tr.line_offsets)
    for on in (False, True):
        flow.set_new_settings(dict(rotating_helicity_bands=on))
        a = flow.trajectory_arrays_bands()
        assert a["ribbon_directions"] is None
        assert a["helicity"].tobytes() == hel.tobytes() and np.array_equal(a["attribute"], att)
        assert a["max_helicity"] == flow.max_helicity == np.float32(0.03)
    plain = host_api.LineDataFlow().set_trajectories(tr.positions, att, tr.line_offsets).trajectory_arrays_bands()
    assert plain["ribbon_directions"] is None and plain["helicity"] is None and plain["max_helicity"] == 0.0
