"""hull_fragment_pool at the boundaries, without a GPU: the key in the header with its default and restrictions, in the option parser
and the options struct; the two host plugins that handle it; the command line's help."""
import os
import re

from linevis_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _read(*parts):
    return open(os.path.join(ROOT, *parts)).read()


def test_key_in_the_header_the_parser_and_the_options():
    header = open(capi.HEADER_PATH).read()
    m = re.search(r"^ \*   hull_fragment_pool \(build-owned switch\): \"off\" \(default", header, flags=re.M)
    assert m
    text = re.sub(r"\s*\n \*\s+", " ", header[m.start():m.start() + 3300])        # (the comment's line breaks are not the point)
    for needle in ("\"on\"", "(segments << 6) + hull triangle", "0xFFFFFFFE", "LV_E_CAPACITY", "ppll_prism_rasteriser = lbvh",
                   "capsule_entry", "Quads (Programmable Pull)", "Pooled mode 6 draws no hull", "lv_hull_pool.h", "LV_KERNEL_HULL"):
        assert needle in text, needle
    assert header.index("hull_ray_tracing (build-owned switch)") < m.start()       # next to its sibling
    assert re.search(r"bool\s+hullFragmentPool\s*=\s*false\s*;", _read("linevis_amd", "csrc", "lv_internal.h"))
    api = _read("linevis_amd", "csrc", "lv_api.hip")
    m = re.search(r'k == "hull_fragment_pool"\) \{(.*?)\n    \} else if', api, flags=re.S)
    assert m and '"on"' in m.group(1) and '"off"' in m.group(1) and "return bad();" in m.group(1)
    assert "hull_fragment_pool=on" in _read("linevis_amd", "__main__.py")


def test_host_plugins_handle_the_key():
    src = _read("linevis_amd", "host", "LineRenderer.cpp")
    # one statement of the switch: the key's value reaches the library, and drawsHull follows it
    m = re.search(r"bool LineRenderer::setHullSwitch\(const SettingsMap& settings, const char\* key\) \{(.*?)\n\}", src, flags=re.S)
    assert m and "setOption(key, value)" in m.group(1) and 'drawsHull = value == "on";' in m.group(1)
    assert 'setOption("hull_opacity", "0")' in m.group(1) and "linesDirty = true;" in m.group(1)
    for cls in ("HipPerPixelLinkedListLineRenderer", "HipMLABRenderer"):
        body = re.search(r"bool %s::setNewSettings\(const SettingsMap& settings\) \{(.*?)\n\}" % cls, src, flags=re.S)
        assert body and 'setHullSwitch(settings, "hull_fragment_pool")' in body.group(1), cls
    other = re.search(r"bool HipMBOITRenderer::setNewSettings\(const SettingsMap& settings\) \{(.*?)\n\}", src, flags=re.S)
    assert other and "hull_fragment_pool" not in other.group(1)                     # pooled mode 6 draws no hull
    assert 'setHullSwitch(settings, "hull_ray_tracing")' in src
    assert "bool setHullSwitch(const SettingsMap& settings, const char* key);" in _read("linevis_amd", "host", "LineRenderer.hpp")
