"""Every device buffer of a context is owned: lv_all_buffers() (lv_api.hip) is the list lv_destroy frees and lv_get_stats sums into
device_bytes, so a LvDeviceBuffer member that is missing from it leaks with every context and is invisible in the memory accounting.
The members are read from the structs in lv_internal.h, the list from the function's text -- no GPU needed."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "linevis_amd", "csrc")


def _strip_comments(text):
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    return re.sub(r"//[^\n]*", "", text)


def _block(text, head):
    """the brace-balanced body that follows the first match of `head`"""
    m = re.search(head, text)
    assert m, head
    i = text.index("{", m.end() - 1)
    depth, j = 0, i
    while True:
        depth += {"{": 1, "}": -1}.get(text[j], 0)
        if depth == 0:
            return text[i + 1:j], j
        j += 1


def _buffer_members(body):
    names = []
    for decl in re.findall(r"\bLvDeviceBuffer\b([^;()]*);", body):
        for n in decl.split(","):
            n = n.strip()
            assert re.fullmatch(r"[A-Za-z_]\w*", n), "unexpected LvDeviceBuffer declaration: %r" % decl
            names.append(n)
    return names


def declared_buffers():
    """expressions (relative to the context) of every LvDeviceBuffer in lv_ctx, LvSvgfState and lv_ctx::GroupOrder"""
    text = _strip_comments(open(os.path.join(CSRC, "lv_internal.h")).read())
    svgf, _ = _block(text, r"\bstruct\s+LvSvgfState\s*\{")
    ctx, _ = _block(text, r"\bstruct\s+lv_ctx\s*\{")
    group, end = _block(ctx, r"\bstruct\s+GroupOrder\s*\{")
    instance = re.match(r"\s*(\w+)\s*\[\s*(\d+)\s*\]\s*;", ctx[end + 1:])
    assert instance, "lv_ctx::GroupOrder is expected to be declared with its array of instances"
    group_name, group_count = instance.group(1), int(instance.group(2))
    svgf_name = re.search(r"\bLvSvgfState\s+(\w+)\s*;", ctx).group(1)
    top = ctx.replace(group, "")
    out = _buffer_members(top)
    out += ["%s.%s" % (svgf_name, n) for n in _buffer_members(svgf)]
    out += ["%s[%d].%s" % (group_name, i, n) for i in range(group_count) for n in _buffer_members(group)]
    return out


def listed_buffers():
    text = _strip_comments(open(os.path.join(CSRC, "lv_api.hip")).read())
    body, _ = _block(text, r"\blv_all_buffers\s*\(\s*lv_ctx\s*\*\s*ctx\s*\)\s*\{")
    return [re.sub(r"\s+", "", e) for e in re.findall(r"&\s*ctx\s*->\s*([\w.\[\]\s]+?)\s*[,}]", body)]


def test_the_parser_sees_the_structs():
    d = declared_buffers()
    assert len(d) > 90 and len(set(d)) == len(d)
    for name in ("points", "svgf.colorHistory", "groupOrder[0].cost", "groupOrder[1].order", "flowOccupancy", "stackOverflow"):
        assert name in d, name
    assert "stream" not in d and "pinned" not in d


def test_every_device_buffer_is_in_lv_all_buffers():
    declared, listed = declared_buffers(), listed_buffers()
    assert len(set(listed)) == len(listed), "listed twice (freed twice): %s" % sorted(n for n in set(listed) if listed.count(n) > 1)
    missing = sorted(set(declared) - set(listed))
    assert not missing, "LvDeviceBuffer members that lv_destroy never frees and device_bytes omits: %s" % missing
    unknown = sorted(set(listed) - set(declared))
    assert not unknown, "lv_all_buffers() names something that is no LvDeviceBuffer member: %s" % unknown
