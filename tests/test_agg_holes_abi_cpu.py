"""CPU: far3d_aggregate_batched_holes exists at every layer of the C ABI -- the cross-compiled library exports it, far3d_amd.lib binds it
with far3d_aggregate_batched's arguments plus the hole, and include/far3d_hip.h declares it that way."""
import ctypes
import os
import re

from tests.conftest import ROOT

NAME, BASE = "far3d_aggregate_batched_holes", "far3d_aggregate_batched"


def _declaration(name):
    """The parameter list of `name` in the header, comments dropped: a list of (type, parameter name)."""
    src = open(os.path.join(ROOT, "include", "far3d_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, src)
    assert m, "include/far3d_hip.h does not declare %s" % name
    params = [" ".join(p.split()) for p in m.group(1).split(",")]
    return [tuple(re.match(r"(.*?)(\w+)$", p).groups()) for p in params]


def test_the_library_exports_the_entry(hip_lib):
    assert hasattr(hip_lib, NAME), "libfar3d_hip.so does not export %s" % NAME
    assert hasattr(hip_lib, BASE)


def test_the_binding_is_the_batched_entrys_plus_the_hole():
    from far3d_amd import lib
    res, args = lib.SIGNATURES[NAME]
    res0, args0 = lib.SIGNATURES[BASE]
    assert res is res0 is ctypes.c_int
    # the existing arguments, then (hole_count, hole_start, hole_end), then the stream
    assert list(args) == list(args0[:-1]) + [ctypes.c_void_p, ctypes.c_int, ctypes.c_int] + [args0[-1]]


def test_the_header_declares_it_with_the_three_new_arguments():
    new, old = _declaration(NAME), _declaration(BASE)
    assert new[:len(old) - 1] == old[:-1] and new[-1] == old[-1]
    added = [(t.strip(), n) for t, n in new[len(old) - 1:-1]]
    assert added == [("const int32_t*", "hole_count"), ("int", "hole_start"), ("int", "hole_end")]
    from far3d_amd import lib
    assert len(lib.SIGNATURES[NAME][1]) == len(new)
