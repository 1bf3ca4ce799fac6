"""CPU: the C-ABI library loads and exports every symbol include/unidom_hip.h declares, and the ctypes binding derived from the header
(unidom_amd/_abi.py) agrees with the C compiler about every struct and carries every prototype (no compute calls)."""
import ctypes
import os
import re

from conftest import ROOT


def _header_symbols():
    src = open(os.path.join(ROOT, "include", "unidom_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(ud_[a-z0-9_]+)\s*\(", src)))


def test_library_exports_every_declared_symbol():
    from unidom_amd import _lib
    so = _lib.build()
    L = ctypes.CDLL(so)
    declared = _header_symbols()
    assert declared, "no symbols parsed from the header"
    missing = [s for s in declared if not hasattr(L, s)]
    assert not missing, f"declared in include/unidom_hip.h but not exported: {missing}"
    assert sorted(_lib.SYMBOLS) == declared, (sorted(_lib.SYMBOLS), declared)
    L.ud_version.restype = ctypes.c_char_p
    assert b"gfx950" in L.ud_version()


def test_product_never_imports_the_oracle():
    """The oracle is test infrastructure: nothing under unidom_amd/ may reference it."""
    bad = []
    for dp, _, fns in os.walk(os.path.join(ROOT, "unidom_amd")):
        for fn in fns:
            if fn.endswith((".py", ".hip", ".h", ".cpp")):
                txt = open(os.path.join(dp, fn)).read()
                if re.search(r"^\s*(from|import)\s+oracle\b|#include\s+\"[^\"]*oracle", txt, flags=re.M):
                    bad.append(os.path.join(dp, fn))
    assert not bad, bad


def test_missing_library_fails_loudly(monkeypatch, tmp_path):
    from unidom_amd import _lib
    monkeypatch.setattr(_lib, "SO_PATH", str(tmp_path / "nope.so"))
    monkeypatch.setattr(_lib, "_LIB", None)
    try:
        _lib.lib()
    except _lib.UnidomError as e:
        assert "no fallback" in str(e).lower()
    else:
        raise AssertionError("expected UnidomError")


def _leaf(t):
    """(innermost element type, number of array levels) of a ctypes field type"""
    n = 0
    while hasattr(t, "_length_"):
        t, n = t._type_, n + 1
    return t, n


def test_ctypes_structs_match_the_header_layout(tmp_path):
    """include/unidom_hip.h is the contract; unidom_amd/_abi.py parses its structs into ctypes.  The C compiler is the independent party:
    compile the header with gcc and compare sizeof, every offsetof and (through _Generic on the innermost element) every field's
    element type, for every struct the header defines."""
    import ctypes as C
    import subprocess

    from unidom_amd import _abi, _lib
    structs = _abi.STRUCTS
    assert list(structs) == ["ud_cloth_conf", "ud_mpm_conf", "ud_plb_conf", "ud_plb_render_conf", "ud_plb_render_light",
                             "ud_cloth_render_conf", "ud_mpm_render_conf"]
    assert _abi.DEFINES["UD_PLB_RENDER_MAX_PRIM"] == 4 == _lib.RENDER_MAX_PRIM
    names = {C.c_int: "int", C.c_float: "float", C.c_double: "double"}
    lines = ["#include <stddef.h>", "#include <stdio.h>", '#include "unidom_hip.h"',
             '#define ELEM(x) _Generic((x), int: "int", float: "float", double: "double", default: "other")', "int main(void) {"]
    for name, st in structs.items():
        assert issubclass(st, C.Structure) and st.__name__ == name and getattr(_lib, name) is st
        lines.append(f'  printf("{name} %zu -\\n", sizeof({name}));')
        for field, t in st._fields_:
            lines.append(f'  printf("{name}.{field} %zu %s\\n", offsetof({name}, {field}), ELEM((({name}*)0)->{field}{"[0]" * _leaf(t)[1]}));')
    lines += ["  return 0;", "}"]
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = {k: (int(n), ty) for k, n, ty in (line.split() for line in subprocess.check_output([str(exe)], text=True).splitlines())}
    for name, st in structs.items():
        assert got[name][0] == C.sizeof(st), (name, got[name], C.sizeof(st))
        for field, t in st._fields_:
            assert got[f"{name}.{field}"] == (getattr(st, field).offset, names[_leaf(t)[0]]), (name, field, got[f"{name}.{field}"])
    assert len(got) == len(structs) + sum(len(st._fields_) for st in structs.values())


def test_integration_stub_and_lib_structs_are_the_header():
    """INTEGRATION.md shows the reference-side ctypes binding; its struct block is rendered from the parsed header
    (tools/gen_binding_stub.py) and must be current.  (That the parsed structs ARE the header's is the compiler's word, above.)"""
    import importlib.util

    spec = importlib.util.spec_from_file_location("gen_binding_stub", os.path.join(ROOT, "tools", "gen_binding_stub.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    assert gen.current_block() == gen.render(), "run `python tools/gen_binding_stub.py --write`"
    assert set(re.findall(r"^class (\w+)\(C\.Structure\)", gen.current_block(), flags=re.M)) == {"ud_cloth_conf", "ud_mpm_conf", "ud_plb_conf"}


def test_every_function_is_typed_from_the_header():
    from unidom_amd import _abi, _lib
    L = _lib.lib()
    assert sorted(_abi.PROTOTYPES) == _header_symbols() == _lib.SYMBOLS
    assert len(_abi.PROTOTYPES) == 76
    for name, (restype, argtypes) in _abi.PROTOTYPES.items():
        fn = getattr(L, name)
        assert fn.restype is restype and list(fn.argtypes) == argtypes, name


def test_awkward_declarations_have_their_known_answers():
    from ctypes import c_char_p, c_double, c_float, c_int, c_long, c_size_t, c_uint
    from ctypes import c_void_p as p

    from unidom_amd._abi import PROTOTYPES as P
    assert P["ud_last_error"] == (c_char_p, [])
    assert P["ud_version"] == (c_char_p, [])
    assert P["ud_cloth_destroy"] == (None, [p]) and P["ud_mpm_destroy"] == (None, [p]) and P["ud_plb_destroy"] == (None, [p])
    assert P["ud_plb_render_destroy"] == (c_int, [p])
    assert P["ud_cloth_create"] == (c_int, [p, p, p])
    assert P["ud_cloth_ckpt_bytes"] == (c_size_t, [p, c_int, c_int])
    assert P["ud_mpm_focus_fwd"] == (c_int, [c_int] * 4 + [c_float] * 2 + [p] * 6)      # const float* const*, float* const* among them
    assert P["ud_plb_policy_fwd"] == (c_int, [c_int] * 6 + [p, c_int, c_double] + [p] * 5 + [c_long] + [p] * 3)
    assert P["ud_plb_policy_bwd"] == (c_int, [c_int] * 6 + [p, c_int, c_double] + [p, c_long] + [p] * 8)
    assert P["ud_plb_density_seq_fwd"] == (c_int, [p, c_long, p, p, c_int] + [p] * 4 + [c_size_t, p])
    assert P["ud_plb_density_seq_work_bytes"] == (c_size_t, [p, c_long])
    assert P["ud_plb_density_iou"] == (c_int, [c_long, c_int, p, p, c_int] + [p] * 3)
    assert P["ud_plb_chamfer"] == (c_int, [c_long, c_int, p, c_int, c_int] + [p] * 6)
    assert P["ud_plb_target_sdf"] == (c_int, [c_int, c_int, p, c_double, c_int] + [p] * 5)
    assert P["ud_plb_render_image"] == (c_int, [p, c_int] + [p] * 3 + [c_int, c_uint] + [p] * 2)
    assert P["ud_plb_render_read_volume"] == (c_int, [p, c_int] + [p] * 3)              # long long* packed
    assert P["ud_cloth_render_frames"] == (c_int, [p, c_int] + [p] * 6)                 # unsigned char* color
    assert P["ud_pc_ball_query"] == (c_int, [c_int] * 3 + [c_float, c_int] + [p] * 5)
    assert P["ud_cloth_depth_fwd"] == (c_int, [c_int] * 4 + [c_float] * 2 + [p] * 4)


_MINI = """/* a header */
#define UD_N 3
typedef struct ud_thing ud_thing;
typedef struct { int a; %s } ud_thing_conf;
int ud_thing_create(const ud_thing_conf* conf, ud_thing** out);
%s
"""


def test_the_parser_fails_loudly(tmp_path):
    import ctypes as C

    import pytest

    from unidom_amd import _abi
    h = tmp_path / "mini.h"
    h.write_text(_MINI % ("double b[UD_N][2], c;", "long long ud_thing_count(const ud_thing* h, unsigned n, long long k);"))
    defines, structs, protos = _abi.parse(str(h))
    assert defines == {"UD_N": 3}
    assert [(f, C.sizeof(t)) for f, t in structs["ud_thing_conf"]._fields_] == [("a", 4), ("b", 48), ("c", 8)]
    assert protos == {"ud_thing_create": (C.c_int, [C.c_void_p] * 2), "ud_thing_count": (C.c_longlong, [C.c_void_p, C.c_uint, C.c_longlong])}
    for field, proto, named in [("", "int ud_thing_step(ud_thing* h, short n);", "ud_thing_step"),          # an unknown scalar type
                                ("", "short ud_thing_step(ud_thing* h);", "ud_thing_step"),
                                ("short s;", "", "short s"),
                                ("int (*fn)(int);", "", "ud_thing_conf"),                                    # a field it cannot split
                                ("int a[UD_M];", "", "UD_M"),
                                ("", "int ud_thing_step(ud_thing* h, int n[3]);", "ud_thing_step"),
                                ("", "static int x;", "static int x")]:                                      # not a prototype at all
        h.write_text(_MINI % (field, proto))
        with pytest.raises(_abi.UnidomError) as e:
            _abi.parse(str(h))
        assert named in str(e.value), (named, str(e.value))
    with pytest.raises(_abi.UnidomError) as e:
        _abi.parse(str(tmp_path / "absent.h"))
    assert "absent.h" in str(e.value)
