"""The C ABI as include/unidom_hip.h declares it, parsed once at import: the conf structs as ctypes.Structure classes, every ud_*
prototype as (restype, argtypes) and the integer #defines.  The header is the only place where a prototype or a struct field is
written; _lib.py, tools/gen_binding_stub.py and tests/test_abi.py all read this module.  No torch, no GPU work.

Mapping is by ABI class: a parameter whose declaration contains `*` is a c_void_p (handles, out pointers, arrays of pointers); the
scalars are those of SCALARS.  Whatever the parser does not recognise raises UnidomError naming the declaration -- nothing is guessed
and nothing is skipped."""
from __future__ import annotations

import ctypes as C
import os
import re

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "unidom_hip.h")
SCALARS = {"int": C.c_int, "long": C.c_long, "long long": C.c_longlong, "unsigned": C.c_uint, "unsigned int": C.c_uint,
           "size_t": C.c_size_t, "float": C.c_float, "double": C.c_double}


class UnidomError(RuntimeError):
    pass


def _scalar(ty, decl):
    ty = " ".join(w for w in ty.split() if w != "const")
    if ty not in SCALARS:
        raise UnidomError(f"include/unidom_hip.h: unknown scalar type `{ty}` in `{decl}`")
    return SCALARS[ty]


def _struct(name, body, defines):
    fields = []
    for decl in filter(None, (d.strip() for d in body.split(";"))):
        m = re.match(r"((?:\w+\s+)+)(\w+(?:\[\w+\])*(?:\s*,\s*\w+(?:\[\w+\])*)*)$", decl)
        if not m:
            raise UnidomError(f"include/unidom_hip.h: cannot split field `{decl}` of {name}")
        ct = _scalar(m.group(1), f"{name}: {decl}")
        for item in re.split(r"\s*,\s*", m.group(2)):
            t = ct
            for dim in reversed(re.findall(r"\[(\w+)\]", item)):      # a[2][4] = two rows of four: (T * 4) * 2
                if not dim.isdigit() and dim not in defines:
                    raise UnidomError(f"include/unidom_hip.h: unknown array size `{dim}` in `{decl}` of {name}")
                t = t * (int(dim) if dim.isdigit() else defines[dim])
            fields.append((item.split("[")[0], t))
    return type(name, (C.Structure,), {"_fields_": fields})


def _prototype(decl):
    m = re.match(r"(.*?)\b(ud_\w+)\s*\((.*)\)$", decl, flags=re.S)
    if not m:
        raise UnidomError(f"include/unidom_hip.h: not a ud_* prototype: `{decl}`")
    ret, name, args = " ".join(m.group(1).split()), m.group(2), " ".join(m.group(3).split())
    if "*" in ret:
        if ret.replace(" ", "") != "constchar*":
            raise UnidomError(f"include/unidom_hip.h: unknown return type `{ret}` in `{decl}`")
        restype = C.c_char_p
    else:
        restype = None if ret == "void" else _scalar(ret, decl)
    argtypes = []
    for arg in ([] if args == "void" else args.split(",")):
        if "*" in arg:
            argtypes.append(C.c_void_p)
            continue
        m = re.match(r"\s*((?:\w+\s+)+)\w+\s*$", arg)           # type words, then the parameter's name
        if not m:
            raise UnidomError(f"include/unidom_hip.h: cannot split parameter `{arg.strip()}` in `{decl}`")
        argtypes.append(_scalar(m.group(1), decl))
    return name, (restype, argtypes)


def parse(header=HEADER):
    """(DEFINES, STRUCTS, PROTOTYPES) of one header file."""
    try:
        src = open(header).read()
    except OSError as e:
        raise UnidomError(f"{header} is missing: the binding is derived from it ({e})") from None
    src = re.sub(r"/\*.*?\*/", " ", src, flags=re.S)
    defines = {n: int(v, 0) for n, v in re.findall(r"^[ \t]*#[ \t]*define[ \t]+(\w+)[ \t]+(-?(?:0[xX][0-9a-fA-F]+|\d+))[ \t]*$", src, flags=re.M)}
    src = re.sub(r"^[ \t]*#.*$", "", src, flags=re.M)
    structs = {}

    def take(m):
        structs[m.group(2)] = _struct(m.group(2), m.group(1), defines)
        return ""
    src = re.sub(r"typedef\s+struct\s*\w*\s*\{(.*?)\}\s*(\w+)\s*;", take, src, flags=re.S)
    src = re.sub(r"typedef\s+enum\s*\w*\s*\{.*?\}\s*\w+\s*;|typedef\s+struct\s+\w+\s+\w+\s*;|extern\s+\"C\"\s*\{", "", src, flags=re.S)
    src = re.sub(r"^\}\s*$", "", src, flags=re.M)               # the closing brace of extern "C"
    protos = dict(_prototype(d.strip()) for d in src.split(";") if d.strip())
    return defines, structs, protos


DEFINES, STRUCTS, PROTOTYPES = parse()
