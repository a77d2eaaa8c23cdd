"""The C headers as the ABI tests read them (tests/test_abi_conformance.py, the per-header
tests/test_*_abi.py and tests/test_guard_coverage.py): one parser for the declarations
and the structs of include/*.h, and the C type -> ctypes rule of the bindings
(hetersumgraph_amd/_lib.py for libhsg.so, datapipe.py for libhsg_host.so).

The parser knows what the headers use and no more: block and line comments, declarations
of the form ``ret hsg_name(params);`` and structs of scalar, pointer and struct-array
fields.  A type it does not know is a KeyError, not a guess.  No GPU needed.
"""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")

SCALARS = {"int": ctypes.c_int, "float": ctypes.c_float, "long": ctypes.c_long, "size_t": ctypes.c_size_t,
           "int64_t": ctypes.c_int64, "int32_t": ctypes.c_int32, "uint32_t": ctypes.c_uint32}


def source(header):
    """The header's text (a name under include/, or a path) without comments and directives."""
    src = open(os.path.join(INCLUDE, header)).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    src = re.sub(r"//[^\n]*", "", src)
    return re.sub(r"^\s*#[^\n]*", "", src, flags=re.M)


def declared_functions(header):
    """Sorted names of every ``hsg_*(`` the header mentions outside its comments."""
    return sorted(set(re.findall(r"\b(hsg_[a-z0-9_]+)\s*\(", source(header))))


def declarations(header):
    """{name: (return type, [parameter strings])} of the header's function declarations,
    whitespace normalised: ``("int", ["const hsg_rel *rel", "int H", ...])``; ``(void)`` is []."""
    out = {}
    for ret, name, params in re.findall(r"\b((?:const\s+)?\w+[\s*]+)(hsg_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", source(header)):
        assert name not in out, f"{header} declares {name} twice"
        params = [" ".join(p.split()) for p in params.split(",")]
        out[name] = (" ".join(ret.split()), [] if params in ([""], ["void"]) else params)
    return out


def writable_entry_points(headers):
    """hsg_* functions with a pointer parameter whose pointee is not const (the stream
    handle aside), from the headers' declarations: {name: [parameter strings]}."""
    out = {}
    for header in headers:
        for name, (_, params) in declarations(header).items():
            w = [p for p in params if "*" in p and not p.startswith("const ") and not p.endswith("*stream")]
            if w:
                out[name] = w
    return out


def struct_fields(header, name):
    """(type, field) pairs of ``struct <name> {...}`` in the header, in order; a pointer
    field's type ends in `` *``, an array field keeps its ``[n]``."""
    body = re.search(r"\bstruct %s\s*\{(.*?)\}" % name, source(header), flags=re.S).group(1)
    out = []
    for decl in body.split(";"):
        decl = " ".join(decl.split())
        if not decl:
            continue
        ty, names = re.match(r"((?:const )?\w+) (.*)", decl).groups()
        for n in names.split(","):
            n = n.strip()
            out.append((ty + (" *" if n.startswith("*") else ""), n.lstrip("*")))
    return out


def struct_pointers():
    """The parameters that are bound as a pointer to a struct mirror, by their C type."""
    from hetersumgraph_amd import _lib, datapipe
    return {"const hsg_rel *": _lib.HsgRel, "const struct hsg_mt_tensor *": _lib.HsgMtTensor,
            "const hsg_res_store *": _lib.HsgResStore, "const hsg_docs *": datapipe.HsgDocs}


def ctype_of_param(prm):
    """The ctypes type of one parameter string: a struct pointer for the mirrored structs,
    ``c_void_p`` for every other pointer, the scalar's type otherwise."""
    ty = prm[:len(prm) - len(re.search(r"\w+$", prm).group(0))].rstrip()
    if "*" in ty:
        ty = re.sub(r"\s*\*", " *", ty)
        mirror = struct_pointers().get(ty)
        return ctypes.POINTER(mirror) if mirror is not None else ctypes.c_void_p
    return SCALARS[ty]


def ctype_of_return(ret):
    """The ctypes restype of a declared return type (``void`` is None)."""
    if ret == "void":
        return None
    return ctypes.c_char_p if re.sub(r"\s*\*", " *", ret) == "const char *" else SCALARS[ret]


def signature(header, name):
    """(restype, argtypes) that the header's declaration of ``name`` asks of a binding."""
    ret, params = declarations(header)[name]
    return ctype_of_return(ret), [ctype_of_param(p) for p in params]


def mirror_fields(header, name, nested=()):
    """The ``_fields_`` a ctypes mirror of ``struct <name>`` must have; ``nested`` maps the
    C name of a struct used as an array field to its mirror."""
    nested = dict(nested)
    out = []
    for ty, field in struct_fields(header, name):
        m = re.match(r"(\w+)\[(\d+)\]$", field)
        if ty.endswith("*"):
            out.append((field, ctypes.c_void_p))
        elif m:
            out.append((m.group(1), nested[ty] * int(m.group(2))))
        else:
            out.append((field, SCALARS[ty]))
    return out
