"""ctypes binding of libtexpose_amd.so, derived at import from include/texpose_amd.h (the C ABI's one source).

Every `TP_X` constant of the header is published as `TP_X` and as `X`, every `typedef struct tp_foo_bar` as the
ctypes.Structure `FooBar`, and load() gives every prototype its argtypes / restype.

There is deliberately NO fallback: if the HIP library is missing or a launch fails, the
product path raises.  (The CPU oracle under oracle/ is test infrastructure only.)
"""
from __future__ import annotations

import ctypes as C
import os
import re
from typing import Dict, List, NamedTuple, Tuple

_HERE = os.path.dirname(os.path.abspath(__file__))
# TEXPOSE_AMD_LIB selects another build of the SAME library (e.g. the `make trace` diagnostic build); never a fallback
LIB_PATH = os.environ.get("TEXPOSE_AMD_LIB") or os.path.join(_HERE, "libtexpose_amd.so")
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "texpose_amd.h")


class TexposeLibraryError(RuntimeError):
    pass


class Header(NamedTuple):
    constants: Dict[str, int]                      # #define TP_X <integer> and every enumerator
    structs: Dict[str, type]                       # C name -> ctypes.Structure subclass, in declaration order
    prototypes: Dict[str, Tuple[object, List]]     # name -> (restype, argtypes), in declaration order


_SCALARS = {"int": C.c_int, "unsigned int": C.c_uint, "float": C.c_float, "double": C.c_double, "size_t": C.c_size_t,
            **{f"{u}int{b}_t": getattr(C, f"c_{u}int{b}") for u in ("", "u") for b in (8, 16, 32, 64)}}
# the include guard, #include lines and the extern "C" wrapper: the only preprocessor lines besides `#define NAME <integer>`
_CPP_WRAPPER = re.compile(r'#ifdef __cplusplus\s*(?:extern "C" \{|\})\s*#endif')
_CPP_PLAIN = re.compile(r"#\s*(?:include\s*<[\w./]+>|ifndef \w+_H|define \w+_H|endif)")
_CPP_DEFINE = re.compile(r"#\s*define (\w+) (-?\w+)")
_TOP_LEVEL = re.compile(r"""\s*(?:typedef\ struct\ (?P<tag>\w+)\s*\{(?P<fields>[^{}]*)\}\s*(?P<struct>\w+)\s*;
                                 |enum\s*\w*\s*\{(?P<enum>[^{}]*)\}\s*;
                                 |typedef\s+(?P<alias_of>[^;{}()]+?)(?P<alias>\w+)\s*;
                                 |(?P<ret>[^;{}()]+?)(?P<fn>\w+)\s*\((?P<params>[^;{}()]*)\)\s*;)""", re.X)
_STATEMENT = re.compile(r"((?:const\s+)?(?:unsigned\s+)?\w+)\b(.*)", re.S)
_DECLARATOR = re.compile(r"(\**)\s*(?:const\s+)?(\w+)\s*(?:\[\s*(\w+)\s*\])?")


def parse_header(text: str) -> Header:
    """Constants, struct layouts and prototypes of a C header written in the subset include/texpose_amd.h uses.
    Anything outside that subset raises TexposeLibraryError: the parser never skips what it does not understand."""
    constants: Dict[str, int] = {}
    structs: Dict[str, type] = {}
    prototypes: Dict[str, Tuple[object, List]] = {}
    types = dict(_SCALARS)                          # + typedef names and struct names as they are declared

    def bad(what: str, where: str):
        return TexposeLibraryError(f"C header: {what}: {' '.join(where.split())[:120]!r}")

    def integer(word: str, where: str) -> int:
        try:
            return constants[word] if word in constants else int(word, 0)
        except ValueError:
            raise bad("not an integer constant", where) from None

    def ctype(spec: str, stars: int, struct_pointers: bool):
        base = " ".join(w for w in spec.replace("*", " ").split() if w != "const")
        if stars == 0 and base in types:
            return types[base]
        if stars == 1 and base == "char":
            return C.c_char_p
        if stars == 1 and struct_pointers and base in structs:
            return C.POINTER(structs[base])
        if stars and (base in types or base == "void"):
            return C.c_void_p
        raise bad("unknown type", spec)

    def fields_of(body: str) -> List[Tuple[str, object]]:
        fields = []
        for statement in filter(None, map(str.strip, body.split(";"))):
            typed = _STATEMENT.fullmatch(statement)
            for declarator in typed[2].split(",") if typed else [""]:
                m = _DECLARATOR.fullmatch(declarator.strip())
                if not m:
                    raise bad("field declaration", statement)
                stars, name, count = m.groups()
                t = ctype(typed[1], len(stars), struct_pointers=False)
                fields.append((name, t * integer(count, statement) if count else t))
        return fields

    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)
    text = _CPP_WRAPPER.sub(" ", text)
    code = []
    for line in text.splitlines():
        define = _CPP_DEFINE.fullmatch(line.strip())
        if define:
            constants[define.group(1)] = integer(define.group(2), line)
        elif line.lstrip().startswith("#") and not _CPP_PLAIN.fullmatch(line.strip()):
            raise bad("preprocessor line", line)
        code.append("" if line.lstrip().startswith("#") else line)
    text = "\n".join(code).rstrip()
    pos = 0
    while pos < len(text):
        m = _TOP_LEVEL.match(text, pos)
        if not m:
            raise bad("construct the binding cannot classify", text[pos:])
        pos = m.end()
        if m["struct"]:
            if m["tag"] != m["struct"]:
                raise bad("struct tag and typedef name differ", m[0])
            name = "".join(part.capitalize() for part in m["struct"].split("_")[1:])
            # __slots__ = (): an instance has no __dict__, so assigning a misspelt field raises AttributeError
            types[m["struct"]] = structs[m["struct"]] = type(name, (C.Structure,), {"__slots__": (), "_fields_": fields_of(m["fields"])})
        elif m["enum"] is not None:
            value = -1
            for entry in filter(None, map(str.strip, m["enum"].split(","))):
                name, _, given = map(str.strip, entry.partition("="))
                constants[name] = value = integer(given, entry) if given else value + 1
        elif m["alias"]:
            types[m["alias"]] = ctype(m["alias_of"], m["alias_of"].count("*"), struct_pointers=False)
        else:
            params = [] if m["params"].strip() in ("", "void") else m["params"].split(",")
            split = [re.fullmatch(r"(.*[\s*])\w+", p.strip(), re.S) for p in params]      # type, then the parameter's name
            if not all(split):
                raise bad("parameter list", m[0])
            prototypes[m["fn"]] = (ctype(m["ret"], m["ret"].count("*"), struct_pointers=False),
                                   [ctype(s[1], s[1].count("*"), struct_pointers=True) for s in split])
    return Header(constants, structs, prototypes)


if not os.path.exists(HEADER_PATH):
    raise TexposeLibraryError(f"{HEADER_PATH} is missing: the binding is derived from it")
with open(HEADER_PATH) as _f:
    HEADER = parse_header(_f.read())
globals().update(HEADER.constants)
globals().update({k[3:]: v for k, v in HEADER.constants.items() if k.startswith("TP_")})      # ABI_VERSION, SCENE_MAX_OBJECTS, ...
globals().update({cls.__name__: cls for cls in HEADER.structs.values()})                        # RaygenArgs, SnWeight, ...
SYMBOLS = tuple(HEADER.prototypes)

_lib = None


def load() -> C.CDLL:
    """Load the HIP library (after torch, so that both share one libamdhip64 runtime)."""
    global _lib
    if _lib is not None:
        return _lib
    import torch  # noqa: F401  (loads torch's bundled libamdhip64.so.7 first; same SONAME => one runtime)
    if not os.path.exists(LIB_PATH):
        raise TexposeLibraryError(
            f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(hipcc --offload-arch=gfx950).  texpose_amd has no CPU or eager fallback.")
    lib = C.CDLL(LIB_PATH, mode=C.RTLD_GLOBAL)
    try:
        for name, (restype, argtypes) in HEADER.prototypes.items():
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = restype, argtypes
    except AttributeError as e:
        raise TexposeLibraryError(f"{LIB_PATH} is older than {HEADER_PATH}: {e}") from None
    if lib.tp_abi_version() != HEADER.constants["TP_ABI_VERSION"]:
        raise TexposeLibraryError(f"ABI mismatch: library {lib.tp_abi_version()} != header {HEADER.constants['TP_ABI_VERSION']}")
    _lib = lib
    return lib


def check(rc: int, what: str) -> None:
    if rc != 0:
        raise TexposeLibraryError(f"{what} failed (rc={rc}): {load().tp_last_error().decode()}")
