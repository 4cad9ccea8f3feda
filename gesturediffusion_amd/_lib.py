"""ctypes binding of libgdx.so, derived from its C ABI, include/gdx.h, at import.

The header is the one statement of the ABI: ``parse_header`` reads its constants, structs and prototypes, and this module
builds the ``ctypes.Structure`` classes (``gdx_dpm_step_args_t`` -> ``DpmStepArgs``), the ``GDX_*`` constants, ``EXPORTS`` and
every function's ``argtypes`` / ``restype`` from them.  The only hand-written part is the table from C type names to ctypes
(``_CTYPES``).  The parser takes exactly the C the header uses and raises on anything else, so a header change it does not
understand stops the import instead of producing a shorter struct.  tests/test_abi_host.py has a C compiler confirm every
size, offset and prototype.

The product path has NO fallback: if the HIP library is missing or fails to load, every
compute entry point raises.  Build it with ``python __graft_entry__.py`` (or
``make -C gesturediffusion_amd/csrc``); the .so stays in-tree next to its sources.
"""
import collections
import ctypes as C
import os
import re

_HERE = os.path.dirname(os.path.abspath(__file__))
# GDX_LIBGDX: another build of the same library (A/B measurements of one kernel on one box); there is still no fallback
LIB_PATH = os.environ.get("GDX_LIBGDX") or os.path.join(_HERE, "csrc", "libgdx.so")
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "gdx.h")
INT64_MIN, INT64_MAX = -2**63, 2**63 - 1   # gdx_set_guidance_interval's default: every timestep


class GdxError(RuntimeError):
    pass


# C type name -> ctypes.  `const char*` is c_char_p, a pointer to a parsed struct is POINTER(that struct) and every other
# pointer is c_void_p (_ctype): the header cannot tell a device address from a host out-parameter.
_CTYPES = {"int32_t": C.c_int32, "int64_t": C.c_int64, "uint32_t": C.c_uint32, "uint64_t": C.c_uint64, "uint8_t": C.c_uint8,
           "float": C.c_float, "double": C.c_double, "int": C.c_int, "gdx_handle_t": C.c_void_p}

# constants: {name: int};  structs: {C name: [(type, field, array length or None)]};  prototypes: {name: (return type,
# [(type, parameter)])}, all in header order.  A type is written "[const ]T[*]".
Header = collections.namedtuple("Header", "constants structs prototypes")

# The grammar, one pattern per form.  A type in front of a function's or a parameter's name is "[const] T" then '*' or a blank.
_INT = r"([-+]?(?:0[xX][0-9a-fA-F]+|\d+))"
_TYPE = r"(const\s+)?(\w+)(\s*\*\s*|\s+)"
_COMMENT = re.compile(r"/\*.*?\*/|//[^\n]*", re.S)
_CPLUSPLUS = re.compile(r'#ifdef __cplusplus\s+(?:extern "C" \{|\})\s+#endif\b')
_GUARD = re.compile(r"\s*#ifndef (\w+)\s+#define \1[ \t]*\n(.*)#endif\s*", re.S)
_DIRECTIVE = re.compile(r"^[ \t]*(#[^\n]*?)[ \t]*$", re.M)
_DEFINE = re.compile(r"#define (\w+)\s+" + _INT)
_DECL = re.compile(r"\s*([^;{}]*(?:\{[^{}]*\}[^;{}]*)?);")      # at most one pair of braces, never nested, ended by ';'
_ENUM = re.compile(r"enum\s*\{(.*)\}", re.S)
_ENUM_ENTRY = re.compile(r"\s*(\w+)\s*=\s*" + _INT + r"\s*")
_HANDLE = re.compile(r"typedef\s+struct\s+\w+\s*\*\s*(\w+)")
_STRUCT = re.compile(r"typedef\s+struct\s*\{(.*);\s*\}\s*(\w+)", re.S)
_FIELD = re.compile(r"\s*(const\s+)?(\w+)\b(.*)", re.S)          # the type, then one declarator or several
_DECLARATOR = re.compile(r"\s*(\*?)\s*(\w+)\s*(?:\[\s*(\d+)\s*\])?\s*")
_PROTO = re.compile(_TYPE + r"(\w+)\s*\((.*)\)", re.S)
_PARAM = re.compile(r"\s*" + _TYPE + r"(\w+)\s*")


def parse_header(text):
    """Parse the subset of C that include/gdx.h is written in; ValueError, naming the text, on anything else.

    Accepted: comments, the include guard, ``#include <stdint.h>``, the ``#ifdef __cplusplus`` / ``extern "C"`` wrapper,
    ``#define NAME integer``, anonymous enums with explicit values, ``typedef struct tag* name;`` for a name in the type table,
    ``typedef struct { ... } name;`` whose fields are ``[const] T name``, ``[const] T* name`` or ``[const] T* name[N]`` (several
    declarators per line allowed), and prototypes ``[const] T[*] name(void | [const] T[*] name, ...);``."""
    hdr = Header({}, {}, {})

    def bad(what, src):
        return ValueError(f"gdx.h: {what}: {' '.join(src.split())!r}")

    def add(table, name, value, src):
        if name in table:
            raise bad(f"{name} declared twice", src)
        table[name] = value

    def ctype_name(const, base, star, src):
        star = star.strip()
        if base in hdr.structs and not star:
            raise bad(f"struct {base} by value (a nested struct)", src)
        if not (base in _CTYPES or base in hdr.structs or (star and base in ("void", "char"))):
            raise bad(f"unknown type {base!r}", src)
        return ("const " if const else "") + base + star

    def directive(m):
        define = _DEFINE.fullmatch(m.group(1))
        if define:
            add(hdr.constants, define.group(1), int(define.group(2), 0), m.group(1))
        elif m.group(1) != "#include <stdint.h>":
            raise bad("unknown directive", m.group(1))
        return " "

    text = _COMMENT.sub(" ", text)
    if "/*" in text:
        raise bad("unterminated comment", text[text.index("/*"):][:60])
    text = _CPLUSPLUS.sub(" ", text)
    guard = _GUARD.fullmatch(text)
    text = _DIRECTIVE.sub(directive, guard.group(2) if guard else text)

    decls, pos = [], 0
    while m := _DECL.match(text, pos):
        decls.append(m.group(1).strip())
        pos = m.end()
    if text[pos:].strip():
        raise bad("nested braces or an unfinished declaration", text[pos:][:200])

    for d in decls:
        if m := _ENUM.fullmatch(d):
            for entry in m.group(1).split(","):
                e = _ENUM_ENTRY.fullmatch(entry)
                if not e:
                    raise bad("enum constant without an explicit integer value", entry)
                add(hdr.constants, e.group(1), int(e.group(2), 0), entry)
        elif m := _HANDLE.fullmatch(d):
            if m.group(1) not in _CTYPES:
                raise bad(f"unknown type {m.group(1)!r}", d)
        elif m := _STRUCT.fullmatch(d):
            fields = []
            for line in m.group(1).split(";"):
                t = _FIELD.fullmatch(line)
                for declarator in t.group(3).split(",") if t else [""]:
                    f = _DECLARATOR.fullmatch(declarator)
                    if not f or (f.group(3) and not f.group(1)):        # an array of anything but pointers is not in use
                        raise bad("not a field declaration", line)
                    if f.group(2) in [name for _, name, _ in fields]:
                        raise bad(f"field {f.group(2)} declared twice", line)
                    fields.append((ctype_name(t.group(1), t.group(2), f.group(1), line), f.group(2),
                                   int(f.group(3)) if f.group(3) else None))
            add(hdr.structs, m.group(2), fields, d)
        elif m := _PROTO.fullmatch(d):
            params = []
            for p in m.group(5).split(",") if m.group(5).strip() != "void" else []:
                q = _PARAM.fullmatch(p)
                if not q:
                    raise bad("not a parameter declaration", p)
                params.append((ctype_name(*q.group(1, 2, 3), p), q.group(4)))
            add(hdr.prototypes, m.group(4), (ctype_name(*m.group(1, 2, 3), d), params), d)
        else:
            raise bad("not a declaration this binding understands", d)
    return hdr


def _read_header():
    try:
        with open(HEADER_PATH) as f:
            text = f.read()
    except OSError as e:
        raise GdxError(f"cannot read the C ABI {HEADER_PATH}: {e}") from e
    return parse_header(text)


HEADER = _read_header()
STRUCTS = {}        # C name -> ctypes.Structure class, also a module attribute under its CamelCase name


def _ctype(t):
    if t == "const char*":
        return C.c_char_p
    base = t.removeprefix("const ").rstrip("*")
    if t.endswith("*"):
        return C.POINTER(STRUCTS[base]) if base in STRUCTS else C.c_void_p
    return _CTYPES[base]


def _class_name(c_name):
    """gdx_dpm_sde_step_args_t -> DpmSdeStepArgs"""
    return "".join(w.capitalize() for w in c_name.removeprefix("gdx_").removesuffix("_t").split("_"))


for _c_name, _fields in HEADER.structs.items():
    STRUCTS[_c_name] = type(_class_name(_c_name), (C.Structure,),
                            {"_fields_": [(f, _ctype(t) * n if n else _ctype(t)) for t, f, n in _fields]})
globals().update({cls.__name__: cls for cls in STRUCTS.values()})
globals().update(HEADER.constants)      # GDX_ROW_PAD, GDX_BPD_CHUNK, GDX_ARCH_*, GDX_COND ..., GDX_DTYPE_*, GDX_SAMPLER_*
EXPORTS = list(HEADER.prototypes)
SIGNATURES = {name: (_ctype(ret), [_ctype(t) for t, _ in params]) for name, (ret, params) in HEADER.prototypes.items()}

_lib = None


def load():
    """Load libgdx.so once; raise GdxError (never fall back) when it is unavailable."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise GdxError(f"HIP library not built: {LIB_PATH} is missing "
                       f"(run `python __graft_entry__.py` or `make -C gesturediffusion_amd/csrc`)")
    try:
        # torch ships its own HIP runtime; importing it first makes libgdx.so bind to that same
        # runtime instance, so torch's streams / device pointers are valid inside the library.
        import torch  # noqa: F401
        lib = C.CDLL(LIB_PATH)
    except OSError as e:  # missing libamdhip64, wrong arch ...
        raise GdxError(f"cannot load {LIB_PATH}: {e}") from e
    for name, (restype, argtypes) in SIGNATURES.items():
        fn = getattr(lib, name)
        fn.argtypes, fn.restype = argtypes, restype
    _lib = lib
    return lib


def check(rc, lib=None):
    if rc != 0:
        lib = lib or load()
        raise GdxError(lib.gdx_last_error().decode() or f"libgdx error {rc}")
