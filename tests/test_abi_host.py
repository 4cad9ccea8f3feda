"""The C ABI (include/gdx.h) against its ctypes binding (gesturediffusion_amd/_lib.py), whole, no GPU needed: the header parser on
strings, then every struct's layout and every prototype confirmed by a C compiler, every argtypes list against the type table,
and the library's exported symbols against the declared ones in both directions."""
import ctypes as C
import os
import re
import subprocess

import pytest

from conftest import REPO
from gesturediffusion_amd import _lib
from gesturediffusion_amd._lib import parse_header

HDR = open(os.path.join(REPO, "include", "gdx.h")).read()
BARE = re.sub(r"/\*.*?\*/|//[^\n]*", " ", HDR, flags=re.S)         # without comments: what the tests count in, without the parser
# the type table of the binding, restated: a wrong entry in _lib._CTYPES must not confirm itself
SCALARS = {"int32_t": C.c_int32, "int64_t": C.c_int64, "uint32_t": C.c_uint32, "uint64_t": C.c_uint64, "uint8_t": C.c_uint8,
           "float": C.c_float, "double": C.c_double, "int": C.c_int, "gdx_handle_t": C.c_void_p}
CLASSES = {C.c_float: "float", C.c_double: "double", C.c_int32: "int32_t", C.c_int64: "int64_t", C.c_uint32: "uint32_t",
           C.c_uint64: "uint64_t"}       # what the probe's _Generic tells apart; pointers and arrays are "default"


def table_ctype(t):
    base = t.replace("const ", "").rstrip("*")
    if not t.endswith("*"):
        return SCALARS[base]
    return C.c_char_p if t == "const char*" else C.POINTER(_lib.STRUCTS[base]) if base in _lib.STRUCTS else C.c_void_p


def compile_c(tmp_path, source, *flags):
    cc = next((c for c in ("cc", "gcc", "clang", "/opt/rocm/llvm/bin/clang") if subprocess.run(
        ["sh", "-c", f"command -v {c}"], capture_output=True).returncode == 0), None)
    assert cc, "no C compiler"
    (tmp_path / "probe.c").write_text(source)
    return subprocess.run([cc, "-std=c11", "-Werror", "-I", os.path.join(REPO, "include"), str(tmp_path / "probe.c"), *flags],
                          capture_output=True, text=True)


# ---------------------------------------------------------------------------------------------------- the parser, on strings
def test_parser_accepts_every_form_the_header_uses():
    h = parse_header('''/* a block
        comment; with { braces */
        #ifndef X_H
        #define X_H
        #include <stdint.h>
        #ifdef __cplusplus
        extern "C" {
        #endif
        typedef struct gdx_model* gdx_handle_t;   // a line comment
        #define GDX_N 0x10
        enum { GDX_A = 1,  /* why */
               GDX_B = -2 };
        typedef struct {
            int32_t batch, njoints;
            const float *a, *b;
            const int64_t* t;      /* [B] */
            const float* eps[4];
            float* out; uint64_t seed;
            gdx_handle_t h;
        } gdx_one_args_t;
        int gdx_one(const gdx_one_args_t* a,
                    void* stream);
        const char* gdx_text(void);
        int gdx_two(gdx_handle_t h, const char* name, int64_t* n, gdx_handle_t* out, float phi);
        #ifdef __cplusplus
        }
        #endif
        #endif /* X_H */''')
    assert h.constants == {"GDX_N": 16, "GDX_A": 1, "GDX_B": -2}
    assert h.structs == {"gdx_one_args_t": [
        ("int32_t", "batch", None), ("int32_t", "njoints", None), ("const float*", "a", None), ("const float*", "b", None),
        ("const int64_t*", "t", None), ("const float*", "eps", 4), ("float*", "out", None), ("uint64_t", "seed", None),
        ("gdx_handle_t", "h", None)]}
    assert list(h.prototypes.items()) == [
        ("gdx_one", ("int", [("const gdx_one_args_t*", "a"), ("void*", "stream")])), ("gdx_text", ("const char*", [])),
        ("gdx_two", ("int", [("gdx_handle_t", "h"), ("const char*", "name"), ("int64_t*", "n"), ("gdx_handle_t*", "out"),
                             ("float", "phi")]))]
    assert parse_header("") == ({}, {}, {})


@pytest.mark.parametrize("text, names", [
    ("typedef struct { size_t n; } a_t;", "unknown type 'size_t'.*size_t n"),
    ("int gdx_f(unsigned n);", "unknown type 'unsigned'.*unsigned n"),
    ("int gdx_f(long n);", "unknown type 'long'"),
    ("typedef struct { int32_t a; struct { float x; } in; } a_t;", "nested braces.*struct { float x"),
    ("typedef struct { int32_t a; } a_t; typedef struct { a_t in; } b_t;", "struct a_t by value.*a_t in"),
    ("typedef struct { struct foo in; } a_t;", "not a field declaration.*struct foo in"),
    ("typedef struct { int32_t a : 3; } a_t;", "not a field declaration.*a : 3"),
    ("typedef struct { int (*fn)(int); } a_t;", r"not a field declaration.*\(\*fn\)"),
    ("typedef struct { float x[4]; } a_t;", r"not a field declaration.*x\[4\]"),
    ("typedef struct { float** x; } a_t;", r"not a field declaration.*\*\* x"),
    ("typedef struct { int32_t a; int32_t a; } a_t;", "field a declared twice"),
    ("typedef struct { int32_t a } a_t;", "not a declaration.*int32_t a }"),
    ("typedef struct { } a_t;", "not a declaration.*a_t"),
    ("typedef union { float f; int32_t i; } u_t;", "not a declaration.*typedef union"),
    ("typedef struct { union { float f; int32_t i; } u; } a_t;", "nested braces.*union"),
    ("typedef struct gdx_other* gdx_other_t;", "unknown type 'gdx_other_t'"),
    ("typedef int32_t gdx_index_t;", "not a declaration.*gdx_index_t"),
    ("enum { GDX_A, GDX_B = 1 };", "without an explicit integer value.*GDX_A"),
    ("enum { GDX_A = GDX_B + 1 };", "without an explicit integer value.*GDX_B"),
    ("enum gdx_kind { GDX_A = 0 };", "not a declaration.*enum gdx_kind"),
    ("#define GDX_F 1.5f", "unknown directive.*GDX_F"),
    ("#define GDX_SQ(x) ((x)*(x))", "unknown directive.*GDX_SQ"),
    ("#include <stddef.h>", "unknown directive.*stddef"),
    ("#if 0\n#endif", "unknown directive.*#if 0"),
    ("#define GDX_N 1\n#define GDX_N 2", "GDX_N declared twice"),
    ("int gdx_f(void); int gdx_f(void);", "gdx_f declared twice"),
    ("int gdx_f(int32_t);", "not a parameter.*int32_t"),
    ("int gdx_f(int32_t a, ...);", r"not a parameter.*\.\.\."),
    ("int gdx_f(int (*cb)(int), void* s);", "not a declaration|not a parameter"),
    ("gdx_f(void);", "not a declaration.*gdx_f"),
    ("static inline int gdx_f(void) { return 0; }", "unfinished declaration.*static inline"),
    ("extern int gdx_count;", "not a declaration.*gdx_count"),
    ("int gdx_f(void)", "unfinished declaration.*gdx_f"),
    ("int gdx_f(void); /* no end", "unterminated comment.*no end"),
])
def test_parser_refuses_what_it_does_not_understand(text, names):
    with pytest.raises(ValueError, match=names):
        parse_header(text)


def test_binding_names_and_constants_come_from_the_header(tmp_path, monkeypatch):
    assert [c.__name__ for c in _lib.STRUCTS.values()] == [
        "Config", "CfgRescaleArgs", "CfgDeltaArgs", "UpdateArgs", "PlmsArgs", "PlmsStepArgs", "DpmStepArgs", "DpmSdeStepArgs",
        "UnipcStepArgs", "LoopArgs", "BpdArgs", "BpdLoopArgs", "PlmsLoopArgs", "DpmLoopArgs", "DpmSdeLoopArgs", "UnipcLoopArgs"]
    assert all(getattr(_lib, c.__name__) is c for c in _lib.STRUCTS.values())
    consts = {n: int(v) for n, v in re.findall(r"#define (GDX_\w+) (\d+)", BARE) + re.findall(r"\b(GDX_\w+) = (\d+)", BARE)}
    assert consts and consts == _lib.HEADER.constants and all(getattr(_lib, n) == v for n, v in consts.items())
    assert (_lib.GDX_BPD_CHUNK, _lib.GDX_ROW_PAD, _lib.GDX_CFG, _lib.GDX_SAMPLER_DDIM, _lib.GDX_ARCH_MDM) == (4096, 256, 2, 1, 2)
    from gesturediffusion_amd import engine
    assert engine.COMPUTE_DTYPES == {"fp32": 0, "fp16": 1, "bf16": 2}
    monkeypatch.setattr(_lib, "HEADER_PATH", str(tmp_path / "include" / "gdx.h"))
    with pytest.raises(_lib.GdxError, match=re.escape(str(tmp_path / "include" / "gdx.h"))):
        _lib._read_header()


def test_header_states_the_rules_the_samplers_rely_on():
    """Sentences of the header that tests of the guidance features lean on (they moved here with the symbol checks)."""
    assert "token-major" in HDR[HDR.index("int gdx_set_guidance_interval"):HDR.index("int gdx_set_guidance_rescale")]
    rule = HDR[HDR.index("int gdx_cfg_rescale("):HDR.index("int gdx_set_guidance_refresh(")]
    for word in ("n % every == 0", "token-major", "trained", "gdx_bpd_loop", "block-wise"):
        assert word in rule, word


# ------------------------------------------------------------------------------------------- layout, checked by the compiler
def test_every_struct_and_field_has_the_compilers_layout(tmp_path):
    bodies = re.findall(r"typedef struct \{(.*?)\}", BARE, re.S)
    structs = _lib.HEADER.structs
    assert len(structs) == len(bodies) == HDR.count("typedef struct {") > 0
    assert [len(f) for f in structs.values()] == [b.count(";") + b.count(",") for b in bodies]
    lines, want = [], []
    for name, fields in structs.items():
        cls = _lib.STRUCTS[name]
        assert [f for f, _ in cls._fields_] == [f for _, f, _ in fields]
        lines.append(f'printf("{name} %zu\\n", sizeof({name}));')
        want.append(f"{name} {C.sizeof(cls)}")
        for (t, f, n), (_, ct) in zip(fields, cls._fields_):
            assert ct is (table_ctype(t) * n if n else table_ctype(t)), (name, f)      # ctypes caches array types
            lines.append(f'printf("{name}.{f} %zu %zu %s\\n", offsetof({name}, {f}), sizeof((({name}*)0)->{f}), '
                         f'CLASS((({name}*)0)->{f}));')
            want.append(f"{name}.{f} {getattr(cls, f).offset} {getattr(cls, f).size} {CLASSES.get(ct, 'default')}")
    probe = ('#include <stddef.h>\n#include <stdio.h>\n#include "gdx.h"\n#define CLASS(x) _Generic((x), float: "float", '
             'double: "double", int32_t: "int32_t", int64_t: "int64_t", uint32_t: "uint32_t", uint64_t: "uint64_t", '
             'default: "default")\nint main(void) {\n' + "\n".join(lines) + "\nreturn 0; }\n")
    built = compile_c(tmp_path, probe, "-o", str(tmp_path / "probe"))
    assert built.returncode == 0, built.stderr
    got = subprocess.run([str(tmp_path / "probe")], check=True, capture_output=True, text=True).stdout.splitlines()
    assert got == want and len(want) == len(structs) + sum(len(f) for f in structs.values())


# --------------------------------------------------------------------------------------- prototypes, checked by the compiler
def prototype_probe(prototypes):
    return '#include "gdx.h"\n' + "".join(f"static {ret} (*p_{name})({', '.join(t for t, _ in params) or 'void'}) = {name};\n"
                                          for name, (ret, params) in prototypes.items()) + "int main(void) { return 0; }\n"


def test_every_prototype_has_the_parsed_parameter_types(tmp_path):
    protos = _lib.HEADER.prototypes
    assert list(protos) == _lib.EXPORTS == re.findall(r"\b(gdx_[a-z0-9_]+)\s*\(", BARE)
    built = compile_c(tmp_path, prototype_probe(protos), "-c", "-o", str(tmp_path / "probe.o"))
    assert built.returncode == 0, built.stderr
    # negative controls: one parameter dropped, two parameters of different types swapped
    ret, params = protos["gdx_get_tap"]
    for wrong in (params[:-1], [params[0], params[2], params[1]] + params[3:]):
        built = compile_c(tmp_path, prototype_probe({**protos, "gdx_get_tap": (ret, wrong)}), "-c", "-o", str(tmp_path / "probe.o"))
        assert built.returncode != 0 and "p_gdx_get_tap" in built.stderr, built.stderr


def test_every_signature_follows_the_type_table():
    assert list(_lib.SIGNATURES) == _lib.EXPORTS
    for name, (ret, params) in _lib.HEADER.prototypes.items():
        restype, argtypes = _lib.SIGNATURES[name]
        assert restype is table_ctype(ret) and len(argtypes) == len(params), name
        assert all(a is table_ctype(t) for a, (t, _) in zip(argtypes, params)), name
    assert _lib.SIGNATURES["gdx_last_error"] == (C.c_char_p, [])
    assert _lib.SIGNATURES["gdx_create"] == (C.c_int, [C.POINTER(_lib.Config), C.c_void_p])


# ------------------------------------------------------------------------------------------------------------ the library
def test_library_exports_exactly_the_declared_symbols():
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libgdx.so not built (run python __graft_entry__.py)")
    syms = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], check=True, capture_output=True, text=True).stdout
    assert _lib.EXPORTS
    for n in _lib.EXPORTS:
        assert f" T {n}\n" in syms, n
    # names ending in '_' are the library's internal convention (gdx_set_error_); nothing else may be exported undeclared
    exported = {s for s in re.findall(r"^\S+ \w (gdx_\w+)$", syms, re.M) if not s.endswith("_")}
    assert exported == set(_lib.EXPORTS)
    lib = _lib.load()                                       # loads on a CPU-only box (no compute calls)
    assert lib.gdx_last_error() is not None
    for name, (restype, argtypes) in _lib.SIGNATURES.items():
        fn = getattr(lib, name)
        assert (fn.restype, list(fn.argtypes)) == (restype, argtypes), name
