"""CPU: libcvcl_hip.so builds, loads and exports every symbol include/cvcl_hip.h declares; the binding multimodal/_hip.py derives
from that header is what the compiler reads in it (arity, argument kinds, struct layouts, constants); argument validation answers
without touching a GPU; the product path refuses CPU tensors (no fallback)."""
import ctypes as C
import importlib.util
import os
import re
import subprocess

import pytest
import torch

from conftest import ROOT


def _declared():
    txt = open(os.path.join(ROOT, "include", "cvcl_hip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(cvcl_[a-z0-9_]+)\s*\(", txt)))


def _build_module():
    spec = importlib.util.spec_from_file_location("cvcl_build", os.path.join(ROOT, "multimodal-baby_amd", "build.py"))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    return b


@pytest.fixture(scope="module")
def lib():
    _build_module().build(verbose=False)
    from multimodal import _hip
    return _hip


def test_every_declared_symbol_is_bound_and_exported(lib):
    declared = _declared()
    assert declared, "header parse failed"
    assert sorted(lib.SIGNATURES.keys()) == declared
    l = lib.load()
    for name in declared:
        assert hasattr(l, name), name
    assert l.cvcl_abi_version() == lib.ABI_VERSION


def test_argument_validation_without_gpu(lib):
    l = lib.load()
    a = lib.GemmArgs()
    assert l.cvcl_gemm(lib.F32, a, None) == -1            # CVCL_EINVAL: null operands
    assert b"null" in l.cvcl_last_error()
    assert l.cvcl_l2norm_fwd(None, None, None, 0, 0, 1e-12, None) == -1
    assert l.cvcl_infonce_workspace_bytes(256) == 6 * 256 * 4


def test_no_cpu_fallback(lib):
    from multimodal import ops
    with pytest.raises(lib.CvclError):
        ops.l2_normalize(torch.randn(4, 8))
    with pytest.raises(lib.CvclError):
        lib.gemm(torch.randn(4, 8), torch.randn(4, 8))


# ---- the derived binding against the compiler ----
# One letter per kind of C type.  ctypes has one class for long / int64_t / long long and one for size_t / unsigned long /
# unsigned long long (they are the same machine types on this ABI), so each of those groups shares a letter; a pointer to one
# of the header's structs gets that struct's own letter, every other pointer 'p'.
_KIND = {C.c_int: "i", C.c_long: "l", C.c_ulong: "m", C.c_float: "f", C.c_double: "d", C.c_void_p: "p", C.c_char_p: "p"}
_UNIT_HEAD = """#include <cstddef>
#include <type_traits>
#include "cvcl_hip.h"
template <class T> constexpr char kind() {
    using U = std::remove_cv_t<std::remove_pointer_t<T>>;
    if constexpr (std::is_pointer_v<T>) {
%s        return 'p';
    } else if constexpr (std::is_same_v<T, int>) return 'i';
    else if constexpr (std::is_same_v<T, long> || std::is_same_v<T, long long>) return 'l';
    else if constexpr (std::is_same_v<T, unsigned long> || std::is_same_v<T, unsigned long long>) return 'm';
    else if constexpr (std::is_same_v<T, float>) return 'f';
    else if constexpr (std::is_same_v<T, double>) return 'd';
    else return '?';
}
template <class R, class... A> constexpr bool same(R (*)(A...), const char* want) {
    const char got[] = {kind<R>(), kind<A>()..., 0};
    for (int i = 0;; ++i) {
        if (got[i] != want[i]) return false;
        if (!got[i]) return true;
    }
}
"""


def _abi_unit(consts, structs, sigs):
    """A C++ translation unit of static_asserts: what these tables say about cvcl_hip.h, for the compiler to judge."""
    letter = {cls: chr(ord("A") + i) for i, cls in enumerate(structs.values())}

    def kind(t):
        return letter[t._type_] if hasattr(t, "contents") else _KIND[t]

    out = [_UNIT_HEAD % "".join(f"        if constexpr (std::is_same_v<U, {n}>) return '{letter[c]}';\n" for n, c in structs.items())]
    out += [f'static_assert({n} == {v}, "{n}");' for n, v in consts.items()]
    for n, cls in structs.items():
        out.append(f'static_assert(sizeof({n}) == {C.sizeof(cls)}, "sizeof {n}");')
        for f, t in cls._fields_:
            out.append(f'static_assert(offsetof({n}, {f}) == {getattr(cls, f).offset} && kind<decltype({n}::{f})>() == \'{kind(t)}\', "{n}.{f}");')
    out += [f'static_assert(same(&{n}, "{kind(res)}{"".join(map(kind, args))}"), "{n}");' for n, (res, args) in sigs.items()]
    return "\n".join(out) + "\n"


def _syntax_check(path, unit):
    path.write_text(unit)
    return subprocess.run([_build_module().HIPCC, "-x", "c++", "-std=c++17", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(path)],
                          capture_output=True, text=True)


def test_compiler_agrees_with_the_derived_binding(tmp_path):
    from multimodal import _hip as H
    assert len(H.SIGNATURES) > 150 and len(H.STRUCTS) == 3 and len(H.CONSTANTS) > 40        # the unit is not vacuous
    r = _syntax_check(tmp_path / "abi.cpp", _abi_unit(H.CONSTANTS, H.STRUCTS, H.SIGNATURES))
    assert r.returncode == 0, r.stderr
    # the same unit refuses tables that are off in one place: an argument kind, an arity, a field order, a constant
    gemm, rows = H.SIGNATURES["cvcl_gemm"], H.SIGNATURES["cvcl_col_stats_rows"]
    fields = list(H.GemmFp8Args._fields_)
    fields[3], fields[4] = fields[4], fields[3]                                        # int lda <-> const void* W8
    swapped = type("cvcl_gemm_fp8_args", (C.Structure,), {"_fields_": fields})
    for what, (consts, structs, sigs) in {
        "cvcl_col_stats_rows": (H.CONSTANTS, H.STRUCTS, dict(H.SIGNATURES, cvcl_col_stats_rows=(rows[0], [C.c_int]))),   # long as int
        "cvcl_gemm": (H.CONSTANTS, H.STRUCTS, dict(H.SIGNATURES, cvcl_gemm=(gemm[0], gemm[1][:-1]))),
        "cvcl_gemm_fp8_args.lda": (H.CONSTANTS, dict(H.STRUCTS, cvcl_gemm_fp8_args=swapped), {}),
        "CVCL_STATS_ACCUMULATE": (dict(H.CONSTANTS, CVCL_STATS_ACCUMULATE=1), H.STRUCTS, {}),
    }.items():
        r = _syntax_check(tmp_path / "off.cpp", _abi_unit(consts, structs, sigs))
        assert r.returncode != 0 and re.search(rf'static[_ ]assert(ion)? failed[^\n]*"?{re.escape(what)}\b', r.stderr), (what, r.stderr[-2000:])


def test_kernel_classes_match_enum():
    from multimodal import _hip as H
    classes = sorted((v, k) for k, v in H.CONSTANTS.items() if k.startswith("CVCL_K_") and k != "CVCL_K_NCLASSES")
    assert [v for v, _ in classes] == list(range(H.CONSTANTS["CVCL_K_NCLASSES"]))              # dense, 0 .. NCLASSES - 1
    assert len(H.KERNEL_CLASSES) == H.CONSTANTS["CVCL_K_NCLASSES"] == len(classes) and len(set(H.KERNEL_CLASSES)) == len(classes)
    # where bench.py's names are the enum's own they sit at the enum's index
    for v, k in classes:
        name = k[len("CVCL_K_"):].lower()
        if name in H.KERNEL_CLASSES:
            assert H.KERNEL_CLASSES.index(name) == v, k


# ---- the header parser on literal snippets (no file, no library) ----
def test_parser_reads_the_header_dialect():
    from multimodal import _hip as H
    consts, structs, sigs = H.parse_header("""
        #ifndef SNIPPET_H
        #define SNIPPET_H
        #include <stdint.h>
        #ifdef __cplusplus
        extern "C" {
        #endif
        #define X (-1)
        #define Y 7   /* a trailing comment; with a semicolon */
        enum { A = 0, B = 5, C, D = -2 };
        typedef struct {
            const void* A; const void* W; void* C;
            int M, N, K;    /* a comment; with a semicolon, and a comma */
            const float* scale; float eps; int64_t* n; long rows;
            // a line comment; int not_a_field;
            double *p, q;
        } blk;
        int
        f(int dtype, const blk* args,
          const float* centre /* [64] or NULL */, long rows, size_t bytes, unsigned long long seed, int64_t n, double alpha,
          float eps, const double** out, void* stream);
        const char* last_error(void);
        size_t ws_bytes(int);
        #ifdef __cplusplus
        }
        #endif
        #endif
    """)
    assert consts == {"X": -1, "Y": 7, "A": 0, "B": 5, "C": 6, "D": -2}
    P = C.c_void_p
    assert list(structs) == ["blk"] and structs["blk"]._fields_ == [
        ("A", P), ("W", P), ("C", P), ("M", C.c_int), ("N", C.c_int), ("K", C.c_int), ("scale", P), ("eps", C.c_float), ("n", P),
        ("rows", C.c_long), ("p", P), ("q", C.c_double)]
    assert sigs == {"f": (C.c_int, [C.c_int, C.POINTER(structs["blk"]), P, C.c_long, C.c_size_t, C.c_ulonglong, C.c_int64, C.c_double,
                                    C.c_float, P, P]),
                    "last_error": (C.c_char_p, []), "ws_bytes": (C.c_size_t, [C.c_int])}


@pytest.mark.parametrize("snippet,named", [
    ("int f(short x);", "short x"),                                    # a type outside the map
    ("int f(unsigned x);", "unsigned x"),
    ("int f(long long);", "long long"),
    ("typedef struct { int a; } s; int f(s by_value);", "s by_value"),
    ("typedef struct { int a; } s; typedef struct { s inner; } t;", "s inner"),
    ("typedef struct { int a; } s; s f(void);", "s"),
    ("int f(int (*callback)(int));", "int (*callback)(int)"),
    ("int f(const char* fmt, ...);", "..."),
    ("int f();", "''"),
    ("void f(int x);", "void"),
    ("typedef struct { int a[4]; } s;", "int a[4]"),
    ("typedef struct { int a : 3; } s;", "int a : 3"),
    ("typedef struct { int; } s;", "int"),
    ("struct s { int a; };", "struct s { int a; }"),
    ("extern int counter;", "extern int counter"),
    ("typedef int handle;", "typedef int handle"),
    ("enum { A = 1 << 3 };", "A = 1 << 3"),
    ("#define SCALE 1.5", "#define SCALE 1.5"),
    ("#define SQ(x) ((x) * (x))", "#define SQ(x) ((x) * (x))"),
    ("#if 0\nint f(void);\n#endif", "#if 0"),
    ("int f(void)", "int f(void)"),                                     # no terminating semicolon
    ("int f(void) { return 0; }", "int f(void) { return 0; }"),
])
def test_parser_refuses_what_it_cannot_classify(snippet, named):
    from multimodal import _hip as H
    with pytest.raises(H.CvclError) as e:
        H.parse_header(snippet)
    assert named in str(e.value)


def test_missing_header_is_an_error(monkeypatch, tmp_path):
    from multimodal import _hip as H
    monkeypatch.setattr(H, "HEADER_PATH", str(tmp_path / "include" / "cvcl_hip.h"))
    with pytest.raises(H.CvclError, match=re.escape(str(tmp_path / "include" / "cvcl_hip.h"))):
        H._read_header()
