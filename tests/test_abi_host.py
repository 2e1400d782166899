"""The C ABI is declared once, in include/rrl.h, and rrl_hip/_abi.py reads it for the Python binding.  What the reader
makes of the header against what gcc makes of it (one probe program: every structure's size, every field's offset and size,
every constant), the built library's exports against the declarations, and the reader itself on small inline headers:
what it accepts and what it must refuse.  No GPU, no GPU call."""
import ctypes
import re
import subprocess

import pytest

from rrl_hip import _abi, _lib, build

STRUCTS = {"rrl_opts": "Opts", "rrl_chamfer_rider": "ChamferRider", "rrl_demo_epoch_args": "DemoEpochArgs",
           "rrl_register_epoch_args": "RegisterEpochArgs", "rrl_register_newton_args": "RegisterNewtonArgs",
           "rrl_kabsch_args": "KabschArgs", "rrl_icp_epoch_args": "IcpEpochArgs", "rrl_sinkhorn_args": "SinkhornArgs",
           "rrl_plane_args": "PlaneArgs", "rrl_plane_epoch_args": "PlaneEpochArgs"}


def gcc_probe(header, structs, constants, tmp):
    """{word: int} as gcc sees `header`: `S` sizeof, `S.f` offsetof, `S.f#` sizeof of every field of `structs`
    ({c_name: [(field, ...), ...]}), and every name of `constants`."""
    src = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{header}"', 'int main(void) {']
    for s, fields in structs.items():
        src.append(f'  printf("{s} %zu\\n", sizeof({s}));')
        src += [f'  printf("{s}.{f} %zu\\n{s}.{f}# %zu\\n", offsetof({s}, {f}), sizeof((({s} *)0)->{f}));' for f, *_ in fields]
    src += [f'  printf("{k} %lld\\n", (long long)({k}));' for k in constants]
    src += ['  return 0;', '}']
    (tmp / "abi.c").write_text("\n".join(src))
    subprocess.check_call(["gcc", "-std=c99", "-o", str(tmp / "abi"), str(tmp / "abi.c")])
    return {k: int(v) for k, v in (line.split() for line in subprocess.check_output([str(tmp / "abi")], text=True).splitlines())}


def assert_layout(got, c_name, cls):
    assert got[c_name] == ctypes.sizeof(cls), c_name
    for f, _ in cls._fields_:
        assert (got[f"{c_name}.{f}"], got[f"{c_name}.{f}#"]) == (getattr(cls, f).offset, getattr(cls, f).size), (c_name, f)
    if hasattr(cls, "struct_bytes"):
        assert cls.struct_bytes.offset == 0, c_name


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    return gcc_probe(build.HEADER, _abi.STRUCTS, _abi.CONSTANTS, tmp_path_factory.mktemp("abi"))


def test_abi_exports_match_header():
    header = open(build.HEADER).read()
    declared = sorted(set(re.findall(r"\b(rrl_[a-z0-9_]+)\s*\(", header)))  # (not the reader's own list: it must not lose one)
    assert len(declared) >= 17
    lib = ctypes.CDLL(build.build_lib())  # hipcc cross-compiles gfx950 without a GPU
    for name in declared:
        assert hasattr(lib, name), f"{name} declared in include/rrl.h but not exported"
    assert sorted(_lib.EXPORTS) == declared == sorted(_abi.PROTOS)
    assert set(_lib._SIGS) == {n for n, (res, _) in _abi.PROTOS.items() if res is ctypes.c_int}
    assert {n: res for n, (res, _) in _abi.PROTOS.items() if n not in _lib._SIGS} == dict(
        {n: ctypes.c_size_t for n in declared if n.endswith("_bytes")}, rrl_version=ctypes.c_char_p)
    lib.rrl_version.restype = ctypes.c_char_p
    assert b"gfx950" in lib.rrl_version()


def test_every_struct_matches_the_header_compiled_by_gcc(probe):
    """An ABI drift between include/rrl.h and the ctypes classes would silently shift pointers."""
    assert sorted(_abi.STRUCTS) == sorted(STRUCTS)
    for c_name, py_name in STRUCTS.items():
        cls = getattr(_lib, py_name)  # the names the package and the tests use: rrl_ stripped, CamelCase
        assert issubclass(cls, ctypes.Structure) and cls._fields_ == _abi.STRUCTS[c_name], c_name
        assert_layout(probe, c_name, cls)


def test_every_constant_matches_the_header_compiled_by_gcc(probe):
    assert len(_abi.CONSTANTS) >= 72
    for name, value in _abi.CONSTANTS.items():
        assert probe[name] == value, name
    mirrored = {k: v for k, v in vars(_lib).items() if k.isupper() and type(v) is int}  # F_*, FIT_*, PLANE_*, NEWTON_*, ...
    assert len(mirrored) >= 39 and {"F_CHAIN", "FIT_KEYMEAN", "MCTL_ERR", "PLANE_SKIPPED", "NEWTON_DONE", "ICP_DONE"} <= set(mirrored)
    for name, value in mirrored.items():
        assert _abi.CONSTANTS["RRL_" + name] == value, name


def test_opts_defaults_are_pinned():
    o = _lib.Opts()
    assert o.struct_bytes == ctypes.sizeof(_lib.Opts) and (o.flags, o.scan_counter_rows, o.problems) == (0, 0, 0)
    assert (o.reduce_mode, o.deterministic, o.sort_parts, o.scan_variant) == (-1, -1, -1, -1)
    assert all(getattr(o, f) is None for f, t in _lib.Opts._fields_ if t is ctypes.c_void_p)


# ---- the reader on inline headers ---------------------------------------------------------------------------------------
V, I = ctypes.c_void_p, ctypes.c_int


def test_reader_prototypes():
    protos, _, _ = _abi.parse("""
        /* a comment with int rrl_not_this(void); inside */
        int rrl_a(const float *x, long long dims[4], long long n, size_t bytes, double eps, float r, int32_t k, void *stream);
        size_t rrl_b(void);
        const char *rrl_c(const char **name,
                          int *out);  // over two lines
    """)
    assert protos == {"rrl_a": (I, [V, V, ctypes.c_longlong, ctypes.c_size_t, ctypes.c_double, ctypes.c_float, ctypes.c_int32, V]),
                      "rrl_b": (ctypes.c_size_t, []), "rrl_c": (ctypes.c_char_p, [V, V])}


def test_reader_structs():
    _, structs, _ = _abi.parse("""
        typedef struct rrl_inner { int32_t struct_bytes; uint64_t *best_x, *best_y; float *value; } rrl_inner;
        typedef struct rrl_outer {
            const int32_t *order1, *order2;  /* shared type, const */
            rrl_inner *inner; long long rows; double eps;
        } rrl_outer;
        int rrl_use(const rrl_outer *args, void *stream);
    """)
    assert structs == {"rrl_inner": [("struct_bytes", ctypes.c_int32), ("best_x", V), ("best_y", V), ("value", V)],
                       "rrl_outer": [("order1", V), ("order2", V), ("inner", V), ("rows", ctypes.c_longlong), ("eps", ctypes.c_double)]}


def test_reader_constants():
    _, _, constants = _abi.parse("""
        #ifndef RRL_H
        #define RRL_H
        #include <stddef.h>
        #ifdef __cplusplus
        extern "C" {
        #endif
        #define RRL_FOUR 4 /* a literal */
        #define RRL_E (-1)
        #define RRL_HEX 0x10
        #define RRL_SAME RRL_FOUR
        #define RRL_AGAIN RRL_SAME
        #define RRL_TABLE(X) \\
            X(A, int32_t, 4) \\
            X(B, float, RRL_FOUR)
        #define RRL_ENUM_(name, type, ...) RRL_F_##name,
        enum { RRL_TABLE(RRL_ENUM_) RRL_F_FIELDS };
        enum { RRL_ZERO, RRL_ONE, RRL_SEVEN = 7, RRL_EIGHT, RRL_TWENTY = 20, RRL_NEXT, RRL_LIKE = RRL_FOUR, RRL_FIVE };
        #ifdef __cplusplus
        }
        #endif
        #endif
    """)
    assert constants == dict(RRL_FOUR=4, RRL_E=-1, RRL_HEX=16, RRL_SAME=4, RRL_AGAIN=4, RRL_ZERO=0, RRL_ONE=1, RRL_SEVEN=7, RRL_EIGHT=8,
                             RRL_TWENTY=20, RRL_NEXT=21, RRL_LIKE=4, RRL_FIVE=5)  # (the enum made by a macro: skipped, by that rule)


@pytest.mark.parametrize("text, names", [
    ("int rrl_a(unsigned n);", "unsigned n"),  # an unknown type word
    ("int rrl_a(int64_t n);", "int64_t"),  # known behind a pointer only
    ("int rrl_a(foo_t *p);", "foo_t"),  # ... and unknown even there
    ("int rrl_a(int);", "int"),  # no name
    ("int rrl_a(int (*callback)(int));", "rrl_a"),  # a declarator it cannot split
    ("typedef struct rrl_s { int a; long b; } rrl_s;", "long b"),
    ("typedef struct rrl_s { int a, int b; } rrl_s;", "int b"),
    ("typedef struct rrl_s { int a; };", "rrl_s"),  # the trailing name is missing
    ("typedef struct rrl_s { int a; } rrl_t;", "rrl_s"),  # ... or another
    ("typedef struct rrl_s { rrl_later *p; } rrl_s;", "rrl_later"),
    ("float rrl_a(void);", "rrl_a"),  # a return type the binding does not know
    ("int *rrl_a(void);", "rrl_a"),
    ("static int x;", "static int x"),  # no declaration of the ABI
    ("int rrl_a(void) { return 0; }", "rrl_a"),
    ("#define RRL_M(x) (x)\n#define RRL_A RRL_M(3)\n", "RRL_A"),  # a function-like macro used as a constant
    ("#define RRL_M(x) (x)\n#define RRL_A RRL_M\n", "RRL_A"),
    ("#define RRL_A RRL_LATER\n#define RRL_LATER 1\n", "RRL_A"),
    ("#define RRL_A 1 + 2\n", "RRL_A"),
    ("#define RRL_A 1.5\n", "RRL_A"),
    ("enum { RRL_A = 1 << 2 };", "RRL_A"),
    ("enum { RRL_A = RRL_UNKNOWN };", "RRL_A"),
    ("#if 0\nint rrl_a(void);\n#endif\n", "#if 0"),  # a declaration that may not be there
    ("#ifdef RRL_X\nint rrl_a(void);\n#endif\n", "#ifdef RRL_X"),
])
def test_reader_refuses_what_it_does_not_know(text, names):
    """Nothing is skipped and nothing defaults to int: ValueError, naming the declaration."""
    with pytest.raises(ValueError, match=re.escape(names)) as err:
        _abi.parse(text)
    assert "include/rrl.h" in str(err.value)
