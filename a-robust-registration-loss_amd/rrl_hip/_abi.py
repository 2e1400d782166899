"""The C ABI as include/rrl.h declares it, read once per process: the Python binding's only source.

PROTOS     {name: (restype, [argtypes])} of every `TYPE rrl_name(args);`
STRUCTS    {c_name: [(field, ctype), ...]} of every `typedef struct NAME {...} NAME;`
CONSTANTS  {RRL_NAME: int} of the object-like `#define`s and the enumerators

The accepted grammar is what the header uses today, and nothing more.  Comments; `#include`, `#ifndef`, `#endif`, an
`#ifdef __cplusplus` block (dropped: this is the C view), `#define`.  An object-like `#define RRL_X` whose body is an
integer literal, a parenthesised one or an earlier RRL_ name is a constant, one with an empty body is none (the include
guard, `#ifndef RRL_H`), function-like macros are ignored, any other body or directive raises.  At file scope only the three declarations above and
`enum { NAME [= integer | RRL_NAME], ... };`.  A parameter or field is `[const] TYPE [*...] name [[n]]` with TYPE one
of _SCALARS, void, char or a struct declared earlier; fields may share a type (`uint64_t *best_x, *best_y;`).  Any
pointer or array is a c_void_p; only a return type tells `const char *` apart.  Everything else raises ValueError
naming the declaration -- nothing is skipped and nothing defaults to int -- so whoever adds a new form to the header
extends this parser in the same commit.
"""
import ctypes
import re

from .build import HEADER

_SCALARS = {"int": ctypes.c_int, "int32_t": ctypes.c_int32, "size_t": ctypes.c_size_t, "long long": ctypes.c_longlong,
            "double": ctypes.c_double, "float": ctypes.c_float}
_POINTEES = {"void", "char", "uint8_t", "int64_t", "uint64_t"}  # met behind a `*` only
_INT = r"-?(?:0[xX][0-9a-fA-F]+|\d+)"


def _declarator(decl, structs, base=None):
    """`[const] TYPE [*...] name [[n]]` -> (name, ctype, TYPE); `base`: the TYPE of a field list's later declarators."""
    m = re.fullmatch(r"((?:\w+\s+)*)((?:\*\s*)*)(\w+)\s*(\[\w*\])?", decl.strip())
    words = [w for w in m.group(1).split() if w != "const"] if m else []
    kind = " ".join(words) or base
    if not m or (words and base) or kind not in _SCALARS and kind not in _POINTEES and kind not in structs:
        raise ValueError(f"include/rrl.h: cannot read the declarator `{decl.strip()}`")
    if m.group(2) or m.group(4):
        return m.group(3), ctypes.c_void_p, kind
    if kind not in _SCALARS:
        raise ValueError(f"include/rrl.h: `{decl.strip()}` passes a `{kind}` by value")
    return m.group(3), _SCALARS[kind], kind


def _fields(body, structs):
    out = []
    for decl in filter(str.strip, body.split(";")):
        base = None
        for part in decl.split(","):
            name, ctype, base = _declarator(part, structs, base)
            out.append((name, ctype))
    return out


def _value(text, constants, where):
    text = text.strip()
    while text.startswith("(") and text.endswith(")"):
        text = text[1:-1].strip()
    if re.fullmatch(_INT, text):
        return int(text, 0)
    if re.fullmatch(r"RRL_\w+", text) and text in constants:
        return constants[text]
    raise ValueError(f"include/rrl.h: `{where.strip()}` is no integer, (integer) or earlier RRL_ constant")


def _enum(body, constants):
    if re.search(r"\w\s*\(", body):
        return  # the body invokes a macro: the two X-macro field enums, whose rows rrl_workspace_field describes to Python
    value = -1
    for item in filter(str.strip, body.split(",")):
        name, eq, explicit = (x.strip() for x in item.partition("="))
        if not re.fullmatch(r"RRL_\w+", name):
            raise ValueError(f"include/rrl.h: cannot read the enumerator `{item.strip()}`")
        value = constants[name] = _value(explicit, constants, item) if eq else value + 1


def parse(text):
    """(PROTOS, STRUCTS, CONSTANTS) of a header's text."""
    protos, structs, constants = {}, {}, {}
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)
    text = re.sub(r"^[ \t]*#[ \t]*ifdef[ \t]+__cplusplus\b.*?^[ \t]*#[ \t]*endif\b[^\n]*$", "", text, flags=re.S | re.M)

    def directive(m):
        line = m.group(0).replace("\\\n", " ")
        d = re.fullmatch(r"\s*#\s*define\s+(\w+)(\(?)(.*)", line, flags=re.S)
        if d and not d.group(2) and d.group(3).strip():  # object-like and not empty: a constant, or an error
            constants[d.group(1)] = _value(d.group(3), constants, line)
        elif not d and not re.match(r"\s*#\s*(include|ifndef\s+RRL_H|endif)\b", line):
            raise ValueError(f"include/rrl.h: unknown preprocessor line `{line.strip()}`")
        return ""
    text = re.sub(r"^[ \t]*#(?:[^\n\\]|\\\n|\\.)*$", directive, text, flags=re.M)

    declaration = re.compile(r"\s*(?:typedef\s+struct\s+(\w+)\s*\{([^{}]*)\}\s*(\w*)\s*;"  # 1, 2, 3
                             r"|enum\s*\{([^{}]*)\}\s*;"  # 4
                             r"|([\w\s*]+?)\b(rrl_\w+)\s*\(([^(){};]*)\)\s*;)")  # 5, 6, 7
    pos = 0
    while text[pos:].strip():
        m = declaration.match(text, pos)
        if not m:
            raise ValueError(f"include/rrl.h: cannot read the declaration `{' '.join(text[pos:].split())[:80]}`")
        pos = m.end()
        if m.group(1):
            if m.group(3) != m.group(1):
                raise ValueError(f"include/rrl.h: typedef struct {m.group(1)} must end in `}} {m.group(1)};`")
            structs[m.group(1)] = _fields(m.group(2), structs)
        elif m.group(4) is not None:
            _enum(m.group(4), constants)
        else:
            ret = " ".join(m.group(5).split())
            if ret not in ("int", "size_t", "const char *"):
                raise ValueError(f"include/rrl.h: {m.group(6)} returns `{ret}`: not int, size_t or const char *")
            args = m.group(7).strip()
            argtypes = [] if args == "void" else [_declarator(a, structs)[1] for a in args.split(",")]
            protos[m.group(6)] = (ctypes.c_char_p if "*" in ret else _SCALARS[ret], argtypes)
    return protos, structs, constants


with open(HEADER) as _f:
    PROTOS, STRUCTS, CONSTANTS = parse(_f.read())
