"""A ctypes mirror of a struct of include/rrl.h against the header compiled by gcc (no GPU, no library)."""
import ctypes
import os
import subprocess

from conftest import ROOT


def assert_struct_matches_header(cls, name, tmp_path, extra_printf=()):
    """Same size, same offset of every field of ctypes class `cls` and C struct `name`; struct_bytes first, like
    rrl_demo_epoch_args.  extra_printf: further C statements of the probe program; returns its output as {first word:
    second word} so that the caller can check what they printed."""
    src = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{os.path.join(ROOT, "include", "rrl.h")}"', 'int main(void) {',
           f'  printf("{name} %zu\\n", sizeof({name}));']
    src += [f'  printf("{name}.{f} %zu\\n", offsetof({name}, {f}));' for f, _ in cls._fields_]
    src += [*extra_printf, '  return 0;', '}']
    c = tmp_path / "abi.c"
    c.write_text("\n".join(src))
    exe = tmp_path / "abi"
    subprocess.check_call(["gcc", "-std=c99", "-o", str(exe), str(c)])
    got = dict(line.split() for line in subprocess.check_output([str(exe)], text=True).splitlines())
    assert int(got[name]) == ctypes.sizeof(cls)
    for f, _ in cls._fields_:
        assert int(got[f"{name}.{f}"]) == getattr(cls, f).offset, f
    assert cls.struct_bytes.offset == 0
    return got
