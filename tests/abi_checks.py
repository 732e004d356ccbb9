"""What the C-ABI tests (test_*_abi.py, test_model_and_abi.py) share: the ctypes mirrors against the header's
layout through gcc, and the entry points against the two built libraries."""
import ctypes as C
import os
import subprocess
import tempfile

from panda_gym_amd import _native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header_layout(structs, extra_printfs=()):
    """``structs``: C struct name -> ctypes mirror.  Compiles (gcc, as C99, warnings are errors) and runs a
    program that prints ``sizeof`` and every field's ``offsetof`` from include/pgx.h, asserts that the mirror
    has the same size and offsets, and returns what the ``extra_printfs`` statements (each printing one
    ``name value...`` line) wrote as {name: rest of the line}."""
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{ROOT}/include/pgx.h"', "int main(void){"]
    for s, cls in structs.items():
        lines.append(f'printf("{s} %zu\\n", sizeof({s}));')
        for f, _ in cls._fields_:
            lines.append(f'printf("{s}.{f} %zu\\n", offsetof({s}, {f}));')
    lines += list(extra_printfs) + ["return 0;}"]
    with tempfile.TemporaryDirectory() as tmp:
        src, exe = os.path.join(tmp, "lay.c"), os.path.join(tmp, "lay")
        with open(src, "w") as fh:
            fh.write("\n".join(lines))
        subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-o", exe, src], check=True)
        text = subprocess.run([exe], capture_output=True, text=True, check=True).stdout
    out = dict(l.split(" ", 1) for l in text.split("\n") if l)
    for s, cls in structs.items():
        assert int(out.pop(s)) == C.sizeof(cls), s
        for f, _ in cls._fields_:
            assert int(out.pop(f"{s}.{f}")) == getattr(cls, f).offset, (s, f)
    return out


def assert_exported(names):
    """Every name is an entry point of the loaded library, of ``_native.EXPORTS`` and of libpgx_rtmodel.so."""
    lib = _native.load()
    for name in names:
        assert hasattr(lib, name), name
        assert name in _native.EXPORTS, name
    rt = os.path.join(ROOT, "panda-gym_amd", "libpgx_rtmodel.so")
    assert os.path.exists(rt), "build() makes the runtime-model library too"
    rtlib = C.CDLL(rt)
    for name in names:
        assert hasattr(rtlib, name), name
