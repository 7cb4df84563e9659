"""CPU-side check of ``pc_gemm_w4_rows_args``: the ctypes mirror has the size and the field offsets the C compiler gives the
header's struct (as tests/test_abi_symbols.py::test_struct_layouts_match_the_header checks the structs of its tuple), and the
entry point is in the signature table with the header's arity."""
import ctypes
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_w4_rows_struct_layout_matches_the_header(tmp_path):
    from promptcache_amd import _native
    st, cls = "pc_gemm_w4_rows_args", _native.GemmW4RowsArgs
    body = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{ROOT}/include/promptcache_hip.h"', 'int main(void) {',
            f'  printf("{st} %zu\\n", sizeof({st}));']
    for f, _ in cls._fields_:
        body.append(f'  printf("{st}.{f} %zu\\n", offsetof({st}, {f}));')
    body += ['  return 0;', '}']
    src = tmp_path / "layout.c"
    src.write_text("\n".join(body))
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-Wno-unused-function", str(src), "-o", str(exe)])
    got = dict(line.rsplit(" ", 1) for line in subprocess.check_output([str(exe)], text=True).strip().splitlines())
    assert int(got[st]) == ctypes.sizeof(cls)
    for name, _ in cls._fields_:
        assert int(got[f"{st}.{name}"]) == getattr(cls, name).offset, name
    assert [f for f, _ in cls._fields_] == ["struct_bytes", "epilogue", "codes", "scales", "xf_hi", "xf_lo", "M", "N", "K", "kslices",
                                           "y", "ldy", "of_hi", "of_lo"]


def test_w4_rows_entry_is_declared_and_mirrored():
    from promptcache_amd import _native
    restype, argtypes = _native.SIGNATURES["pc_gemm_w4_rows"]
    assert restype is ctypes.c_int and len(argtypes) == 2
    assert argtypes[0] is ctypes.POINTER(_native.GemmW4RowsArgs)
    assert callable(_native.gemm_w4_rows)
