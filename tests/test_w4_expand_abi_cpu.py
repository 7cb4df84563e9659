"""CPU-side check of ``pc_w4_expand``: the ctypes mirror of ``pc_w4_expand_args`` has the size and the field offsets the C compiler
gives the header's struct, the entry point is in the signature table with the header's arity, and every argument error is
answered with ``PC_ERR_ARG`` before anything touches a device (tests/test_w4_rows_abi_cpu.py is the pattern)."""
import ctypes
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_w4_expand_struct_layout_matches_the_header(tmp_path):
    from promptcache_amd import _native
    st, cls = "pc_w4_expand_args", _native.W4ExpandArgs
    body = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{ROOT}/include/promptcache_hip.h"', 'int main(void) {',
            f'  printf("{st} %zu\\n", sizeof({st}));', '  printf("FRAG %d\\n", PC_W4_EXPAND_FRAG);',
            '  printf("ROWMAJOR %d\\n", PC_W4_EXPAND_ROWMAJOR);']
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
    assert [f for f, _ in cls._fields_] == ["struct_bytes", "layout", "N", "K", "codes", "scales", "row_perm", "out", "ld_out"]
    assert (int(got["FRAG"]), int(got["ROWMAJOR"])) == (_native.W4_EXPAND_FRAG, _native.W4_EXPAND_ROWMAJOR)


def test_w4_expand_entry_is_declared_and_mirrored():
    from promptcache_amd import _native
    restype, argtypes = _native.SIGNATURES["pc_w4_expand"]
    assert restype is ctypes.c_int and len(argtypes) == 2
    assert argtypes[0] is ctypes.POINTER(_native.W4ExpandArgs)
    assert callable(_native.w4_expand)
    assert hasattr(_native.load(), "pc_w4_expand")


A = 0x10000          # a 16-byte aligned address that is never dereferenced: every call below is refused before a launch


@pytest.mark.parametrize("kw,word", [
    (dict(N=40), "N%16"), (dict(K=192), "K%128"), (dict(N=0), "N%16"), (dict(K=0), "K%128"),
    (dict(layout=2), "layout"), (dict(layout=-1), "layout"),
    (dict(layout=1, ld_out=248), "ld_out"), (dict(layout=1, ld_out=260), "ld_out"), (dict(layout=1, ld_out=0), "ld_out"),
    (dict(codes=None), "null"), (dict(scales=None), "null"), (dict(out=None), "null"),
    (dict(codes=A + 8), "aligned"), (dict(scales=A + 4), "aligned"), (dict(out=A + 2), "aligned"),
    (dict(struct_bytes=8), "struct_bytes"), (dict(struct_bytes=64), "struct_bytes"),
])
def test_w4_expand_argument_errors_need_no_gpu(kw, word):
    from promptcache_amd import _native
    f = dict(codes=A, scales=A, out=A, N=48, K=256, layout=0, ld_out=0)
    f.update(kw)
    with pytest.raises(RuntimeError, match="-1001") as e:
        _native.w4_expand(f["codes"], f["scales"], f["out"], f["N"], f["K"], f["layout"], ld_out=f["ld_out"],
                          struct_bytes=f.get("struct_bytes"), stream=0)
    assert word in str(e.value), str(e.value)


def test_w4_expand_null_args_pointer():
    from promptcache_amd import _native
    assert _native.load().pc_w4_expand(None, None) == -1001
