"""CPU checks of the device sampler's numpy restatement (tests/sample_ref.py) and of its C-ABI parameter block."""
import ctypes
import os
import subprocess

import numpy as np

from oracle import sampling_oracle as so
from tests import sample_ref as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _hex(words):
    return " ".join(f"{int(w):08x}" for w in words)


def test_philox_known_answers():
    cases = (((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
             ((0xffffffff,) * 4, (0xffffffff, 0xffffffff), "408f276d 41c83b0e a20bc7c6 6d5451fd"),
             ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), "d16cfe09 94fdcceb 5001e420 24126ea1"))
    for ctr, key, want in cases:
        assert _hex(sr.philox4x32_10(np.array([ctr], dtype=np.uint32), key)[0]) == want


def test_uniforms_lie_in_the_open_unit_interval_and_follow_the_counter_layout():
    seed, step = 0x0123456789abcdef, 7
    u = sr.uniforms(10, seed, step)
    assert u.shape == (10,) and np.all(u > 0) and np.all(u < 1)
    w = sr.philox4x32_10(np.array([[2, step, 0, 0]], dtype=np.uint32), (seed & 0xffffffff, seed >> 32))[0]
    assert u[9] == ((int(w[1]) >> 8) + 0.5) * 2.0 ** -24         # token 9: counter 9 >> 2 = 2, word 9 & 3 = 1
    assert not np.array_equal(u, sr.uniforms(10, seed, step + 1))
    assert not np.array_equal(u, sr.uniforms(10, seed + 1, step))


def test_draws_follow_the_processed_softmax():
    rng = np.random.default_rng(3)
    V = 40
    logits = (rng.standard_normal(V) * 2).astype(np.float32)
    hist = [1, 5, 7, 30]
    T, rp, tp, tk = 0.8, 1.3, 0.9, 12
    proc = so.process_logits(logits, hist, T, rp, tp, tk)
    keep = np.isfinite(proc)
    p = np.zeros(V)
    e = np.exp(proc[keep].astype(np.float64) - proc[keep].max())
    p[keep] = e / e.sum()
    seed = 0x5eed
    x = proc.astype(np.float64)
    n = 50_000
    counts = np.zeros(V, dtype=np.int64)
    for step in range(n):
        s = np.where(keep, x - np.log(-np.log(sr.uniforms(V, seed, step))), -np.inf)
        counts[int(np.argmax(s))] += 1
    assert counts[~keep].sum() == 0
    tv = 0.5 * np.abs(counts / n - p).sum()
    assert tv < 0.01, tv
    # the helper's draw is this same race
    for step in (0, 1, 17):
        tok, margin, got = sr.draw(logits, hist, T, rp, tp, tk, seed, step)
        assert np.array_equal(np.isfinite(got), keep) and keep[tok] and margin > 0


def test_greedy_rule_and_non_finite_rows():
    x = np.array([1.0, 3.0, 3.0, np.nan, -np.inf], dtype=np.float32)
    assert sr.draw(x, [], 0.0, 1.0, 1.0, -1, 1, 0)[0] == 1            # lowest index among equal maxima
    assert sr.draw(x, [1], 0.0, 1.5, 1.0, -1, 1, 0)[0] == 2           # the penalty moves the argmax
    assert sr.draw(np.full(6, -np.inf, dtype=np.float32), [], 1.0, 1.0, 0.9, -1, 1, 0)[0] == 0
    tok, _, _ = sr.draw(x, [], 0.7, 1.0, 1.0, 1, 9, 3)                # top_k = 1: one of the maxima
    assert tok in (1, 2)


def test_sample_params_layout_matches_the_header(tmp_path):
    from promptcache_amd import _native
    cls = _native.SampleParams
    src = tmp_path / "layout.c"
    body = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{ROOT}/include/promptcache_hip.h"', 'int main(void) {',
            '  printf("size %zu\\n", sizeof(pc_sample_params));']
    body += [f'  printf("{f} %zu\\n", offsetof(pc_sample_params, {f}));' for f, _ in cls._fields_]
    body += ['  return 0;', '}']
    src.write_text("\n".join(body))
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", str(src), "-o", str(exe)])
    got = dict(line.rsplit(" ", 1) for line in subprocess.check_output([str(exe)], text=True).strip().splitlines())
    assert int(got["size"]) == ctypes.sizeof(cls) == len(_native.sample_params_bytes(1.0, 1.0, 1.0, -1, 0))
    for name, _ in cls._fields_:
        assert int(got[name]) == getattr(cls, name).offset, name
    blk = _native.sample_params_bytes(0.7, 1.1, 0.9, 40, 2 ** 62 + 5)
    assert np.frombuffer(blk[:12], dtype=np.float32).tolist() == [np.float32(0.7), np.float32(1.1), np.float32(0.9)]
    assert int.from_bytes(blk[12:16], "little", signed=True) == 40 and int.from_bytes(blk[16:24], "little") == 2 ** 62 + 5


def test_sample_advance_argument_errors_need_no_gpu():
    from promptcache_amd import _native
    lib = _native.load()
    assert lib.pc_sample_advance(None, 10, None, None, None, None, None, None, None, 4, None, None) == -1001
    assert b"pc_sample_advance" in lib.pc_last_error_string()
