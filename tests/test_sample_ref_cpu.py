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


# ---- the parameter block the sampled loop writes (LlamaHIP._sample_state_fill) ---------------------------------------------
def _filled_block(T, rp, tp, tk, seed=12345, V=1000):
    """The pc_sample_params bytes _sample_state_fill writes for one GenerationParameters (host tensors: no GPU)."""
    import types

    import torch
    from promptcache_amd import _native
    from promptcache_amd.generation_engine import GenerationParameters
    from promptcache_amd.model.llama_hip import LlamaHIP
    st = dict(params=torch.zeros(ctypes.sizeof(_native.SampleParams), dtype=torch.uint8),
              hist=torch.zeros((V + 31) // 32, dtype=torch.int32))
    params = GenerationParameters(temperature=T, repetition_penalty=rp, top_p=tp, top_k=tk)
    LlamaHIP._sample_state_fill(types.SimpleNamespace(config=types.SimpleNamespace(vocab_size=V)), st, params, seed, [3, 999])
    return params, bytes(st["params"].numpy())


def _kernel_reads(blk, V):
    """What pc_sample_advance decides from a block, restated in fp32 (csrc/pc_sample.hip: greedy, tdiv, pen, want_p, want_k)."""
    T, rp, tp = (np.float32(v) for v in np.frombuffer(blk[:12], dtype=np.float32))
    tk = int.from_bytes(blk[12:16], "little", signed=True)
    return dict(greedy=bool(T < np.float32(1e-5) or tp < np.float32(1e-8)), tdiv=bool(T >= np.float32(1e-5) and T != 1),
                pen=bool(rp > 1), want_p=bool(tp >= np.float32(1e-8) and tp < 1), k=min(tk, V) if tk > 0 else V,
                T=T, rp=rp, tp=tp, seed=int.from_bytes(blk[16:24], "little"))


def _reference_decides(params, V):
    return dict(greedy=params.greedy, tdiv=params.temperature >= 1e-5 and params.temperature != 1.0,
                pen=params.repetition_penalty > 1.0, want_p=1e-8 <= params.top_p < 1.0,
                k=min(params.top_k, V) if params.top_k > 0 else V)


EDGE_T = (0.0, 9.9999999e-6, np.nextafter(1e-5, 0.0), 1e-5, np.nextafter(1e-5, 1.0), 0.7, np.nextafter(1.0, 0.0), 1.0,
          np.nextafter(1.0, 2.0), 1.0 + 1e-9, 100.0, float("nan"))
EDGE_P = (0.0, np.nextafter(1e-8, 0.0), 1e-8, np.nextafter(1e-8, 1.0), 0.5, 0.95, np.nextafter(1.0, 0.0), 1.0, 1.5)
EDGE_RP = (0.5, np.nextafter(1.0, 0.0), 1.0, np.nextafter(1.0, 2.0), 1.0 + 1e-9, 1.1, 2.0)
EDGE_K = (-(2 ** 40), -1, 0, 1, 40, 999, 1000, 1001, 2 ** 31 - 1, 2 ** 31, 2 ** 32 + 5, 2 ** 40)


def test_sampled_loop_block_decides_as_the_reference_in_double():
    """Every threshold the kernel re-tests in fp32 decides as the reference decided in double, at the neighbours of T = 1e-5,
    T = 1, top_p = 1e-8, top_p = 1 and rp = 1.  The one accepted exception: a top_p in [1e-8, 1) that rounds to 1.0f (top-p
    off on the device, mass below 1e-7)."""
    V, n = 1000, 0
    for T in EDGE_T:
        for tp in EDGE_P:
            for rp in EDGE_RP[::2] if tp not in (0.5, 1.0) else EDGE_RP:
                params, blk = _filled_block(T, rp, tp, 40)
                got, want = _kernel_reads(blk, V), _reference_decides(params, V)
                if want["want_p"] and not got["want_p"]:
                    assert np.float32(tp) == 1.0, (T, rp, tp)
                    got["want_p"] = True
                if want["greedy"]:
                    got.pop("tdiv"), want.pop("tdiv")                 # greedy: no division either way (kernel T = 0)
                    assert got["T"] == 0.0
                # a warper whose fp32 factor is 1.0 is the identity: skipping it decides the same
                for key, v in (("tdiv", T), ("pen", rp)):
                    if want.get(key) and not got[key] and np.float32(v) == 1.0:
                        want[key] = False
                for key in ("greedy", "tdiv", "pen", "want_p", "k"):
                    assert got.get(key) == want.get(key), (key, T, rp, tp, got, want)
                if want.get("tdiv"):
                    assert got["T"] == np.float32(T)
                if want["pen"]:
                    assert got["rp"] == np.float32(rp)
                assert got["seed"] == 12345
                n += 1
    assert n > 300


def test_sampled_loop_block_canonical_values():
    # case 1: T just below 1e-5 is greedy in the reference; the fp32 1e-5f would sample
    assert np.float32(9.9999999e-6) == np.float32(1e-5)
    params, blk = _filled_block(9.9999999e-6, 1.2, 1.0, -1)
    assert params.greedy and _kernel_reads(blk, 1000)["greedy"]
    assert np.frombuffer(blk[:12], dtype=np.float32).tolist() == [0.0, np.float32(1.2), 1.0]
    # case 2: a top_k past int32 keeps everything (the reference: min(top_k, V)), not top_k mod 2^32
    for tk in (2 ** 31, 2 ** 32 + 5, 2 ** 40):
        _, blk = _filled_block(0.7, 1.0, 1.0, tk)
        assert int.from_bytes(blk[12:16], "little", signed=True) == 2 ** 31 - 1
    for tk in (0, -5, -(2 ** 40)):
        _, blk = _filled_block(0.7, 1.0, 1.0, tk)
        assert int.from_bytes(blk[12:16], "little", signed=True) == -1
    # no warper in the reference -> the neutral value on the device
    _, blk = _filled_block(1.0 + 1e-9, 0.9, 1.5, 40)
    assert np.frombuffer(blk[:12], dtype=np.float32).tolist() == [1.0, 1.0, 1.0]
    _, blk = _filled_block(0.7, 1.0, np.nextafter(1e-8, 0.0), 40)       # greedy by top_p: T = 0, no top-p warper
    assert np.frombuffer(blk[:12], dtype=np.float32).tolist() == [0.0, 1.0, 1.0]
    # the raw block stays raw (kernel tests feed edge values through it)
    raw = _native_raw(9.9999999e-6, 1.2, 1.0, 2 ** 31 - 1)
    assert np.frombuffer(raw[:4], dtype=np.float32)[0] == np.float32(1e-5)


def _native_raw(T, rp, tp, tk):
    from promptcache_amd import _native
    return _native.sample_params_bytes(T, rp, tp, tk, 0)
