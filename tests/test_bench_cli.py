"""bench.py's command line: a plain run prints the headline only, ``--full`` adds the other legs, and ``--dump-outputs DIR`` writes
what the last timed step returned -- the same arrays from a plain and a ``--full`` run of the same arguments."""
import json
import os
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class _FakeKV:
    """The ``past_key_values`` interface ``step_outputs`` reads: per layer (K, V) views [B, Hkv, rows, D] of one arena."""

    def __init__(self, buf, n):
        self.buf, self.n = buf, n

    def __len__(self):
        return self.buf.shape[1]

    def __getitem__(self, i):
        return self.buf[:, i, 0, :, :self.n], self.buf[:, i, 1, :, :self.n]


@pytest.mark.parametrize("L,Hkv,S,q", [(2, 4, 5, 3), (32, 32, 300, 12), (40, 40, 40, 80)])
def test_step_outputs_are_seeded_and_bounded(tmp_path, L, Hkv, S, q):
    sys.path.insert(0, ROOT)
    import bench
    D, V = 128, 32000
    g = torch.Generator().manual_seed(0)
    buf = torch.randn(1, L, 2, Hkv, S + q + 5, D, generator=g).half()
    out = types.SimpleNamespace(logits=torch.randn(1, q, V, generator=g).half(), past_key_values=_FakeKV(buf, S + q))
    ids, pos = list(range(7, 7 + q)), list(range(S, S + q))
    a = bench.step_outputs(out, ids, pos)
    b = bench.step_outputs(out, ids, pos)
    assert a.keys() == b.keys() and all(np.array_equal(np.asarray(a[k]), np.asarray(b[k])) for k in a)
    bench.dump_outputs(str(tmp_path), a)
    files = sorted(os.listdir(tmp_path))
    assert files == sorted(k + ".npy" for k in a)
    assert sum(os.path.getsize(tmp_path / f) for f in files) <= bench.DUMP_LIMIT_BYTES
    got = {f[:-4]: np.load(tmp_path / f) for f in files}
    assert all(v.dtype in (np.float32, np.float64) for v in got.values())
    assert np.array_equal(got["input_ids"], ids) and np.array_equal(got["position_ids"], pos)
    lr = got["logits_rows"].astype(int)
    assert np.array_equal(got["logits"], out.logits[0, lr].float().numpy())
    new, new_rows = got["kv_new"], got["kv_new_rows"].astype(int)
    staged, staged_rows = got["kv_staged_sample"], got["kv_staged_sample_rows"].astype(int)
    assert new_rows.min() >= S and new_rows.max() < S + q and staged_rows.max() < S
    assert len(new_rows) == new.shape[3] == min(q, len(new_rows)) and len(staged_rows) == staged.shape[3] <= 16
    assert (q <= 16) == (len(new_rows) == q) and (q <= 64) == (len(lr) == q)
    assert np.array_equal(new[:, 0, :, -1], buf[0, :, 0, :, new_rows[-1]].float().numpy())
    assert np.array_equal(staged[:, 1, :, 0], buf[0, :, 1, :, staged_rows[0]].float().numpy())


def _bench(*extra, dump):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--model", "mid",
           "--max-ctx", "2048", "--dump-outputs", str(dump), *extra]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_and_full_runs_dump_the_same_step(tmp_path):
    plain = _bench(dump=tmp_path / "plain")
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in plain
    assert plain["steps"] == 3 and plain["warmup"] == 1 and plain["ms_per_step"] > 0 and plain["value"] > 0
    for k in ("encode", "encode_library", "roofline", "roofline_gather", "cpu_baseline", "parity", "configs", "decode"):
        assert k not in plain, k
    full = _bench("--full", "--no-context", "--no-cpu-baseline", dump=tmp_path / "full")
    assert full["encode"]["tokens"] > 0 and full["encode_library"]["schemas"] == 8 and "roofline_gather" in full
    names = sorted(os.listdir(tmp_path / "plain"))
    assert names == sorted(os.listdir(tmp_path / "full")) and "logits.npy" in names
    for n in names:
        a, b = np.load(tmp_path / "plain" / n), np.load(tmp_path / "full" / n)
        assert a.dtype in (np.float32, np.float64) and a.shape == b.shape and np.isfinite(a).all(), n
        np.testing.assert_allclose(a, b, rtol=0, atol=1e-3, err_msg=n)
