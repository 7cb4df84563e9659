"""bench.py -- cached-prefill TTFT / tokens-per-second of the prompt-cache hot path on MI355X.

    python bench.py [--gpus N --steps K --warmup W] [--dump-outputs DIR] [--full]
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P \
        bench.py --gpus N --steps K --warmup W

Workload (BASELINE.json metric: "TTFT + cached-prefill tokens/sec, Llama-2-7b persona schema"):
Llama-2-7b shape (L=32, H=Hkv=32, D=128, hidden 4096, inter 11008, vocab 32000), fp16 weights drawn
N(0, 0.02) on the device (no checkpoints offline), a synthetic PML schema with the structure of
examples/persona_generation.xml (29 encode passes, 25 staged segments, S = 1725 cached tokens, q = 12 new
tokens; promptcache_amd/synth.py) and the deterministic stand-in tokenizer.

One STEP = one pass of the hot path for one prompt, exactly what the reference times as
cache_time + response_time (eval.py:212-215):
    CacheEngine.process(prompt)            request assembly + module-KV gather into the staged buffer
    lm(input_ids, position_ids, past=...)  prefill of the q new tokens over the staged KV (all 32 layers,
                                           logits for every new row)
The staged buffer is reset before every step so the gather always moves all S tokens (no retained
segments), inputs are resident in HBM.  value = N * (S + q) / TTFT: every rank serves its own replica of
the prompt (single-prompt TTFT has no cross-GPU step; "weak" scaling).  Schema encode -- the part of the
path that does shard -- runs before the timed region, sharded over the ranks with one all-gather, and is
reported under "encode".

A plain run sets up (model, one schema encode), warms up, times the K steps and prints the headline line
("breakdown_ms", "staging" and "roofline_step" come from the timed steps themselves).  --full adds every other
leg, each with runs of its own: the steady-state "encode" and the schema-library "encode_library", "roofline"
(the dominant hand-written kernel, HIP-event timed on its launch stream) and the other per-kernel rooflines,
the context legs (no_cache, decode, cold shapes, host tier, int8), "cpu_baseline" (the numpy oracle on the
host cores, bounded sample), "parity" (same-run max |delta logit| GPU vs oracle at the true layer shape) and
"configs" (BASELINE configs 2-4, compact); the --no-* options switch single legs of a --full run off.

--dump-outputs DIR writes what the last timed step returned to its caller as DIR/<name>.npy (float32, integer
ids as float64; a fixed, seeded sample of the staged K/V rows), 64 MB at most: two builds run with the same
arguments see identical inputs and can be compared output for output.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
for _p in (ROOT, os.path.join(ROOT, "prompt-cache_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

HBM_PEAK_GBS = 8000.0   # MI355X HBM3E spec peak (guides/MI355X_MICROARCH.md); ~6.3 TB/s is the measured copy ceiling
MFMA_PEAK_TFLOPS = 2500.0   # dense fp16 MFMA peak (guides/MI355X_MICROARCH.md; the headline 5 PF includes 2:1 sparsity)


def cpu_baseline_and_parity(lm, eng, prompt, ids, pos, k_layers: int, repeats: int = 2, parity_layers: int = 0):
    """Time the numpy oracle (oracle/, 'port' of the reference's CPU path) on the host cores on a bounded
    sample -- the full-size gather plus k of the 32 layers and lm_head, scaled by L/k -- and compare the
    GPU logits of the FULL-depth stack (``parity_layers``, default all L) with the oracle's on identical weights and
    staged KV: shallow stacks say little about parity, and the oracle's cost for the q new rows
    is one pass over the fp32 weights per layer."""
    import numpy as np
    import torch
    from threadpoolctl import threadpool_info, threadpool_limits
    from oracle.llama_oracle import LlamaOracle, OracleConfig, kv_gather

    m = lm.hf_model
    c = m.config
    L = c.num_hidden_layers
    # --- weights of the first k layers (+ embed, norm, lm_head) as fp32 numpy: identical values ---
    w = {"embed": m.embed.float().cpu().numpy(), "norm": m.norm.float().cpu().numpy(),
         "lm_head": m.lm_head.float().cpu().numpy()}
    H, Hkv, D = m.H, m.Hkv, m.D
    p_layers = L if parity_layers <= 0 else min(parity_layers, L)
    for i in range(max(k_layers, p_layers)):
        lw = m.layers[i]
        wqkv = lw["wqkv"].float().cpu().numpy()
        w[f"l{i}.wq"], w[f"l{i}.wk"], w[f"l{i}.wv"] = wqkv[:H * D], wqkv[H * D:(H + Hkv) * D], wqkv[(H + Hkv) * D:]
        wgu = lw["wgu"].float().cpu().numpy()
        w[f"l{i}.gate"], w[f"l{i}.up"] = wgu[:c.intermediate_size], wgu[c.intermediate_size:]
        for k in ("ln1", "ln2", "wo"):
            w[f"l{i}.{k}"] = lw[k].float().cpu().numpy()
        w[f"l{i}.down"] = lw["wdown"].float().cpu().numpy()
    cfg = OracleConfig(vocab_size=c.vocab_size, hidden_size=c.hidden_size, intermediate_size=c.intermediate_size,
                       num_hidden_layers=max(k_layers, p_layers), num_attention_heads=H, num_key_value_heads=Hkv,
                       rms_norm_eps=c.rms_norm_eps, rope_theta=c.rope_theta, inv_freq=m.inv_freq_cpu.numpy())
    oracle = LlamaOracle(cfg, w)
    # --- module KV of the used segments on the host (all layers: the gather is timed at full size) ---
    staged_mods = eng.prompt_cache.staged
    segs = []
    for sc in staged_mods:
        st = sc.store.cpu().numpy()                                   # [L,2,Hkv,len,D] fp16
        segs.append([(st[i, 0], st[i, 1]) for i in range(L)])
    max_ctx = eng.prompt_cache.max_ctx_length
    ids_np, pos_np = np.asarray([ids]), np.asarray([pos])
    logits = None
    blas_default = max([p.get("num_threads", 1) for p in threadpool_info() if p.get("user_api") == "blas"] or [1])
    # The BLAS pool's default width is not its best one on a many-core host (tools/blas_probe.py on a 256-CPU box: sgemm at 130
    # rows 0.54 TFLOP/s on the default 64 threads, 2.6-2.8 on 16-32): the baseline is timed at several widths and the FASTEST
    # is reported, with `cores` = that width.
    tried = {}
    for nt in sorted({16, 32, blas_default} if blas_default > 16 else {blas_default}):
        t_gather, t_prefill = [], []
        with threadpool_limits(limits=nt, user_api="blas"):
            for _ in range(repeats):
                t0 = time.perf_counter()
                staged, S = kv_gather(segs, max_ctx)                          # PromptCache.update on the CPU
                t1 = time.perf_counter()
                past = [(k[None], v[None]) for k, v in staged[:k_layers]]
                logits, _ = oracle.forward(ids_np, pos_np, past=past, n_layers=k_layers)
                t2 = time.perf_counter()
                t_gather.append(t1 - t0)
                t_prefill.append(t2 - t1)
            # lm_head + embedding are paid once, the k layers scale to L
            t0 = time.perf_counter()
            _ = (np.zeros((len(ids), c.hidden_size), np.float32) @ w["lm_head"].T)
            t_head = time.perf_counter() - t0
        tp = min(t_prefill)
        tried[nt] = (min(t_gather) + (tp - t_head) * (L / k_layers) + t_head, min(t_gather))
    threads = min(tried, key=lambda k: tried[k][0])
    ttft_cpu, t_gather = tried[threads][0], [tried[threads][1]]
    _best_blas = threadpool_limits(limits=threads, user_api="blas")      # (the parity run below uses the fastest width too)
    # --- parity at the true shape AND depth: GPU cached prefill (the timed step's own forward) vs the oracle over the
    # same staged KV, all p_layers layers ---
    t0 = time.perf_counter()
    staged, S = kv_gather(segs, max_ctx)
    logits, _ = oracle.forward(ids_np, pos_np, past=[(k[None], v[None]) for k, v in staged[:p_layers]], n_layers=p_layers)
    t_par = time.perf_counter() - t0
    ids2, pos2, _, cache = eng.process(prompt)
    out = lm(input_ids=torch.tensor([ids2], device=lm.device), position_ids=torch.tensor([pos2], device=lm.device),
             past_key_values=cache, use_cache=True, num_layers=None if p_layers == L else p_layers)
    err = float(np.abs(out.logits[0].float().cpu().numpy() - logits[0]).max())
    n_tok = S + len(ids)
    _best_blas.restore_original_limits()
    base = {"value": n_tok / ttft_cpu, "unit": "tokens/s", "cores": int(threads), "kind": "port",
            "host_cpus": os.cpu_count(), "ttft_ms": ttft_cpu * 1e3, "gather_ms": min(t_gather) * 1e3,
            "blas_threads_tried_ttft_ms": {str(k): round(v[0] * 1e3, 1) for k, v in sorted(tried.items())},
            "sample": (f"numpy oracle (oracle/llama_oracle.py), same persona-like prompt: full-size gather (L={L}) + "
                       f"{k_layers} of {L} layers at the 7b layer shape + lm_head, best of {repeats}; layer time scaled by "
                       f"{L}/{k_layers}")}
    parity = {"max_abs_dlogit": err, "tol": 1e-2, "layers": p_layers, "staged_tokens": int(S), "new_tokens": len(ids),
              "max_abs_logit": float(np.abs(logits).max()), "oracle_seconds": t_par,
              "what": "GPU cached prefill of the timed step (all layers) vs the numpy oracle on identical weights, "
                      "staged module KV and positions; end-to-end parity incl. the encode: tests/test_gpu_fullsize.py"}
    return base, parity


def compact_summary(result: dict) -> dict:
    """Every leg's headline value in <= 1500 characters, as the LAST key of the JSON line (the driver's record keeps the tail of
    stdout: the legs' full objects above scroll out of it).  Recipe the legs mirror: /root/reference/eval.py:172-219."""
    def g(path, nd=None):
        x = result
        for k in path.split("."):
            if not isinstance(x, dict) or k not in x or x[k] is None:
                return None
            x = x[k]
        return round(x, nd) if (nd is not None and isinstance(x, float)) else x
    s = {"ttft_ms": g("ms_per_step", 3), "tok_s": g("value", 0), "step_hbm_frac": g("roofline_step.frac", 3),
         "kernel_frac": g("roofline.frac", 3), "gather_GBs": g("roofline_gather.achieved", 0),
         "nocache_ttft_ms": g("no_cache.ttft_ms", 2),
         "decode_tok_s": g("decode.tokens_per_s", 1), "decode_loop_tok_s": g("decode_device_loop.tokens_per_s", 1),
         "decode_loop_hbm_frac": g("decode_device_loop.hbm_frac", 3),
         "encode_tok_s": g("encode.tokens_per_s", 0), "encode_frac": g("encode.roofline.frac", 3),
         "library_tok_s": g("encode_library.tokens_per_s", 0),
         "parity_dlogit": g("parity.max_abs_dlogit", 6), "cpu_tok_s": g("cpu_baseline.value", 0)}
    i8 = result.get("int8_weights")
    if isinstance(i8, dict):
        s["int8"] = {"ttft_ms": g("int8_weights.ttft_ms", 3), "loop_tok_s": g("int8_weights.decode_device_loop_tokens_per_s", 1),
                     "outlier_cols": g("int8_weights.outlier_columns_last_layer.down_proj_in")}
        if isinstance(i8.get("trained_like"), dict):
            s["int8"]["trained_like"] = {"ttft_ms": g("int8_weights.trained_like.ttft_ms", 3),
                                         "loop_tok_s": g("int8_weights.trained_like.decode_device_loop_tokens_per_s", 1),
                                         "outlier_cols": g("int8_weights.trained_like.outlier_cols")}
    cf = result.get("configs")
    if isinstance(cf, dict):
        s["configs"] = {k: [round(v["ms_per_step"], 3), round(v["frac"], 3)] for k, v in cf.items()
                        if isinstance(v, dict) and "ms_per_step" in v}
        s["c4_attn_frac"] = g("configs.4.roofline_attention.frac", 4)
        s["c4_attn_us"] = g("configs.4.roofline_attention.avg_launch_us", 1)
    return {k: v for k, v in s.items() if v is not None}


def _pmc_traffic(kernel_key: str, signature: str):
    """HBM bytes per launch from the committed PMC summary (profiles/pmc_traffic.json, written by tools/pmc_traffic.py from
    separate rocprofv3 --pmc passes: FETCH_SIZE x 2 on gfx950 + WRITE_SIZE).  None unless the summary was taken on exactly
    this workload signature -- the number is never hard-coded here."""
    path = os.path.join(ROOT, "profiles", "pmc_traffic.json")
    try:
        with open(path) as f:
            tab = json.load(f)
    except (OSError, ValueError):
        return None, None
    ent = tab.get(kernel_key)
    if not ent or ent.get("signature") != signature:
        return None, None
    return ent.get("hbm_bytes_per_launch"), ent.get("source")


DUMP_LIMIT_BYTES = 64_000_000       # --dump-outputs: all arrays together


def step_outputs(out, ids, pos, seed: int = 1234) -> dict:
    """What one step of the timed path hands its caller, for ``--dump-outputs``: the ids / positions ``process()`` assembled, the
    logits of the new rows and, from the ``past_key_values`` the forward returned, the K / V it appended for the new rows and a
    fixed, seeded sample of the staged rows it attended to (every layer; rows are key indices).  Row counts shrink with the model
    so that the whole dump stays under DUMP_LIMIT_BYTES; more than 64 new rows are sampled the same way."""
    import numpy as np
    import torch
    rng = np.random.default_rng(seed)

    def pick(n, k):
        return np.arange(n) if n <= k else np.sort(rng.choice(n, k, replace=False))
    logits = out.logits.reshape(-1, out.logits.shape[-1])
    lrows = pick(logits.shape[0], 64)
    res = {"input_ids": np.asarray(ids), "position_ids": np.asarray(pos), "logits_rows": lrows,
           "logits": logits[torch.as_tensor(lrows, device=logits.device)]}
    kv = out.past_key_values
    L = len(kv)
    _, Hkv, n, D = kv[0][0].shape
    q = len(ids)
    S = n - q
    row_bytes = L * 2 * Hkv * D * 4
    budget = max(2, int((DUMP_LIMIT_BYTES * 0.9 - res["logits"].numel() * 4) // row_bytes))
    new_rows = S + pick(q, min(16, budget // 2))
    staged_rows = pick(S, min(16, budget - len(new_rows)))
    for name, rows in (("kv_new", new_rows), ("kv_staged_sample", staged_rows)):
        r = torch.as_tensor(rows, device=kv[0][0].device)
        res[name] = torch.stack([torch.stack([kv[i][0][0][:, r], kv[i][1][0][:, r]]) for i in range(L)])   # [L, 2, Hkv, rows, D]
        res[name + "_rows"] = rows
    return res


def dump_outputs(out_dir: str, arrays: dict) -> None:
    """Write every array as ``out_dir/<name>.npy``: floating point as float32, integers as float64 (exact)."""
    import numpy as np
    import torch
    host = {}
    for name, a in arrays.items():
        if isinstance(a, torch.Tensor):
            a = a.detach().float().cpu().numpy() if a.is_floating_point() else a.detach().cpu().double().numpy()
        a = np.asarray(a)
        host[name] = np.ascontiguousarray(a, dtype=np.float32 if np.issubdtype(a.dtype, np.floating) else np.float64)
    total = sum(a.nbytes for a in host.values())
    if total > DUMP_LIMIT_BYTES:
        raise SystemExit(f"--dump-outputs: {total} bytes exceed the {DUMP_LIMIT_BYTES}-byte limit")
    os.makedirs(out_dir, exist_ok=True)
    for name, a in host.items():
        np.save(os.path.join(out_dir, name + ".npy"), a)


def gemm_rooflines(lm, T: int):
    """Event-time the weight-streaming launches of one decoder layer eagerly on every layer's real weights -- kernels inside
    the captured graph cannot be bracketed by events; the in-graph durations are in profiles/ (rocprofv3).  32 distinct weight
    sets (13 GB) are cycled, so nothing is served from the 256 MB Infinity Cache.
    -> (dominant, extra): `dominant` = the gate|up projection (RMSNorm + SiLU*up fused), the largest single kernel of the timed
    step by time (profiles/r03_bench_kernel_stats.txt); `extra` = {"roofline_nhidden": o_proj + down_proj with the residual add
    as the step dispatches them, "roofline_qkv": q|k|v + RMSNorm + RoPE + append}."""
    import torch
    from promptcache_amd import _native as n
    m = lm.hf_model
    c = m.config
    hid, inter, HD, H, Hkv, D = c.hidden_size, c.intermediate_size, m.H * m.D, m.H, m.Hkv, m.D
    mt = (T + 15) // 16
    x = torch.randn((T, hid), device=m.device)
    xres = torch.zeros((T, hid), device=m.device)
    xh, xl = n.to_act_frags(x)
    ah, al = n.to_act_frags(torch.randn((T, HD), device=m.device))
    ch, cl = n.to_act_frags(torch.randn((T, inter), device=m.device))
    oh = torch.empty((mt, inter // 32, 64, 8), dtype=torch.float16, device=m.device)
    ol = torch.empty_like(oh)
    cs = torch.zeros((T, D // 2, 2), dtype=torch.float32, device=m.device); cs[..., 0] = 1
    q16 = torch.empty((T, HD), dtype=torch.float16, device=m.device); q16l = torch.empty_like(q16)
    kv = torch.zeros((2, Hkv, 64, D), dtype=torch.float16, device=m.device)
    fused = T <= m.NORM_FUSED_MAX_ROWS and m.fuse_norm      # what the timed step launches for this many rows
    ks_down = fused and m.ks_down and T >= m.ks_min_rows and inter >= 2 * hid
    ev = {"gu": [], "o": [], "down": [], "qkv": []}

    def timed(key, fn, keep):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); fn(); e1.record()
        if keep:
            ev[key].append((e0, e1))

    def down(lw):
        if ks_down:
            sc, ctr = m._ks_buffers(hid)
            n.gemm_skinny_ks(lw["wdown_f"], ch, cl, T, hid, inter, xres, hid, m.ks_down[1], m.ks_down[0], sc, ctr)
        else:
            n.gemm_skinny(lw["wdown_f"], ch, cl, T, hid, inter, n.EPI_ADD, y=xres, ldy=hid)

    for rep_ in range(3):
        for lw in m.layers:
            if fused:
                timed("qkv", lambda: n.gemm_qkv_rope_norm(lw["wqkv_f"], x, lw["ln1"], c.rms_norm_eps, T, hid, cs, q16, q16l, HD, kv[0], kv[1],
                                                          0, 64 * D, 1, H, Hkv, D, T, 0, 64), rep_ > 0)
                timed("gu", lambda: n.gemm_skinny_norm(lw["wgu_f"], x, lw["ln2"], c.rms_norm_eps, T, 2 * inter, hid, n.EPI_SILU,
                                                       of_hi=oh, of_lo=ol), rep_ > 0)
                timed("o", lambda: n.gemm_skinny(lw["wo_f"], ah, al, T, hid, HD, n.EPI_ADD, y=xres, ldy=hid), rep_ > 0)
                timed("down", lambda: down(lw), rep_ > 0)
            else:
                timed("gu", lambda: n.gemm_skinny(lw["wgu_f"], xh, xl, T, 2 * inter, hid, n.EPI_SILU, of_hi=oh, of_lo=ol), rep_ > 0)
    torch.cuda.synchronize()

    def us(key):
        v = sorted(a.elapsed_time(b) * 1e3 for a, b in ev[key])
        return (sum(v) / len(v), v[0], len(v)) if v else (None, None, 0)

    how = ("HIP events on the launch stream around eager launches on each layer's weights right after the timed region (kernels "
           "inside the captured hipGraph of the timed step cannot be bracketed; event pairs include ~2 us of launch gap); the "
           "in-graph average of the same kernel is in profiles/r03_bench_kernel_stats.txt")
    sig = f"T={T},hid={hid},inter={inter}"
    gu_avg, gu_min, gu_n = us("gu")
    nb_gu = 2 * inter * hid * 2
    tr, src = _pmc_traffic("gemm_skinny_gate_up", sig)
    gate_up = {"kernel": "gemm_skinny_kernel<1,3,EPI_SILU,NORM> (gate|up projection with RMSNorm and SiLU*up fused): the largest "
                         "single kernel of the timed step by time", "bound": "hbm",
               "achieved": nb_gu / (gu_avg * 1e-6) / 1e9, "peak": HBM_PEAK_GBS, "unit": "GB/s",
               "frac": nb_gu / (gu_avg * 1e-6) / 1e9 / HBM_PEAK_GBS, "traffic": tr, "traffic_source": src,
               "algorithmic_bytes_per_launch": nb_gu, "avg_launch_us": gu_avg, "min_launch_us": gu_min, "launches_timed": gu_n,
               "launches_per_step": c.num_hidden_layers, "how": how}
    extra = {}
    if fused:
        o_avg, o_min, o_n = us("o")
        d_avg, d_min, _ = us("down")
        q_avg, q_min, q_n = us("qkv")
        nb_o, nb_d, nb_q = hid * HD * 2, hid * inter * 2, (H + 2 * Hkv) * D * hid * 2
        tr, src = _pmc_traffic("gemm_skinny_add", sig)
        ach = (nb_o + nb_d) / ((o_avg + d_avg) * 1e-6) / 1e9
        extra["roofline_nhidden"] = {
            "kernel": "o_proj (gemm_skinny_kernel<1,1,EPI_ADD>) + down_proj (" +
                      (f"gemm_skinny_ks_kernel: {m.ks_down[0]} tiles x {m.ks_down[1]} K slices, reduced inside the launch"
                       if ks_down else "gemm_skinny_kernel<1,1,EPI_ADD>") + "), residual add fused", "bound": "hbm",
            "achieved": ach, "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": ach / HBM_PEAK_GBS, "traffic": tr, "traffic_source": src,
            "algorithmic_bytes_per_launch": (nb_o + nb_d) / 2, "avg_launch_us": (o_avg + d_avg) / 2, "o_proj_us": o_avg,
            "down_proj_us": d_avg, "min_launch_us": min(o_min, d_min), "launches_timed": 2 * o_n,
            "launches_per_step": 2 * c.num_hidden_layers, "how": how}
        extra["roofline_qkv"] = {"kernel": "gemm_skinny_kernel<1,3,EPI_ROPE,NORM> (q|k|v + RMSNorm + RoPE + in-place KV append)",
                                 "bound": "hbm", "achieved": nb_q / (q_avg * 1e-6) / 1e9, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                                 "frac": nb_q / (q_avg * 1e-6) / 1e9 / HBM_PEAK_GBS, "traffic": _pmc_traffic("gemm_skinny_qkv", sig)[0],
                                 "traffic_source": _pmc_traffic("gemm_skinny_qkv", sig)[1],
                                 "algorithmic_bytes_per_launch": nb_q, "avg_launch_us": q_avg, "min_launch_us": q_min,
                                 "launches_timed": q_n, "launches_per_step": c.num_hidden_layers, "how": how}
    return gate_up, extra


def attn_roofline(lm, staged, q_len: int):
    """Event-time the cached-prefill attention (pc_attn_fwd + its split-KV merge) eagerly on every layer's staged K/V:
    HBM-bound on the K/V stream, bytes = 2*Hkv*(S+q)*D*2 per layer."""
    import torch
    from promptcache_amd import _native as n
    from promptcache_amd.model.kv_arena import arena_from_past
    m = lm.hf_model
    H, Hkv, D = m.H, m.Hkv, m.D
    arena, S = arena_from_past(staged, m.L, Hkv, D)
    q16 = torch.randn((q_len, H * D), device=m.device).half()
    out = torch.empty_like(q16)
    ws = torch.empty(max(n.attn_workspace_bytes(1, H, D, q_len, S + q_len), 4) // 4, dtype=torch.float32, device=m.device)
    plan = arena.pending
    gather_for = lambda li: None                                                    # noqa: E731
    staging = plan is not None
    if staging:
        # the timed step's variant: every staged row read from its module store and written to the arena (pc_attn gather_rows)
        import numpy as np
        arr = np.array([(p_, off, ln) for p_, ln, off in plan.segs], dtype=np.dtype([("src", "<u8"), ("dst_row", "<i4"), ("len", "<i4")]))
        segs = torch.from_numpy(arr.view(np.uint8).copy()).to(m.device)
        words = torch.tensor([len(plan.segs), S + q_len], dtype=torch.int32, device=m.device)
        n.kv_row_table(segs, words[0:1], max(len(plan.segs), 1), words[1:2], arena.buf, Hkv, D, arena.cap, arena.row_table())
        gather_for = lambda li: (arena.row_tab, li * 2 * Hkv, (li * 2 + 1) * Hkv)   # noqa: E731
    evs = []
    for rep_ in range(3):
        for li in range(m.L):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            n.attn_fwd(q16, q_len * H * D, H * D, arena.k_plane(li), arena.v_plane(li), arena.batch_stride, arena.head_stride,
                       out, q_len * H * D, H * D, 1, H, Hkv, D, q_len, S, m.softmax_scale, ws, q_lo=q16, gather=gather_for(li))
            e1.record()
            if rep_ > 0:
                evs.append((e0, e1))
    torch.cuda.synchronize()
    us = sorted(a.elapsed_time(b) * 1e3 for a, b in evs)
    avg = sum(us) / len(us)
    nbytes = 2 * Hkv * (S + q_len) * D * 2 + 2 * H * q_len * D * 2 + (2 * Hkv * S * D * 2 if staging else 0)
    return {"kernel": ("attn_small_kernel<128, GATHER> + attn_combine_kernel (pc_attn gather_rows: module K/V read once, staged rows "
                       "written as they pass)" if staging else "attn_small_kernel<128> + attn_combine_kernel (pc_attn, cached prefill)"),
            "staging": staging, "bound": "hbm",
            "achieved": nbytes / (avg * 1e-6) / 1e9, "peak": HBM_PEAK_GBS, "unit": "GB/s",
            "frac": nbytes / (avg * 1e-6) / 1e9 / HBM_PEAK_GBS,
            "traffic": _pmc_traffic("attn_staging" if staging else "attn_cached", f"H={H},Hkv={Hkv},D={D},q={q_len},S={S}")[0],
            "traffic_source": _pmc_traffic("attn_staging" if staging else "attn_cached", f"H={H},Hkv={Hkv},D={D},q={q_len},S={S}")[1],
            "algorithmic_bytes_per_launch": nbytes, "avg_launch_us": avg, "min_launch_us": us[0],
            "launches_timed": len(us), "launches_per_step": m.L,
            "how": "HIP events around eager pc_attn calls (two kernels: split-KV attention + merge) on each layer's "
                   "staged K/V after the timed region; latency-bound at this size (28.5 MB per launch), see DESIGN.md 3.2"}


def attn_many_roofline(lm, q_len: int, S: int):
    """Event-time the many-row attention (> 64 new rows over S staged keys: pc_attn_ring.hip + the split-KV merge) on synthetic
    operands of the model's shape, called as the forward calls it (split-precision Q, residual rows of the pass, fragment output
    up to 512 rows) -- in the form the step runs: STAGING (every key row read from a module store through the row table and written
    to the arena as its stage lands) when the forward fuses the gather, and the plain launch over a staged arena beside it.  The
    launches walk over Lr layers of K/V (~2 GB: nothing is found in the MALL, as inside a forward) and the two forms alternate.
    MFMA-bound: algorithmic flops = 4 H D q (S + (q + 1) / 2) per launch; the kernel executes twice that (Q and
    P enter as hi + lo pairs)."""
    import numpy as np
    import torch
    from promptcache_amd import _native as n
    m = lm.hf_model
    H, Hkv, D, dev = m.H, m.Hkv, m.D, m.device
    cap = S + q_len + 64
    Lr = max(2, min(12, int(2.2e9 / (2 * Hkv * cap * D * 2))))
    arena = torch.randn((Lr, 2, Hkv, cap, D), device=dev).half()
    q16 = torch.randn((q_len, H * D), device=dev).half()
    q16l = (torch.randn((q_len, H * D), device=dev) * 2 ** -11).half()
    lo = torch.zeros((2, Hkv, q_len + 64, D), device=dev).half()
    frag = q_len <= 512
    mt = (q_len + 15) // 16
    ah = torch.empty((mt, H * D // 32, 64, 8), dtype=torch.float16, device=dev)
    al = torch.empty_like(ah)
    out = torch.empty((q_len, H * D), dtype=torch.float16, device=dev)
    ws = torch.empty(max(n.attn_workspace_bytes(1, H, D, q_len, S + q_len), 4) // 4, dtype=torch.float32, device=dev)
    kvlo = (lo[0], lo[1], Hkv * (q_len + 64) * D, (q_len + 64) * D, -1)
    staging = bool(getattr(m, "supports_fused_gather", False)) and frag and D == 128 and os.environ.get("PC_DEFER_GATHER", "1") != "0"
    rows = None
    if staging:
        store = torch.randn((Lr, 2, Hkv, S, D), device=dev).half()
        seg = np.zeros(1, dtype=np.dtype([("src", "<u8"), ("dst_row", "<i4"), ("len", "<i4")]))
        seg[0] = (store.data_ptr(), 0, S)
        segs = torch.from_numpy(seg.view(np.uint8).copy()).to(dev)
        words = torch.tensor([1, S + q_len], dtype=torch.int32, device=dev)
        rows = torch.zeros(cap * 16, dtype=torch.uint8, device=dev)
        n.kv_row_table(segs, words[0:1], 64, words[1:2], arena, Hkv, D, cap, rows)
        staging = bool(n.attn_gather_ok(q16, q_len * H * D, H * D, arena[0, 0], arena[0, 1], 2 * Hkv * cap * D, cap * D, None, 0, 0, 1, H,
                                        Hkv, D, q_len, S, m.softmax_scale, ws, out_frag=(ah, al), q_lo=q16l, kv_lo=kvlo))

    def one(li, gather):
        if frag:
            n.attn_fwd(q16, q_len * H * D, H * D, arena[li, 0], arena[li, 1], 2 * Hkv * cap * D, cap * D, None, 0, 0, 1, H, Hkv, D, q_len,
                       S, m.softmax_scale, ws, out_frag=(ah, al), q_lo=q16l, kv_lo=kvlo,
                       gather=(rows, li * 2 * Hkv, (li * 2 + 1) * Hkv) if gather else None)
        else:
            n.attn_fwd(q16, q_len * H * D, H * D, arena[li, 0], arena[li, 1], 2 * Hkv * cap * D, cap * D, out, q_len * H * D, H * D, 1, H,
                       Hkv, D, q_len, S, m.softmax_scale, ws, q_lo=q16l, out_lo=torch.empty_like(out), kv_lo=kvlo)

    forms = [False, True] if staging else [False]
    evs = {f: [] for f in forms}
    for i in range(3 * m.L):
        for vi, f in enumerate(forms):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            one((len(forms) * i + vi) % Lr, f)
            e1.record()
            if i >= m.L:
                evs[f].append((e0, e1))
    torch.cuda.synchronize()
    us = {f: sorted(a.elapsed_time(b) * 1e3 for a, b in evs[f]) for f in forms}
    avg = sum(us[staging]) / len(us[staging])
    flops = 4.0 * H * D * q_len * (S + (q_len + 1) / 2)
    kv_bytes = 2 * Hkv * S * D * 2
    wide = S >= int(os.environ.get("PC_ATTN_WIDE_MIN", "6144")) and q_len >= int(os.environ.get("PC_ATTN_WIDE_MIN_ROWS", "128")) \
        and os.environ.get("PC_ATTN_NO_WIDE") != "1"
    res = {"kernel": (("attn_wide_kernel<GATHER, R> over the staged keys (all query rows of a head per workgroup, key slices; "
                       "pc_attn_wide.hip) + attn_ring_kernel<KVLO> over the pass's own rows" if wide else "attn_ring_kernel<KVLO, GATHER>") +
                      (" (stages while it reads: pc_attn gather_rows)" if staging else "")) +
                     " + attn_combine_kernel (pc_attn, > 64 split-precision rows): ALL launches of one pc_attn call inside the events",
           "staging": staging, "bound": "mfma", "achieved": flops / (avg * 1e-6) / 1e12, "peak": MFMA_PEAK_TFLOPS, "unit": "TFLOP/s",
           "frac": flops / (avg * 1e-6) / 1e12 / MFMA_PEAK_TFLOPS, "executed_frac": 2 * flops / (avg * 1e-6) / 1e12 / MFMA_PEAK_TFLOPS,
           "traffic": _pmc_traffic("attn_wide_staging" if wide else "attn_ring_staging", f"H={H},Hkv={Hkv},D={D},q={q_len},S={S}")[0] if staging else None,
           "traffic_source": _pmc_traffic("attn_wide_staging" if wide else "attn_ring_staging", f"H={H},Hkv={Hkv},D={D},q={q_len},S={S}")[1] if staging else None,
           "algorithmic_flops_per_launch": flops, "avg_launch_us": avg, "min_launch_us": us[staging][0],
           "launches_timed": len(us[staging]), "launches_per_step": m.L, "q_len": q_len, "staged_keys": S,
           "hbm_bytes_per_launch_algorithmic": (2 if staging else 1) * kv_bytes,
           "hbm_GBps": (2 if staging else 1) * kv_bytes / (avg * 1e-6) / 1e9,
           "how": "HIP events around eager pc_attn calls (ring kernel + split-KV merge) on synthetic K/V of the model's shape, "
                  f"{Lr} layers of K/V cycled (cache-cold); frac = algorithmic flops (one plane) / 2.5 PFLOP/s, executed_frac counts the "
                  "hi + lo planes of Q and P; hbm_*: module K/V read once (+ written once when staging)"}
    if staging:
        res["plain_launch_us"] = sum(us[False]) / len(us[False])
    return res


def config_workload(cfg: int):
    """BASELINE.json configs 2-4 as synthetic PML with each config's structure (no datasets or
    checkpoints offline) -> (model shape name, max_ctx, max_tokens, [(schema_pml, prompt_pml), ...], label)."""
    import numpy as np
    from promptcache_amd import synth
    if cfg == 2:     # examples/code_generation_game.xml via demo.py:46-77: 11 segments, 5 x 800-token documents, max_tokens=800
        return "llama2-7b", 5000, 800, [synth.flat_docs("game", 30, (306, 76, 800, 800, 800, 800, 800), 12)], \
            "llama2-7b shape, code_generation_game-structured schema (S ~ 4.4 k), max_ctx 5000"
    if cfg == 3:     # benchmark/squad_v2.py: one context module per entry, question 10-30 tokens (benchmark/squad_v2.py:36-57)
        rng = np.random.default_rng(0)
        ents = [synth.flat_docs(f"squad{i}", 20, (int(rng.integers(100, 400)),), int(rng.integers(10, 30)), seed=i + 1)
                for i in range(8)]
        return "codellama-7b", 4096, 3500, ents, "codellama-7b shape (theta 1e6), 8 SQuAD-structured entries (S 120-420)"
    # benchmark/longbench.py:102-132: one 8 k-token context module, question ~250 tokens; max_ctx 9186 (llm_config_longchat_7b.json)
    return "llama2-13b", 9186, 8192, [synth.flat_docs("longbench", 10, (8000,), 255)], \
        "llama2-13b shape, LongBench-structured 8 k context, q ~ 260, max_ctx 9186"


def run_config(args, device, world, rank, barrier):
    result = measure_config(args.config, args.steps, args.warmup, device, world, rank, barrier,
                            dump_dir=args.dump_outputs if rank == 0 else None)
    if rank == 0:
        print(json.dumps(result))


def measure_config(cfg, steps, warmup, device, world, rank, barrier, lm=None, repeats: int = 3, attention_leg: bool = True,
                   dump_dir=None):
    """BASELINE.json configs 2-4 with the reference's latency recipe (eval.py:172-219, eval_sys.py:29): for every entry
    add_schema -> process -> first lm() call, the cached run and the no_cache run, ``repeats`` repeats each.  The timed region
    is K cached steps (one step = CacheEngine.process + first forward of the next entry, entries cycled, schemas resident).
    ``lm``: a resident model of the config's shape to reuse (the default run's ``configs`` leg reuses the headline 7b model for
    config 2).  ``dump_dir``: ``--dump-outputs`` of the last timed step."""
    import torch
    import torch.distributed as dist
    from promptcache_amd import CacheEngine, Prompt
    from promptcache_amd.model import Llama2
    args = argparse.Namespace(config=cfg, steps=steps, warmup=warmup)
    name, max_ctx, max_tokens, entries, label = config_workload(args.config)
    if lm is None:
        lm = Llama2(name, device=device, random_init=True, seed=0)
    eng = CacheEngine(max_ctx, lm)
    fmt = lm.get_formatter()
    t0 = time.perf_counter()
    for sp, _ in entries:
        eng.add_schema(fmt(sp), max_tokens=max_tokens)
    torch.cuda.synchronize()
    t_enc = time.perf_counter() - t0
    prompts = [Prompt(pp, [fmt]) for _, pp in entries]
    pc = eng.prompt_cache
    last = {}

    def one(prompt, no_cache):
        pc.reset()
        ids, pos, cache_ms, cache = eng.process(prompt, no_cache=no_cache)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        last["out"] = lm(input_ids=torch.tensor([list(ids)], dtype=torch.long), position_ids=torch.tensor([pos], dtype=torch.long),
                         past_key_values=cache, use_cache=True)
        e1.record()
        torch.cuda.synchronize()
        last["ids"], last["pos"] = ids, pos
        return len(ids), (0 if cache is None else len(pc)), cache_ms, e0.elapsed_time(e1)

    per_entry = []
    for pr in prompts:                                     # the reference's per-entry numbers (3 repeats, eval_sys.py:29)
        ent = {}
        for mode, nc in (("cached", False), ("no_cache", True)):
            runs = [one(pr, nc) for _ in range(repeats + 1)][1:]     # first run of a shape pays hipGraph capture / code-object load
            ent[mode] = {"new_tokens": runs[0][0], "staged_tokens": runs[0][1],
                         "cache_time_ms": [r[2] for r in runs], "response_time_ms": [r[3] for r in runs],
                         "ttft_ms": min(r[2] + r[3] for r in runs)}
        ent["speedup"] = ent["no_cache"]["ttft_ms"] / ent["cached"]["ttft_ms"]
        per_entry.append(ent)
    for i in range(args.warmup):
        one(prompts[i % len(prompts)], False)
    barrier()
    t0 = time.perf_counter()
    tok = 0
    for i in range(args.steps):
        q, S, _, _ = one(prompts[i % len(prompts)], False)
        tok += q + S
    barrier()
    elapsed = time.perf_counter() - t0
    if dist.is_initialized():
        t = torch.tensor([elapsed], device=device, dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())
    if dump_dir:
        dump_outputs(dump_dir, step_outputs(last["out"], last["ids"], last["pos"]))
    ms = elapsed / args.steps * 1e3
    L, Hkv, D = lm.get_cache_shape()
    c = lm.hf_model.config
    w_bytes = 2 * (c.num_hidden_layers * (c.hidden_size * (lm.hf_model.H + 2 * Hkv) * D + lm.hf_model.H * D * c.hidden_size +
                                          3 * c.hidden_size * c.intermediate_size) + c.vocab_size * c.hidden_size)
    kvb = 2 * L * Hkv * D * 2
    mean_tok = tok / args.steps
    step_bytes = w_bytes + 3 * mean_tok * kvb          # gather read + write, staged K/V read once
    gbs = step_bytes / (ms * 1e-3) / 1e9
    result = {"metric": "cached_prefill_tokens_per_s", "value": world * tok / elapsed, "unit": "tokens/s", "n_gpus": world,
              "steps": args.steps, "warmup": args.warmup, "ms_per_step": ms, "higher_is_better": True, "scaling": "weak",
              "vs_baseline": None, "dtype": "f16", "data": "synthetic",
              "config": {"workload": f"BASELINE config {args.config}: {label}; step = CacheEngine.process (gather) + first lm() "
                                     f"call of one entry (entries cycled)", "entries": len(entries), "replicas": world},
              "ttft_ms": ms,
              "roofline": {"bound": "hbm", "achieved": gbs, "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": gbs / HBM_PEAK_GBS,
                           "traffic": None, "kernel": "whole step (weights once + gather read/write + staged K/V once)",
                           "algorithmic_bytes_per_step": step_bytes,
                           "note": "q > 64 rows (config 4) leaves the weight-streaming regime; per-kernel figures: bench.py --config 1"},
              "encode_seconds": t_enc, "entries": per_entry,
              "recipe": f"reference eval.py:172-219: per entry cache_time + response_time, cached and no_cache, best of {repeats}"}
    q0, S0 = per_entry[0]["cached"]["new_tokens"], per_entry[0]["cached"]["staged_tokens"]
    if rank == 0 and q0 > 64 and lm.hf_model.D == 128 and attention_leg:
        result["roofline_attention"] = attn_many_roofline(lm, q0, S0)
    for nm in list(eng.schemas):
        eng.remove_schema(nm)
    return result


def configs_leg(device, world, rank, barrier, lm7b):
    """The other single-GPU BASELINE configs, compact, on the DEFAULT run's JSON line (the driver only runs
    ``bench.py`` with default arguments, so configs 2-4 were builder-run claims): per config the cached step (ms, whole-step HBM
    roofline fraction), staged / new tokens of the first entry, and the no_cache TTFT beside it.  Fewer steps and one repeat less
    than ``--config N`` (which stays the full per-entry recipe)."""
    import torch
    out = {}
    for cfg, steps, warm in ((2, 30, 5), (3, 48, 8), (4, 12, 3)):
        t0 = time.perf_counter()
        r = measure_config(cfg, steps, warm, device, world, rank, barrier, lm=lm7b if cfg == 2 else None, repeats=2,
                           attention_leg=(cfg == 4))
        e0 = r["entries"][0]
        out[str(cfg)] = {"ms_per_step": r["ms_per_step"], "frac": r["roofline"]["frac"], "tokens_per_s": r["value"],
                         "S": e0["cached"]["staged_tokens"], "q": e0["cached"]["new_tokens"], "entries": len(r["entries"]),
                         "steps": steps, "no_cache_ttft_ms": sum(e["no_cache"]["ttft_ms"] for e in r["entries"]) / len(r["entries"]),
                         "cached_ttft_ms_entries": [round(e["cached"]["ttft_ms"], 3) for e in r["entries"]],
                         "workload": r["config"]["workload"], "leg_seconds": None}
        if "roofline_attention" in r:
            ra = r["roofline_attention"]
            out[str(cfg)]["roofline_attention"] = {k: ra[k] for k in ("frac", "achieved", "unit", "avg_launch_us", "bound") if k in ra}
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        out[str(cfg)]["leg_seconds"] = round(time.perf_counter() - t0, 2)
    out["what"] = ("BASELINE configs 2-4 inside the default run: ms_per_step = K cached steps (CacheEngine.process + first lm() call, "
                   "entries cycled), frac = (weights once + gather read/write + staged K/V once) / ms_per_step / 8 TB/s; "
                   "`python bench.py --config N` prints the full per-entry recipe")
    return out


def plan_only(args):
    """``--plan-only`` (CPU, no GPU, no torch.cuda): the schedule of the schema-library encode (BASELINE config 5) for 1 / 2 / 4 /
    8 ranks from the token layout alone -- rows every rank runs through the model, bytes it receives in the module-KV exchange,
    and the speed-ups they predict at a given 1-GPU encode rate and xGMI link rate.  One JSON object on stdout."""
    import types
    from promptcache_amd import pml, synth
    from promptcache_amd.cache_engine import CacheEngine, SchemaCache
    from promptcache_amd.model import _llama_formatter
    from promptcache_amd.model.config import SHAPES
    from promptcache_amd.model.tokenizer import StandInTokenizer
    shape = SHAPES[args.model]
    tok = StandInTokenizer(shape.vocab_size)
    lm = types.SimpleNamespace(hf_tokenizer=tok, unk_token_id=0, eos_token_id=2, encode=tok.encode, use_full_position_ids=False,
                               hf_model=types.SimpleNamespace(batch_invariant=True, supports_ragged_past=True, supports_shared_prefix=True))
    # measured rows-per-forward -> seconds curve of the 1-GPU encode (tools/encode_rate_curve.py, committed under profiles/): a
    # forward of a few hundred rows runs well below the large-M rate, so pricing every rank's rows at ONE rate over-predicts
    curve = None
    cpath = args.plan_curve or os.path.join(ROOT, "profiles", "r04_encode_rate_curve.json")
    if os.path.exists(cpath):
        with open(cpath) as f:
            cj = json.load(f)
        if cj.get("model") == args.model:
            curve = sorted((int(p_["rows"]), float(p_["seconds"])) for p_ in cj["points"])

    def fwd_seconds(rows: int) -> float:
        """Piecewise-linear interpolation of the measured curve (through the origin below its first point, the last point's rate
        beyond its end)."""
        if rows <= curve[0][0]:
            return curve[0][1] * max(rows, 1) / curve[0][0] if rows > curve[0][0] // 2 else curve[0][1] * 0.75
        for (r0, t0), (r1, t1) in zip(curve, curve[1:]):
            if rows <= r1:
                return t0 + (t1 - t0) * (rows - r0) / (r1 - r0)
        return curve[-1][1] * rows / curve[-1][0]
    fmt = _llama_formatter()
    texts = [synth.persona_like(name=f"lib-persona-{i}", system_len=200 + 40 * i, seed=20 + i)[0] for i in range(5)]
    texts += [synth.flat_docs(f"lib-docs-{i}", 30, lens, 8, seed=30 + i)[0]
              for i, lens in enumerate([(306, 76, 800, 800, 800), (1500, 1200), (400,) * 6])]

    def caches_of(texts):
        out = []
        for t in texts:
            sc = SchemaCache.__new__(SchemaCache)
            sc.lm, sc._jobs = lm, None
            sc.schema = pml.Schema(fmt(t), lm)
            out.append(sc)
        return out

    kvb = shape.kv_bytes_per_token
    rate, link = args.plan_rate, args.plan_link_gbs * 1e9
    out = {"what": "predicted multi-GPU schema-encode schedule (CacheEngine.library_schedule / parallel.plan_library), host arithmetic only",
           "model": args.model, "kv_bytes_per_token": kvb, "assumed_1gpu_tokens_per_s": rate, "assumed_link_GBps": args.plan_link_gbs,
           "workloads": {}}
    for name, caches in (("library (config 5 stand-in: 5 persona-structured + 3 document schemas)", caches_of(texts)),
                         ("persona schema alone (the headline schema)", caches_of([synth.persona_like()[0]]))):
        items = [c.plan_items() for c in caches]
        scaffold_tokens = sum(len(j["token_ids"]) for c in caches for j in c._plan())
        one = sum(c.plan_cost() for c in caches)
        rows = []
        t_one_curve = None
        for world in (1, 2, 4, 8):
            order, shards = CacheEngine.library_schedule(caches, world)
            loads, rx, rx_last, t_curve = [0] * world, [0] * world, [0] * world, [0.0] * world
            for k in order:
                trunk, costs, needs = items[k]
                jobs = caches[k]._plan_with_prefix()[0]
                own = [0] * world
                for r in range(world):
                    mine = list(range(len(costs))) if world == 1 else shards[k][r]
                    if mine:
                        loads[r] += (trunk if any(needs[i] for i in mine) else 0) + sum(costs[i] for i in mine)
                        if curve:
                            t_curve[r] += sum(fwd_seconds(f) for f in caches[k].plan_forwards(mine))
                    own[r] = sum(len(tc) for i in mine for tc in jobs[i]["owned"]) * kvb
                for r in range(world):
                    rx[r] += sum(own) - own[r]
                    if k == order[-1]:
                        rx_last[r] = sum(own) - own[r]
            row_rate = rate * one / scaffold_tokens          # computed rows per second at the assumed scaffold-token rate
            t_comp = max(loads) / row_rate
            links = max(world - 1, 1) * link
            t_rx_all, t_rx_last = max(rx) / links, max(rx_last) / links
            extra = {}
            if curve:
                if world == 1:
                    t_one_curve = t_curve[0]
                extra = {"seconds_compute_by_measured_curve": round(max(t_curve), 4),
                         "predicted_speedup_by_measured_curve": round(t_one_curve / (max(t_curve) + t_rx_last), 2),
                         "predicted_speedup_by_measured_curve_exchange_exposed": round(t_one_curve / (max(t_curve) + t_rx_all), 2)}
            lib_bytes = sum(len(tc) for c in caches for j in c._plan_with_prefix()[0] for tc in j["owned"]) * kvb
            rows.append({"ranks": world, "per_rank_computed_rows": loads, "compute_speedup": round(one / max(loads), 2), **extra,
                         "exchange_rx_bytes_per_rank_max": int(max(rx)),
                         # what a rank ALLOCATES for the exchange: one receive slab per peer and schema at its exact size
                         # (parallel.exchange_slabs; the received segments are used in place) -- next to its own slabs that makes
                         # the whole library resident on every rank, as the reference keeps it on its one device
                         "receive_buffer_bytes_per_rank": [int(b) for b in rx],
                         "library_bytes_resident_per_rank": int(lib_bytes),
                         "seconds_compute": round(t_comp, 4), "seconds_exchange_if_fully_exposed": round(t_rx_all, 4),
                         "seconds_exchange_last_schema": round(t_rx_last, 4),
                         "predicted_speedup_overlapped": round((one / row_rate) / (t_comp + t_rx_last), 2),
                         "predicted_speedup_exchange_exposed": round((one / row_rate) / (t_comp + t_rx_all), 2)})
        out["workloads"][name] = {"schemas": len(caches), "scaffold_tokens": scaffold_tokens, "computed_rows_one_rank": one,
                                  "by_ranks": rows}
    out["measured_curve"] = None if not curve else {"file": os.path.relpath(cpath, ROOT), "points": len(curve),
                                                     "what": "seconds of ONE encode forward (many_rows, kv_only) by its row count, 1 GPU; "
                                                             "*_by_measured_curve price every forward of every rank on it instead of one rate"}
    out["memory_note"] = ("every rank ends with the whole module library resident (own slabs + receive slabs = "
                          "library_bytes_resident_per_rank, independent of the rank count): fine at 288 GB of HBM per GPU, and what "
                          "CacheEngine.process needs -- any prompt may name any module")
    out["note"] = ("compute_speedup = rows of a one-rank encode / rows of the most loaded rank (a rank that takes passes of a schema "
                   "re-runs its trunk); seconds_* price rows at the assumed scaffold-token rate (computed rows cost "
                   "scaffold_tokens / computed_rows of a scaffold token each) and the exchange at (ranks - 1) links of the "
                   "assumed rate (one grouped point-to-point step: an owner's slab leaves over ranks - 1 links at once); "
                   "'overlapped' leaves only the LAST schema's exchange exposed (every earlier one runs under later encodes)")
    print(json.dumps(out))


def encode_legs(args, eng, lm, fmt, schema_pml, t_first, world, rank, device, barrier):
    """--full: the persona schema's encode again in steady state (``encode``) and the schema-library encode of BASELINE config 5
    (``encode_library``, unless --no-library), both sharded over the ranks."""
    import torch
    import torch.distributed as dist
    from promptcache_amd import synth
    eng.remove_schema("persona")
    barrier()
    t0 = time.perf_counter()
    eng.add_schema(fmt(schema_pml))
    barrier()
    t_enc = time.perf_counter() - t0
    sc = eng.schemas["persona"]
    enc_tokens = sum(len(j["token_ids"]) for j in sc._plan())
    lib_ok = None
    if dist.is_initialized():
        # after the all-gather every rank must hold the same module library: compare a per-segment checksum
        sig = torch.stack([c.store.float().abs().sum() + c.store.float().sum() * 3.0
                           for _, c in sorted(sc.cache_l1.items(), key=lambda kv: (kv[1].token_sequence.offset, len(kv[1])))])
        lo, hi = sig.clone(), sig.clone()
        dist.all_reduce(lo, op=dist.ReduceOp.MIN)
        dist.all_reduce(hi, op=dist.ReduceOp.MAX)
        lib_ok = bool(torch.equal(lo, hi))
    mcfg = lm.hf_model.config
    _hm = lm.hf_model
    _macs = {"qkv": mcfg.hidden_size * (_hm.H + 2 * _hm.Hkv) * _hm.D, "o": _hm.H * _hm.D * mcfg.hidden_size,
             "gu": 2 * mcfg.hidden_size * mcfg.intermediate_size, "down": mcfg.hidden_size * mcfg.intermediate_size}
    macs_tok = sum(_macs.values())                                         # projection MACs per token per layer
    # activation planes the MFMAs run, averaged over the projections (hi + lo, except the projections on the hi plane only)
    planes = (sum(m_ * (1 if k_ in getattr(_hm, "dense_lo_skip", ()) else 2) for k_, m_ in _macs.items()) / macs_tok) if _hm.precise_dense else 1
    comp_tokens = int(sc.encode_stats["computed_tokens"])
    enc_flops_alg = 2.0 * macs_tok * mcfg.num_hidden_layers * comp_tokens          # 2 * P per token that runs
    enc_flops = planes * enc_flops_alg                                              # what the MFMAs execute (hi + lo planes)
    enc_per_rank = [comp_tokens]
    if dist.is_initialized():
        t = torch.zeros(world, dtype=torch.int64, device=device)
        t[rank] = enc_per_rank[0]
        dist.all_reduce(t)
        enc_per_rank = [int(v) for v in t.tolist()]
    exchange = None
    if world > 1:
        # the module-KV exchange of this schema, alone and blocking (seconds) next to what the encode did not hide of it (exposed)
        t = torch.tensor([sc.reexchange_seconds(), float(sc.encode_stats.get("exchange_exposed_s", 0.0)),
                          float(sc.encode_stats.get("exchange_bytes_rx", 0))], device=device, dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        exchange = {"seconds": float(t[0]), "exposed_seconds": float(t[1]), "bytes_received_per_rank_max": int(t[2]),
                    "GBps_per_rank": float(t[2]) / max(float(t[0]), 1e-9) / 1e9,
                    "what": "seconds: the grouped point-to-point exchange (parallel.exchange_slabs) run again alone, blocking, max over "
                            "ranks; exposed_seconds: what the timed encode waited for it (a single schema has nothing to hide it under)"}
    encode = {"per_rank_computed_tokens": enc_per_rank, "exchange": exchange,
              "roofline": {"bound": "mfma", "achieved": enc_flops_alg / t_enc / 1e12, "peak": 2500.0, "unit": "TFLOP/s",
                           "frac": enc_flops_alg / t_enc / 1e12 / 2500.0, "traffic": None,
                           "executed_TFLOPs": enc_flops / t_enc / 1e12, "executed_frac": enc_flops / t_enc / 1e12 / 2500.0,
                           "reference_work_TFLOPs": 2.0 * macs_tok * mcfg.num_hidden_layers * enc_tokens / t_enc / 1e12,
                           "what": "frac: ALGORITHMIC projection flops (2 x MACs x layers x the tokens that ran through the model; "
                                   "padding rows and attention not counted) / wall time of the whole add_schema call, against the dense "
                                   f"fp16 MFMA peak; executed_*: the same x {planes:.2f} activation plane(s) on average (what the MFMAs run for the "
                                   "split-precision parity); reference_work_*: 2 x MACs x every scaffold token as the reference encodes "
                                   "them (every scaffold in full) / the same wall time -- what trunk reuse and scaffold cutting buy; "
                                   "kernel-level rates: profiles/r02_encode_kernel_stats.txt"},
              "passes": int(sc.encode_stats["total_passes"]), "tokens": int(enc_tokens),
              "cached_tokens": int(sc.encode_stats["cached_tokens"]), "seconds": t_enc,
              "tokens_per_s": enc_tokens / t_enc, "sharded_over": world,
              "first_call_seconds": t_first, "library_identical_on_all_ranks": lib_ok,
              "computed_tokens": int(sc.encode_stats["computed_tokens"]),
              "trunk_shared_passes": int(sc.encode_stats["trunk_shared_passes"]),
              "note": "second add_schema call (steady state); tokens = scaffold tokens as the reference encodes them "
                      "(every scaffold in full); computed_tokens = what ran through the model: scaffolds sharing a "
                      "prefix with the root scaffold are encoded as suffixes over its K/V; passes packed into "
                      "right-padded batches, sharded over the ranks, module KV all-gathered"}

    # ---- module-library encode (BASELINE config 5: a whole schema library, ~150 passes / ~100 k tokens) ----
    # five persona-structured schemas of different sizes + three flat document schemas; every schema's passes are
    # sharded over the ranks and its module KV all-gathered, exactly like the single schema above
    library = None
    if not args.no_library:
        lib_schemas = [synth.persona_like(name=f"lib-persona-{i}", system_len=200 + 40 * i, seed=20 + i)[0] for i in range(5)]
        lib_schemas += [synth.flat_docs(f"lib-docs-{i}", 30, lens, 8, seed=30 + i)[0]
                        for i, lens in enumerate([(306, 76, 800, 800, 800), (1500, 1200), (400,) * 6])]
        lib_runs = []
        for rep_ in range(2):       # (host tokenisation + planning are part of it: the first call also pays cold allocations)
            for n in [n for n in eng.schemas if n.startswith("lib-")]:
                eng.remove_schema(n)
            barrier()
            t0 = time.perf_counter()
            eng.add_schemas([fmt(text) for text in lib_schemas])   # schema-level sharding + overlapped exchange (N > 1)
            barrier()
            lib_runs.append(time.perf_counter() - t0)
        t_lib = min(lib_runs)
        names = [n for n in eng.schemas if n.startswith("lib-")]
        lib_tokens = sum(sum(len(j["token_ids"]) for j in eng.schemas[n]._plan()) for n in names)
        lib_passes = sum(int(eng.schemas[n].encode_stats["total_passes"]) for n in names)
        lib_cached = sum(int(eng.schemas[n].encode_stats["cached_tokens"]) for n in names)
        mine_comp = int(sum(eng.schemas[n].encode_stats["computed_tokens"] for n in names))
        per_rank = [mine_comp]
        if dist.is_initialized():
            t = torch.zeros(world, dtype=torch.int64, device=device)
            t[rank] = mine_comp
            dist.all_reduce(t)
            per_rank = [int(v) for v in t.tolist()]
        lib_exchange = None
        if world > 1:
            t = torch.tensor([sum(eng.schemas[n].reexchange_seconds() for n in names),
                              sum(float(eng.schemas[n].encode_stats.get("exchange_exposed_s", 0.0)) for n in names),
                              float(sum(eng.schemas[n].encode_stats.get("exchange_bytes_rx", 0) for n in names))],
                             device=device, dtype=torch.float64)
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            lib_exchange = {"seconds": float(t[0]), "exposed_seconds": float(t[1]), "bytes_received_per_rank_max": int(t[2]),
                            "GBps_per_rank": float(t[2]) / max(float(t[0]), 1e-9) / 1e9,
                            "what": "seconds: every schema's exchange run again alone and blocking, summed, max over ranks; "
                                    "exposed_seconds: what the (last) library encode actually waited for -- the exchange of schema k "
                                    "runs under the encode of schema k + 1"}
        library = {"per_rank_computed_tokens": per_rank, "exchange": lib_exchange,
                   "schemas": len(names), "passes": lib_passes, "tokens": int(lib_tokens), "cached_tokens": lib_cached,
                   "module_kv_bytes": int(lib_cached) * lm.hf_model.config.kv_bytes_per_token, "seconds": t_lib,
                   "seconds_runs": lib_runs,
                   "tokens_per_s": lib_tokens / t_lib, "sharded_over": world,
                   "note": "BASELINE config 5 stand-in: synthetic schema library through CacheEngine.add_schemas: whole schemas "
                           "dealt to the ranks (LPT on the tokens each encode really runs; every trunk computed once), slabs "
                           "broadcast from their owners at exact size, exchange of schema k overlapped with the encode of k+1"}
        for n in names:
            eng.remove_schema(n)
    return encode, library


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--config", type=int, default=1, choices=[1, 2, 3, 4],
                    help="BASELINE.json config: 1 = the headline (llama2-7b shape, persona-structured schema); 2 = game-like "
                         "schema (7b, max_ctx 5000); 3 = SQuAD-like entries (CodeLlama-7b); 4 = LongBench-like 8k context (13b). "
                         "2-4 follow the reference's latency recipe (eval.py:172-219): every entry, cached and no_cache")
    ap.add_argument("--model", default="llama2-7b")
    ap.add_argument("--max-ctx", type=int, default=4096)        # config/llm_config_llama2_7b.json of the reference
    ap.add_argument("--cpu-layers", type=int, default=8, help="layers the cpu_baseline TIMING runs (scaled by L/k)")
    ap.add_argument("--parity-layers", type=int, default=0, help="layers of the parity leg (0 = all)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-library", action="store_true", help="skip the schema-library encode leg (BASELINE config 5)")
    ap.add_argument("--no-int8", action="store_true", help="skip the int8-weight context leg (builds a second model)")
    ap.add_argument("--no-configs", action="store_true", help="skip the compact BASELINE config 2-4 legs of the default run")
    ap.add_argument("--no-context", action="store_true", help="skip the extra (untimed) no-cache / decode / GEMM-roofline runs")
    ap.add_argument("--plan-only", action="store_true",
                    help="CPU only: print the predicted 1/2/4/8-GPU schedule of the schema-library encode and exit")
    ap.add_argument("--plan-rate", type=float, default=72000.0, help="--plan-only: 1-GPU library encode rate, scaffold tokens/s")
    ap.add_argument("--plan-link-gbs", type=float, default=153.0, help="--plan-only: one xGMI link, GB/s per direction")
    ap.add_argument("--plan-curve", default="", help="--plan-only: JSON of measured (rows per forward, seconds) points "
                                                      "(default profiles/r04_encode_rate_curve.json when present)")
    ap.add_argument("--full", action="store_true",
                    help="run every leg beside the headline (encode, library, rooflines, context, int8, cpu_baseline, parity, "
                         "configs 2-4); a plain run only sets up, warms up, times the steps and prints the headline")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write what the last timed step returned (logits, new and sampled staged K/V, ids) as DIR/<name>.npy")
    args = ap.parse_args()
    if args.plan_only:
        plan_only(args)
        return

    import torch
    import torch.distributed as dist

    if os.environ.get("PC_BENCH_FAULT_S"):          # dev: dump every thread's stack and exit if the run is still going after N seconds
        import faulthandler
        faulthandler.dump_traceback_later(int(os.environ["PC_BENCH_FAULT_S"]), exit=True)
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={world}: launch with torch.distributed.run for N > 1")
    # test hooks (1-GPU smoke of the N > 1 code path): PC_BENCH_SAME_DEVICE=1 puts every rank on cuda:0 and
    # PC_BENCH_BACKEND=gloo replaces RCCL (which refuses two ranks on one device)
    if os.environ.get("PC_BENCH_SAME_DEVICE") == "1":
        local_rank = 0
    torch.cuda.set_device(local_rank)
    device = f"cuda:{local_rank}"
    if world > 1 or os.environ.get("PC_BENCH_FORCE_DIST") == "1":     # (test hook: a one-rank RCCL group runs the collectives below)
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        backend = os.environ.get("PC_BENCH_BACKEND", "nccl")
        if backend == "nccl":
            dist.init_process_group(backend="nccl", device_id=torch.device(device))
        else:
            dist.init_process_group(backend=backend)

    def barrier():
        if dist.is_initialized():
            dist.barrier()
        torch.cuda.synchronize()

    import __graft_entry__ as ge
    if rank == 0:
        ge.build()
    barrier()
    from promptcache_amd import CacheEngine, Prompt, synth
    from promptcache_amd.model import Llama2

    if args.config != 1:
        run_config(args, device, world, rank, barrier)
        if dist.is_initialized():
            barrier()
            dist.destroy_process_group()
        return
    lm = Llama2(args.model, device=device, random_init=True, seed=0)
    eng = CacheEngine(args.max_ctx, lm)
    fmt = lm.get_formatter()
    schema_pml, prompt_pml = synth.persona_like()

    # ---- schema encode (module KV precompute): sharded over ranks + one all-gather ----
    barrier()
    t0 = time.perf_counter()
    eng.add_schema(fmt(schema_pml))
    barrier()
    t_first = time.perf_counter() - t0           # includes hipBLASLt kernel selection / allocator warm-up
    encode = library = None
    if args.full:
        encode, library = encode_legs(args, eng, lm, fmt, schema_pml, t_first, world, rank, device, barrier)

    prompt = Prompt(prompt_pml, [fmt])
    pc = eng.prompt_cache
    pc.record_events = True
    gather_evs, prefill_evs = [], []

    def step(record: bool):
        pc.reset()                                            # full gather every step
        ids, pos, cache_ms, cache = eng.process(prompt)
        # host tensors, as GenerationEngine._forward hands them over: ids, positions, past length and the staging plan travel
        # in ONE pinned copy in front of the graph replay (PC_DEFER_GATHER=0 + device tensors: the round 1-3 step)
        ids_t = torch.tensor([ids], dtype=torch.long)
        pos_t = torch.tensor([pos], dtype=torch.long)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = lm(input_ids=ids_t, position_ids=pos_t, past_key_values=cache, use_cache=True)
        e1.record()
        torch.cuda.synchronize()      # TTFT ends when the logits are there: the next request's assembly must not hide under this one's forward
        if record:
            if pc.last_gather_events is not None:
                gather_evs.append(pc.last_gather_events)
            prefill_evs.append((e0, e1, cache_ms))
        return ids, pos, out

    for _ in range(args.warmup):
        ids, pos, out = step(False)
    barrier()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        ids, pos, out = step(True)
    barrier()
    elapsed = time.perf_counter() - t0
    if dist.is_initialized():
        t = torch.tensor([elapsed], device=device, dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())
    if rank == 0 and args.dump_outputs:
        dump_outputs(args.dump_outputs, step_outputs(out, ids, pos))

    S, q = len(pc), len(ids)
    ttft_ms = elapsed / args.steps * 1e3
    L, Hkv, D = lm.get_cache_shape()
    fused_gather = len(gather_evs) == 0          # the timed steps staged inside their attention launches: no copy launch to time
    prefill_ms = sorted(a.elapsed_time(b) for a, b, _ in prefill_evs)
    process_ms = sorted(c for _, _, c in prefill_evs)
    alg_bytes = 2 * S * (2 * L * Hkv * D * 2)                # read once + write once

    result = {
        "metric": "cached_prefill_tokens_per_s", "value": world * (S + q) / (ttft_ms * 1e-3), "unit": "tokens/s",
        "n_gpus": world, "steps": args.steps, "warmup": args.warmup, "ms_per_step": ttft_ms,
        "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "f16", "data": "synthetic",
        "config": {"workload": f"{args.model} shape, persona-structured PML schema (synthetic text, 29 encode passes), "
                               f"cached prefill: {len(pc.staged)} staged segments S={S} + q={q} new tokens, "
                               f"max_ctx={args.max_ctx}; step = CacheEngine.process (gather) + first lm() call",
                   "staged_tokens": S, "new_tokens": q, "segments": len(pc.staged), "replicas": world},
        "ttft_ms": ttft_ms,
        "breakdown_ms": {"process_incl_gather_median": process_ms[len(process_ms) // 2],
                         "prefill_median": prefill_ms[len(prefill_ms) // 2],
                         "new_token_tokens_per_s": world * q / (ttft_ms * 1e-3)},
    }
    if args.full:
        if fused_gather:
            # pc_kv_gather itself (host tier, callers that look at `cache`, decode-only entries), on the same staging plan, eagerly
            # after the timed region
            segs = [(m.store.data_ptr(), len(m)) for m in pc.staged]
            offs, o = [], 0
            for _, ln in segs:
                offs.append(o); o += ln
            from promptcache_amd import _native as _n
            for i in range(12):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                _n.kv_gather([p_ for p_, _ in segs], [ln for _, ln in segs], offs, pc.arena.buf, pc.arena.L, pc.arena.Hkv, pc.arena.D, pc.arena.cap)
                e1.record()
                if i >= 2:
                    gather_evs.append((e0, e1))
            torch.cuda.synchronize()
        gather_us = sorted(a.elapsed_time(b) * 1e3 for a, b in gather_evs)
        gather_avg_us = sum(gather_us) / len(gather_us)
        achieved = alg_bytes / (gather_avg_us * 1e-6) / 1e9
        result["roofline_gather"] = {
            "kernel": "kv_copy_kernel (pc_kv_gather)", "bound": "hbm", "achieved": achieved, "peak": HBM_PEAK_GBS,
            "unit": "GB/s", "frac": achieved / HBM_PEAK_GBS,
            "traffic": _pmc_traffic("kv_copy_kernel", f"S={S},L={L},Hkv={Hkv},D={D}")[0],
            "traffic_source": _pmc_traffic("kv_copy_kernel", f"S={S},L={L},Hkv={Hkv},D={D}")[1],
            "algorithmic_bytes_per_launch": alg_bytes, "avg_launch_us": gather_avg_us,
            "min_launch_us": gather_us[0], "launches_timed": len(gather_us),
            "in_timed_step": not fused_gather,
            "how": ("HIP events around eager pc_kv_gather launches on the step's staging plan AFTER the timed region: the "
                    "timed steps stage inside their attention launches (pc_attn gather_rows) and launch no copy; "
                    "pc_kv_gather serves the host tier and callers that inspect the staged views") if fused_gather else
                   "HIP events recorded on the launch stream immediately around the launch, every timed step"}
        result["encode"] = encode
        result["encode_library"] = library
    # whole step against the HBM roof: every weight byte once + the gather (read + write) + the staged K/V once
    cfgm = lm.hf_model.config
    w_bytes = 2 * (cfgm.num_hidden_layers * (cfgm.hidden_size * (lm.hf_model.H + 2 * Hkv) * D + lm.hf_model.H * D * cfgm.hidden_size +
                                             3 * cfgm.hidden_size * cfgm.intermediate_size) + cfgm.vocab_size * cfgm.hidden_size)
    kvb = 2 * L * Hkv * D * 2
    step_bytes_r3 = w_bytes + alg_bytes + (S + q) * kvb          # rounds 1-3: gather read + write, then the attention reads the staged rows
    step_bytes = (w_bytes + alg_bytes + q * kvb) if fused_gather else step_bytes_r3
    step_gbs = step_bytes / (ttft_ms * 1e-3) / 1e9
    result["roofline_step"] = {"bound": "hbm", "achieved": step_gbs, "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": step_gbs / HBM_PEAK_GBS,
                               "algorithmic_bytes_per_step": step_bytes, "ms_per_step": ttft_ms,
                               "frac_by_round3_bytes": step_bytes_r3 / (ttft_ms * 1e-3) / 1e9 / HBM_PEAK_GBS,
                               "what": ("weights once + module K/V read once + staged K/V written once (the attention stages while it "
                                        "reads) + the new rows, divided by the driver-timed step; frac_by_round3_bytes prices the same "
                                        "time with round 3's byte count (gather read + write + staged K/V read: 0.9 GB more)")
                               if fused_gather else
                               "weights once + gather (read + write) + staged K/V once, divided by the driver-timed step"}
    result["staging"] = {"mode": "inside the first forward's attention launches (pc_attn gather_rows)" if fused_gather else "pc_kv_gather in CacheEngine.process",
                         "fused_gather_forwards": int(lm.hf_model.stats.get("fused_gather", 0)),
                         "host_glue_ms": ttft_ms - (process_ms[len(process_ms) // 2] + prefill_ms[len(prefill_ms) // 2]),
                         "what": "host_glue_ms = ms_per_step - (median process interval + median first-lm() interval)"}
    context = args.full and not args.no_context              # the legs outside the timed region (--full)
    # `roofline` = the time-dominant hand-written kernel of the timed step (largest share in profiles/r03_bench_kernel_stats.txt)
    if rank == 0 and context:
        result["roofline"], extra_rf = gemm_rooflines(lm, q)
        result.update(extra_rf)
        result["roofline_gemm"] = result["roofline"]          # (round 1-2 key of the gate|up figure)
    if result.get("roofline") is None and "roofline_gather" in result:
        result["roofline"] = dict(result["roofline_gather"], note="context legs off: the event-timed gather stands in; the "
                                                                   "dominant kernel needs the eager legs (drop --no-context)")
    if rank == 0 and context:
        # context (outside the timed region): the same prompt WITHOUT the prompt cache (cache_engine.py:476-493:
        # every token re-encoded, positions range(N)) and the hipGraph-captured decode rate after the prefill
        nids, npos, _, _ = eng.process(prompt, no_cache=True)
        nid_t = torch.tensor([list(nids)], device=device, dtype=torch.long)
        npos_t = torch.tensor([npos], device=device, dtype=torch.long)
        ts = []
        for _ in range(4):
            torch.cuda.synchronize(); t0 = time.perf_counter()
            lm(input_ids=nid_t, position_ids=npos_t, use_cache=True)
            torch.cuda.synchronize(); ts.append(time.perf_counter() - t0)
        result["no_cache"] = {"tokens": len(nids), "ttft_ms": min(ts[1:]) * 1e3,
                              "speedup_from_prompt_cache": min(ts[1:]) * 1e3 / ttft_ms}
        pc.reset()                                            # (a fresh staging, like every timed step: the staging variant is what is measured)
        ids2, pos2, _, cache2 = eng.process(prompt)
        result["roofline_attn"] = attn_roofline(lm, cache2, len(ids2))
        o2 = lm(input_ids=torch.tensor([ids2], device=device), position_ids=torch.tensor([pos2], device=device),
                past_key_values=cache2, use_cache=True)
        past, tok, nstep = o2.past_key_values, int(torch.argmax(o2.logits[0, -1])), 32
        for phase in range(2):
            torch.cuda.synchronize(); t0 = time.perf_counter()
            for i in range(nstep):
                o2 = lm(input_ids=torch.tensor([[tok]], device=device),
                        position_ids=torch.tensor([[max(pos2) + 2 + phase * nstep + i]], device=device),
                        past_key_values=past, use_cache=True)
                past, tok = o2.past_key_values, int(torch.argmax(o2.logits[0, -1]))
            torch.cuda.synchronize(); dt = time.perf_counter() - t0
        result["decode"] = {"tokens_per_s": nstep / dt, "ms_per_token": dt / nstep * 1e3, "kv_len": S + q + 2 * nstep,
                            "how": "greedy steps through lm(), hipGraph replay per step + host argmax (second block of 32 timed)"}
        # the same generation as GenerationEngine runs it: device-side greedy loop (argmax + token feed inside the graph)
        loop = lm.hf_model.greedy_loop(past, tok, max(pos2) + 2 + 2 * nstep, 4 * nstep)
        if loop is not None:
            for _ in range(nstep):
                loop.enqueue()
            loop.token(nstep - 1)                                  # warm: graph captured, code loaded
            torch.cuda.synchronize(); t0 = time.perf_counter()
            for _ in range(2 * nstep):
                loop.enqueue()
            last = loop.token(3 * nstep - 1)
            dtl = time.perf_counter() - t0
            # a decode step against the HBM roof: every weight byte once (lm_head included) + the K/V rows behind the token once
            cfd = lm.hf_model.config
            layer_w = cfd.num_hidden_layers * (cfd.hidden_size * (lm.hf_model.H + 2 * Hkv) * D + lm.hf_model.H * D * cfd.hidden_size +
                                               3 * cfd.hidden_size * cfd.intermediate_size)
            dec_bytes = 2 * layer_w + 2 * cfd.vocab_size * cfd.hidden_size + (S + q + 5 * nstep) * 2 * L * Hkv * D * 2
            result["decode_bytes"] = {"layer_weight_params": layer_w, "fp16_bytes_per_token": dec_bytes}
            result["decode_device_loop"] = {"tokens_per_s": 2 * nstep / dtl, "ms_per_token": dtl / (2 * nstep) * 1e3,
                                            "hbm_frac": dec_bytes / (dtl / (2 * nstep)) / 1e9 / HBM_PEAK_GBS,
                                            "kv_len": S + q + 5 * nstep, "last_token": last,
                                            "how": "GreedyLoop: one hipGraph replay per token (forward + pc_greedy_advance), no "
                                                   "host round trip; what GenerationEngine.generate uses for greedy decoding"}
            del loop
    if rank == 0 and context:
        # context: TTFT of a prompt whose new-token count has not been seen yet (an eager pass + hipGraph capture before
        # the first replay), then the same prompt again (replay): what a serving mix of question lengths pays once per length
        cold = []
        for extra in (3, 9):
            pp2 = prompt_pml.replace("</user>\n</prompt>", " " + synth.words(extra, 4242 + extra) + "</user>\n</prompt>")
            pr2 = Prompt(pp2, [fmt])
            ts2 = []
            for _ in range(3):
                pc.reset()
                torch.cuda.synchronize(); t0 = time.perf_counter()
                i2, p2, _, c2 = eng.process(pr2)
                lm(input_ids=torch.tensor([i2], device=device), position_ids=torch.tensor([p2], device=device),
                   past_key_values=c2, use_cache=True)
                torch.cuda.synchronize(); ts2.append((time.perf_counter() - t0) * 1e3)
            cold.append({"new_tokens": len(i2), "first_call_ms": ts2[0], "warm_ms": min(ts2[1:])})
        result["cold_shape_ttft"] = cold
    if rank == 0 and context:
        # context: the same step with this prompt's modules in the HOST tier (pinned host memory, the reference's default
        # placement, cache_engine.py:283-296) -- pc_kv_gather then reads them in place over PCIe.  Never `value`.
        used = list(pc.staged)
        for m in used:
            m.free()
        torch.cuda.synchronize()
        hs, hg = [], []
        for i in range(6):
            torch.cuda.synchronize(); t0 = time.perf_counter()
            step(False)
            torch.cuda.synchronize(); hs.append((time.perf_counter() - t0) * 1e3)
            a, b = pc.last_gather_events
            hg.append(a.elapsed_time(b))
        host_gather_ms = min(hg[1:])
        result["host_tier"] = {"ttft_ms": min(hs[1:]), "gather_ms": host_gather_ms,
                               "pcie_read_GBps": S * (2 * L * Hkv * D * 2) / (host_gather_ms * 1e-3) / 1e9,
                               "bytes_over_pcie": S * (2 * L * Hkv * D * 2),
                               "what": "module KV of the staged segments in pinned host memory (TokenSequenceCache.free()); "
                                       "same pc_kv_gather launch, sources read over PCIe; modules uploaded back afterwards"}
        for m in used:
            m.upload(device)
        torch.cuda.synchronize()
    if rank == 0 and context and not args.no_int8:
        # context: the reference's GPU configs load the model with load_in_8bit=True (config/llm_config_llama2_7b.json:5) =
        # LLM.int8() through bitsandbytes.  Here: the published algorithm (int8 weights, vector-wise
        # int8 activations, fp16 outlier columns at threshold 6.0), same prompt, same staged module KV (bit-identical
        # gather).  A different numeric mode: never `value`.
        def int8_leg(lm8):
            ids8, pos8, _, cache8 = eng.process(prompt)
            i8_t = torch.tensor([ids8], device=device, dtype=torch.long)
            p8_t = torch.tensor([pos8], device=device, dtype=torch.long)
            ts8 = []
            for _ in range(12):
                pc.reset()
                torch.cuda.synchronize(); t0 = time.perf_counter()
                _, _, _, cache8 = eng.process(prompt)
                o8 = lm8(input_ids=i8_t, position_ids=p8_t, past_key_values=cache8, use_cache=True)
                torch.cuda.synchronize(); ts8.append((time.perf_counter() - t0) * 1e3)
            past8, tok8 = o8.past_key_values, int(torch.argmax(o8.logits[0, -1]))
            # how many fp16 outlier columns the step's last layer split off (the flags of q|k|v's input were cleared by the
            # down_proj quantiser): the cost of the correction scales with them, and a random-init model has far more than an LLM
            fl8 = getattr(lm8.hf_model, "_i8_flags", None)
            outl = None if fl8 is None else {k: int(fl8[i].ne(0).sum()) for i, k in ((1, "o_proj_in"), (2, "gate_up_in"), (3, "down_proj_in"))}
            for phase in range(2):
                torch.cuda.synchronize(); t0 = time.perf_counter()
                for i in range(32):
                    o8 = lm8(input_ids=torch.tensor([[tok8]], device=device),
                             position_ids=torch.tensor([[max(pos8) + 2 + phase * 32 + i]], device=device),
                             past_key_values=past8, use_cache=True)
                    past8, tok8 = o8.past_key_values, int(torch.argmax(o8.logits[0, -1]))
                torch.cuda.synchronize(); dt8 = time.perf_counter() - t0
            # ... and the device-side greedy loop (what GenerationEngine.generate runs; the fp16 figure is `decode_device_loop`)
            loop8, loop8_rate = lm8.hf_model.greedy_loop(past8, tok8, max(pos8) + 2 + 64, 4 * 32), None
            if loop8 is not None:
                for _ in range(32):
                    loop8.enqueue()
                loop8.token(31)
                torch.cuda.synchronize(); t0 = time.perf_counter()
                for _ in range(64):
                    loop8.enqueue()
                loop8.token(95)
                loop8_rate = 64 / (time.perf_counter() - t0)
                del loop8
            # (int8 images: half the layer-weight bytes; lm_head and K/V stay fp16 -- the fraction is lower than fp16's although the
            # step is faster: what is left is per-launch fixed cost, not bytes)
            db = result.get("decode_bytes")
            i8_bytes = None if db is None else db["fp16_bytes_per_token"] - db["layer_weight_params"]

            return {"ttft_ms": sorted(ts8[2:])[len(ts8[2:]) // 2], "decode_tokens_per_s": 32 / dt8,
                    "decode_device_loop_tokens_per_s": loop8_rate,
                    "decode_device_loop_hbm_frac": None if (loop8_rate is None or i8_bytes is None) else
                    i8_bytes * loop8_rate / 1e9 / HBM_PEAK_GBS,
                    "mode": "llm_int8" if lm8.hf_model.llm_int8 else "weight_only",
                    "outlier_columns_last_layer": outl}

        lm8 = Llama2(args.model, device=device, random_init=True, seed=0, load_in_8bit=True)
        i8 = int8_leg(lm8)
        del lm8
        torch.cuda.empty_cache()
        # ... and with an outlier profile closer to a trained model's: N(0, 0.02) init leaves ~460 of down_proj's 11 008 input columns
        # above the LLM.int8 threshold (silu(g) * u with g, u ~ N(0, 1.3): the cost of the fp16 correction scales with them), a trained
        # Llama carries a handful of massive hidden channels instead.  Recipe: six channels of the embedding scaled 60 x (after RMSNorm
        # ~24 against ~0.4 for the rest, as tests/test_gpu_fullsize.py::test_full_depth_7b_with_outlier_feature_channels builds: six
        # flagged columns on every q|k|v / gate|up input) and the gate / up weights halved (g, u ~ N(0, 0.6): the MLP's intermediate
        # activations stay under the threshold but for the columns the massive channels drive).  Synthetic either way: no checkpoint here.
        from promptcache_amd.model.config import SHAPES as _SH
        from promptcache_amd.model.weights import random_weights_device as _rw
        _shape8 = _SH[args.model]
        _w8 = _rw(_shape8, device, torch.float16, 0)
        _w8["embed"][:, [7, 300, 1021, 2049, 3000, 4000]] *= 60.0
        for _k in list(_w8):
            if _k.endswith((".gate", ".up")):
                _w8[_k] *= 0.5
        lm8t = Llama2(name=args.model + "-outlier-channels", shape=_shape8, weights=_w8, device=device, load_in_8bit=True)
        del _w8
        i8t = int8_leg(lm8t)
        i8t["outlier_cols"] = (i8t["outlier_columns_last_layer"] or {}).get("down_proj_in")
        i8t["what"] = ("the same leg on a model with six 60 x hidden channels and halved gate / up weights (a trained-like outlier profile: "
                       "a handful of flagged columns per projection input instead of ~460 on down_proj's)")
        del lm8t
        torch.cuda.empty_cache()
        i8["trained_like"] = i8t
        i8.update({"what": "load_in_8bit=True: LLM.int8() as published (row-wise absmax int8 weights, vector-wise "
                                          "int8 activations, fp16 outlier columns at |x| >= 6), lm_head fp16; module KV from the "
                                          "fp16 engine; the activation quantisers run inside the projection launches (pc_gemm_q8: "
                                          "all four at <= 4 rows, down_proj's at 5..16 rows; PC_INT8_INLAUNCH=0: round 4's quantiser "
                                          "launches); decode_tokens_per_s steps through lm() with a host argmax, "
                                          "decode_device_loop_tokens_per_s is GreedyLoop (compare decode_device_loop); "
                                          "PC_INT8_WEIGHT_ONLY=1 selects round 1's weight-only mode"})
        result["int8_weights"] = i8
    if rank == 0 and world == 1 and args.full and not args.no_cpu_baseline:
        base, parity = cpu_baseline_and_parity(lm, eng, prompt, ids, pos, args.cpu_layers, parity_layers=args.parity_layers)
        result["cpu_baseline"] = base
        result["parity"] = parity
    if rank == 0 and world == 1 and context and not args.no_configs:
        eng.remove_all_schemas()
        torch.cuda.empty_cache()
        result["configs"] = configs_leg(device, world, rank, barrier, lm)
    if rank == 0:
        result["summary"] = compact_summary(result)     # LAST key: the tail of the line is what the driver's record keeps
        print(json.dumps(result))
    if dist.is_initialized():
        barrier()                      # the other ranks wait for rank 0's (untimed) context legs before tearing down
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
