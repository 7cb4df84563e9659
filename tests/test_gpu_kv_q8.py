"""The int8 module KV store on the GPU: ``pc_kv_quant_q8`` and ``pc_kv_gather_q8`` against the numpy restatement
(tests/kv_q8_ref.py) bit for bit, the engine in ``module_kv="int8"`` mode against the fp16 engine's stores, and the cached
prefill over the dequantised K/V against the numpy oracle run over the same dequantised K/V."""
import numpy as np
import pytest
import torch

from oracle import engine_oracle as eo
from tests import helpers as H
from tests import kv_q8_ref as R

pytestmark = pytest.mark.gpu
LOGIT_TOL = 1e-2        # the project's bar: max |delta logit|, as at the top of tests/test_gpu_engine.py

SENTINEL = 0x7BFF       # fp16 65504: never produced by the test data below (|x| stays far smaller)


def _mixed_rows(rng, P, n, D):
    """Random, outlier, all-zero and subnormal rows, interleaved."""
    x = (rng.standard_normal((P, n, D)) * rng.choice([1e-3, 0.3, 4.0, 60.0], size=(P, n, 1))).astype(np.float16)
    flat = x.reshape(-1, D)
    kind = rng.integers(0, 6, size=len(flat))
    out = flat[kind == 1]
    out[:, rng.integers(0, D)] = np.float16(900.0)                      # one outlier column
    flat[kind == 1] = out
    flat[kind == 2] = 0                                                 # all-zero rows
    sub = (rng.integers(-3, 4, size=(int((kind == 3).sum()), D)) * 2.0 ** -24).astype(np.float16)
    flat[kind == 3] = sub                                               # rows of fp16 subnormals (some of them all zero)
    one = np.zeros((int((kind == 4).sum()), D), np.float16)
    one[:, D // 3] = np.float16(2.0 ** -24)                             # exactly one subnormal
    flat[kind == 4] = one
    return flat.reshape(P, n, D)


def _image_tensor(img: np.ndarray, where: str) -> torch.Tensor:
    t = torch.from_numpy(img.copy())
    return t.cuda() if where == "device" else t.pin_memory()


@pytest.mark.parametrize("Hkv", [1, 8, 32])
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("n", [1, 7, 64, 1000])
def test_quant_kernel_equals_the_restatement_bit_for_bit(n, D, Hkv):
    from promptcache_amd import _native
    L = 2
    P = L * 2 * Hkv
    x = _mixed_rows(np.random.default_rng(n * 1000 + D + Hkv), P, n, D)
    src = torch.from_numpy(x).cuda()
    img = torch.full((_native.kv_q8_image_bytes(n, P, D) + 64,), 0xA5, dtype=torch.uint8, device="cuda")
    _native.kv_quant_q8(src, n, P, D, img)
    torch.cuda.synchronize()
    got = img.cpu().numpy()
    want = R.quantise_store(x)
    assert (got[want.size:] == 0xA5).all(), "the kernel wrote past the image"
    gc, gs = R.unpack(got[:want.size], P, n, D)
    wc, ws = R.unpack(want, P, n, D)
    assert np.array_equal(gc, wc), f"codes differ at {np.argwhere(gc != wc)[:5]}"
    assert np.array_equal(gs.view(np.uint32), ws.view(np.uint32)), "scale bits differ"


def test_quant_and_gather_keep_non_finite_rows_visible():
    from promptcache_amd import _native
    P, n, D = 4, 5, 128
    x = np.ones((P, n, D), np.float16)
    x[0, 1, 7], x[1, 2, 0], x[3, 4, 127] = np.nan, np.inf, -np.inf
    img = torch.empty(_native.kv_q8_image_bytes(n, P, D), dtype=torch.uint8, device="cuda")
    _native.kv_quant_q8(torch.from_numpy(x).cuda(), n, P, D, img)
    c, s = R.unpack(img.cpu().numpy(), P, n, D)
    bad = ~np.isfinite(x.astype(np.float32)).all(-1)
    assert bad.sum() == 3 and np.isnan(s[bad]).all() and not c[bad].any()
    assert np.array_equal(s[~bad].view(np.uint32), R.quantise(x)[1][~bad].view(np.uint32)) and np.array_equal(c, R.quantise(x)[0])
    out = torch.zeros((1, 2, 2, n, D), dtype=torch.float16, device="cuda")         # L = 1, Hkv = 2: the image's 4 planes
    _native.kv_gather_q8([img.data_ptr()], [n], [0], out, 1, 2, D, n)
    y = out.cpu().numpy().reshape(P, n, D).astype(np.float32)
    assert np.isnan(y[bad]).all() and np.isfinite(y[~bad]).all()


PERSONA_LENS = [1] * 17 + [3, 9, 40, 130, 257, 300, 64, 8]          # 25 segments, 17 of them one token (as the persona prompt)


def _gather_case(L, Hkv, D, lens, where, seed, gap_every=0):
    from promptcache_amd import _native
    rng = np.random.default_rng(seed)
    P = L * 2 * Hkv
    order = rng.permutation(len(lens))
    lens = [lens[i] for i in order]
    rows, r = [], 3                                                     # unaligned first row, segments back to back ...
    for k, n in enumerate(lens):
        rows.append(r)
        r += n + (5 if gap_every and k % gap_every == 0 else 0)         # ... with holes no segment covers
    cap = r + 7
    images = [R.quantise_store(_mixed_rows(rng, P, n, D)) for n in lens]
    place = [where if where != "mixed" else ("device", "host")[k % 2] for k in range(len(lens))]
    tensors = [_image_tensor(img, w) for img, w in zip(images, place)]
    arena = torch.full((L, 2, Hkv, cap, D), SENTINEL, dtype=torch.int16, device="cuda").view(torch.float16)
    before = arena.cpu().numpy()
    _native.kv_gather_q8([t.data_ptr() for t in tensors], lens, rows, arena, L, Hkv, D, cap)
    torch.cuda.synchronize()
    got = arena.cpu().numpy()
    want = R.gather(before, images, lens, rows)
    covered = np.zeros(cap, bool)
    for n, r0 in zip(lens, rows):
        covered[r0:r0 + n] = True
    assert (got[:, :, :, ~covered].view(np.uint16) == SENTINEL).all(), "rows outside every segment were written"
    assert np.array_equal(got.view(np.uint16), want.view(np.uint16)), \
        f"staged bytes differ at {np.argwhere(got.view(np.uint16) != want.view(np.uint16))[:5]}"


@pytest.mark.parametrize("where", ["device", "host", "mixed"])
@pytest.mark.parametrize("Hkv,D", [(8, 128), (1, 64), (32, 128), (8, 64)])
def test_gather_kernel_equals_the_restatement_bit_for_bit(Hkv, D, where):
    _gather_case(2, Hkv, D, PERSONA_LENS, where, seed=Hkv * 10 + D, gap_every=4)


def test_gather_more_segments_than_one_launch_holds_and_a_long_segment():
    _gather_case(1, 2, 128, [1, 2, 3] * 15, "mixed", seed=1)                   # 45 segments: two launches
    _gather_case(1, 1, 128, [1000, 1, 513], "device", seed=2, gap_every=1)     # several row tiles per segment
    _gather_case(3, 1, 64, [1025, 7], "host", seed=3)


def test_gather_rejects_what_does_not_fit():
    from promptcache_amd import _native
    img = torch.zeros(R.image_bytes(4, 8, 128), dtype=torch.uint8, device="cuda")
    arena = torch.zeros((1, 2, 2, 16, 128), dtype=torch.float16, device="cuda")
    with pytest.raises(RuntimeError, match="exceeds max_ctx"):
        _native.kv_gather_q8([img.data_ptr()], [8], [9], arena, 1, 2, 128, 16)
    assert not arena.any()


# ---- engine level -------------------------------------------------------------------------------------------------------------

def build_product(g, **engine_kw):
    """The recipe of tests/test_gpu_engine.py ``build_product``, with the engine's keyword arguments open."""
    from promptcache_amd import CacheEngine
    from promptcache_amd.model import Falcon, Llama2, Mpt
    from promptcache_amd.model.weights import make_falcon_weights_np, make_mpt_weights_np, make_weights_np
    shape = H.shape_for_case(g)
    if H.is_mpt(g):
        lm = Mpt(name="golden", shape=shape, weights=make_mpt_weights_np(shape, int(g["seed"]), float(g["scale"])),
                 device="cuda:0")
    elif H.is_falcon(g):
        lm = Falcon(name="golden", shape=shape, weights=make_falcon_weights_np(shape, int(g["seed"]), float(g["scale"])),
                    device="cuda:0")
    else:
        lm = Llama2(name="golden", shape=shape, weights=make_weights_np(shape, int(g["seed"]), float(g["scale"])),
                    device="cuda:0")
    return lm, add_engine(g, lm, **engine_kw)


def add_engine(g, lm, **engine_kw):
    from promptcache_amd import CacheEngine
    eng = CacheEngine(int(g["max_ctx"]), lm, **engine_kw)
    mt = int(g["max_tokens"])
    eng.add_schema(lm.get_formatter()(str(g["schema_text"])), max_tokens=None if mt < 0 else mt)
    return eng


def _segments(eng):
    return list(eng.schemas[list(eng.schemas)[0]].cache_l1.values())


def _image_np(c):
    return c.store.cpu().numpy()


def _key(c):
    return c.token_sequence.offset, tuple(c.token_sequence.token_ids())


def _expected_arena(eng, images=None):
    """dequant of the staged segments' images (``images``: {_key: image} recorded earlier; default: the live stores), scattered in
    staging order (numpy)."""
    a = eng.prompt_cache.arena
    staged = eng.prompt_cache.staged
    lens = [len(m) for m in staged]
    rows = list(np.cumsum([0] + lens[:-1]))
    imgs = [_image_np(m) if images is None else images[_key(m)] for m in staged]
    return R.gather(np.zeros((a.L, 2, a.Hkv, a.cap, a.D), np.float16), imgs, lens, rows), sum(lens)


@pytest.mark.parametrize("case", ["tiny_trip", "mid_mha_doc", "tiny_personalike", "falcon_tiny_trip", "falcon_mid_doc"])
def test_int8_engine_images_staging_tiers_and_retention(case):
    """Llama (D = 128 ... whatever the case's shape has) and Falcon (D = 64, MQA) through the same bit checks."""
    from promptcache_amd import Prompt
    g = H.load_case(case)
    lm, ref = build_product(g)                                          # fp16 stores
    eng = add_engine(g, lm, module_kv="int8")
    L, Hkv, D = lm.get_cache_shape()
    fsegs, qsegs = _segments(ref), _segments(eng)
    images0 = {_key(q): _image_np(q) for q in qsegs}                   # as born in HBM
    assert len(fsegs) == len(qsegs) > 0
    for f, q in zip(fsegs, qsegs):                                      # same plan order on both engines
        assert _key(f) == _key(q)
        assert f.format == "fp16" and q.format == "int8" and q.q8_shape == (L, Hkv, D)
        assert q.store.dtype == torch.uint8 and q.store.is_cuda and q.store.numel() == R.image_bytes(L * 2 * Hkv, len(q), D)
        want = R.quantise_store(f.store.cpu().numpy())
        assert np.array_equal(_image_np(q), want), "int8 store != quantise(fp16 store)"
        # the per-layer views keep the reference's shapes, as dequantised copies
        kv = q.cache
        assert len(kv) == L and kv[0][0].shape == (Hkv, len(q), D) and kv[0][0].dtype == torch.float16
        deq = R.dequant_image(want, L, Hkv, len(q), D)
        assert np.array_equal(torch.stack([torch.stack(p) for p in kv]).cpu().numpy().view(np.uint16), deq.view(np.uint16))
        assert q.host_cache is None and q.device_cache is not None
    # store bytes: exactly (D + 4) / 2D of the fp16 engine's
    name = list(eng.schemas)[0]
    assert eng.module_bytes(name) * 2 * D == ref.module_bytes(name) * (D + 4) and eng.module_bytes() == {name: eng.module_bytes(name)}

    fmt = lm.get_formatter()
    full = lm.use_full_position_ids
    i0, p0, _, _ = ref.process(Prompt(str(g["prompt_text"]), [fmt]), return_full_position_ids=full)
    pc = eng.prompt_cache
    pc.record_events = True
    ids, pos, ms, cache = eng.process(Prompt(str(g["prompt_text"]), [fmt]), return_full_position_ids=full)
    assert ids == i0 and pos == p0 and ms >= 0.0
    assert pc.arena.pending is None, "int8 segments must take the explicit gather"
    assert [(m.token_sequence.offset, len(m)) for m in pc.staged] == [(m.token_sequence.offset, len(m)) for m in ref.prompt_cache.staged]
    want, S = _expected_arena(eng)
    assert S == len(pc) == cache[0][0].shape[1] and pc.last_gather_tokens == S and pc.last_gather_events is not None
    staged_dev = pc.arena.buf[0, :, :, :, :S].cpu().numpy()
    assert np.array_equal(staged_dev.view(np.uint16), want[:, :, :, :S].view(np.uint16)), "staged arena != dequant(images)"

    # retention: the same prompt again keeps every segment -- nothing is gathered, rows poisoned in between stay poisoned
    pc.arena.buf[0, :, :, :, :S] = float("nan")
    eng.process(Prompt(str(g["prompt_text"]), [fmt]), return_full_position_ids=full)
    assert pc.last_gather_tokens == 0 and torch.isnan(pc.arena.buf[0, :, :, :, :S]).all()
    # ... and a prompt with another module set keeps exactly the leading segments it shares with what is staged
    other = {"tiny_trip": "tiny_trip2"}.get(case)
    if other is not None:
        prev = list(pc.staged)
        eng.process(Prompt(str(H.load_case(other)["prompt_text"]), [fmt]))
        keep = 0
        for m, p in zip(pc.staged, prev):
            if m is not p:
                break
            keep += 1
        kept_rows = sum(len(m) for m in pc.staged[:keep])
        assert pc.last_gather_tokens == len(pc) - kept_rows
        got = pc.arena.buf[0, :, :, :, :len(pc)]
        assert torch.isnan(got[:, :, :, :kept_rows]).all()
        want2, S2 = _expected_arena(eng)
        assert np.array_equal(got[:, :, :, kept_rows:].cpu().numpy().view(np.uint16), want2[:, :, :, kept_rows:S2].view(np.uint16))
        print(f"[{case}] second prompt kept {keep} leading segments ({kept_rows} rows), gathered {pc.last_gather_tokens}")

    # host tier: offload, stage again from pinned memory (all of it, then mixed with HBM) -- the bytes the HBM-born images give
    # (the usage counters have moved on, so the staging ORDER may differ from the first prompt's: the expectation follows it)
    def restage():
        pc.reset()
        i2, _, _, _ = eng.process(Prompt(str(g["prompt_text"]), [fmt]), return_full_position_ids=full)
        assert i2 == ids and len(pc) == S and pc.last_gather_tokens == S
        w, _ = _expected_arena(eng, images0)
        assert np.array_equal(pc.arena.buf[0, :, :, :, :S].cpu().numpy().view(np.uint16), w[:, :, :, :S].view(np.uint16))

    restage()                                                           # from HBM

    for q in qsegs:
        q.offload()
    assert all(q.device_store is None and q.host_store.is_pinned() and q.host_store.dtype == torch.uint8 for q in qsegs)
    assert all(q.device_cache is None and q.host_cache is not None and not q.host_cache[0][0].is_cuda for q in qsegs)
    restage()
    for q in qsegs[::2]:
        q.upload(lm.device)
    torch.cuda.synchronize()
    restage()
    for q in qsegs:
        q.free()
    restage()
    # an engine born in the host tier holds the same images
    host = add_engine(g, lm, module_kv="int8", module_memory="host")
    for q, h in zip(qsegs, _segments(host)):
        assert h.device_store is None and h.host_store.is_pinned() and torch.equal(h.host_store, q.host_store)
    # a staging takes one format
    mixed = add_engine(g, lm)
    mixed.process(Prompt(str(g["prompt_text"]), [fmt]), return_full_position_ids=full)
    assert len(mixed.prompt_cache.staged) > 1
    mixed.prompt_cache.staged[0].quantize_()
    assert mixed.prompt_cache.staged[0].format == "int8"
    mixed.prompt_cache.reset()
    with pytest.raises(ValueError, match="mix fp16 and int8"):
        mixed.process(Prompt(str(g["prompt_text"]), [fmt]), return_full_position_ids=full)
    # remove_schema / add again / no_cache work as in fp16 mode
    eng.remove_schema(name)
    assert eng.module_bytes() == {}
    mt = int(g["max_tokens"])
    eng.add_schema(fmt(str(g["schema_text"])), max_tokens=None if mt < 0 else mt)
    nids, npos, _, none = eng.process(Prompt(str(g["prompt_text"]), [fmt]), no_cache=True)
    assert none is None and list(nids) == g["nocache_ids"].tolist() and npos == g["nocache_pos"].tolist()
    restage()


@pytest.mark.parametrize("case", ["tiny_trip", "mid_mha_doc", "tiny_personalike", "falcon_mid_doc", "mpt_tiny_trip"])
def test_int8_mode_logits_match_the_oracle_over_the_dequantised_kv(case):
    """Same staged values on both sides (the oracle's module library IS the dequantised images), so the bar is the project's
    own LOGIT_TOL; then greedy generation through GenerationEngine's device loop."""
    from promptcache_amd import GenerationEngine, GenerationParameters, Prompt
    g = H.load_case(case)
    lm, eng = build_product(g, module_kv="int8")
    L, Hkv, D = lm.get_cache_shape()
    fmt = lm.get_formatter()
    full = lm.use_full_position_ids
    ids, pos, _, cache = eng.process(Prompt(str(g["prompt_text"]), [fmt]), return_full_position_ids=full)
    out = lm(input_ids=torch.tensor([ids], device="cuda"), position_ids=torch.tensor([pos], device="cuda"),
             past_key_values=cache, use_cache=True)
    model, _ = H.oracle_for_case(g, H.shape_for_case(g))
    used = [m.token_sequence for m in eng.prompt_cache.staged]
    lib = {}
    for m in eng.prompt_cache.staged:
        deq = R.dequant_image(_image_np(m), L, Hkv, len(m), D).astype(np.float32)
        lib[id(m.token_sequence)] = [(deq[i, 0], deq[i, 1]) for i in range(L)]
    with H.oracle_blas():
        _, S, (logits, present) = eo.cached_prefill(model, lib, used, ids, pos, int(g["max_ctx"]))
    err = float(np.abs(out.logits[0].cpu().numpy() - logits[0]).max())
    print(f"[int8 module KV, {case}] S={S} q={len(ids)} max|dlogit| vs oracle over the dequantised K/V = {err:.2e}")
    assert err < LOGIT_TOL
    n_new = 12
    assert GenerationEngine.device_greedy_loop
    ids, pos, _, cache = eng.process(Prompt(str(g["prompt_text"]), [fmt]), return_full_position_ids=full)
    params = GenerationParameters(temperature=0.0, max_new_tokens=n_new, stop_token_ids=[], stop_str=[])
    outs = list(GenerationEngine(lm).generate(ids, pos, params, cache, stream_interval=1, use_full_position_ids=full))
    assert len(outs) == n_new and outs[-1].elapsed_time > 0
    with H.oracle_blas():
        toks = eo.generate_greedy(model, logits, present, pos, n_new, use_full_position_ids=full)
    agree = outs[-1].new_text == lm.decode(toks)
    print(f"[int8 module KV, {case}] {n_new} greedy tokens {'equal' if agree else 'differ from'} the oracle's")


def test_int8_mode_with_int8_weights_and_a_library():
    """``load_in_8bit`` models and ``add_schemas`` only ever see the staged fp16 arena: both run in int8 mode."""
    from promptcache_amd import CacheEngine, Prompt, synth
    from promptcache_amd.model import Llama2
    from promptcache_amd.model.config import SHAPES
    from promptcache_amd.model.weights import make_weights_np
    shape = SHAPES["mid64_gqa"]
    lm = Llama2(name="x", shape=shape, weights=make_weights_np(shape, 4, 1.0), device="cuda:0", load_in_8bit=True)
    fmt = lm.get_formatter()
    texts = [synth.flat_docs(f"lib{k}", 6, (30, 21), 9, seed=k) for k in range(3)]
    engines = {}
    for kv in ("fp16", "int8"):
        eng = CacheEngine(256, lm, module_kv=kv)
        eng.add_schemas([fmt(sp) for sp, _ in texts])
        engines[kv] = eng
    D = lm.get_cache_shape()[2]
    for nm, b in engines["int8"].module_bytes().items():
        assert b * 2 * D == engines["fp16"].module_bytes(nm) * (D + 4)
    for _, pp in texts:
        outs = {}
        for kv, eng in engines.items():
            ids, pos, _, cache = eng.process(Prompt(pp, [fmt]))
            outs[kv] = lm(input_ids=torch.tensor([ids], device="cuda"), position_ids=torch.tensor([pos], device="cuda"),
                          past_key_values=cache, use_cache=True).logits.clone()
        assert torch.isfinite(outs["int8"]).all() and outs["int8"].shape == outs["fp16"].shape
        print(f"int8 weights: max|logit_int8kv - logit_fp16kv| = {(outs['int8'] - outs['fp16']).abs().max().item():.2e}")
