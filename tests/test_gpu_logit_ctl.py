"""pc_logit_adjust against the numpy rule (tests/logit_ctl_ref.py) on the GPU: bitwise after viewing as uint32, NaN positions
compared as positions.  Every case is one or two launches on at most 64 rows."""
import ctypes

import numpy as np
import pytest
import torch

from tests import logit_ctl_ref as ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENT = 77.0


def _native():
    from promptcache_amd import _native
    _native.load()
    return _native


def _block(n, blk: dict) -> bytes:
    """The device block of ``blk`` exactly as given: ``n_bias`` may exceed the table, ids may lie outside the vocabulary."""
    b = n.LogitCtl()
    bias = list(blk.get("bias", ()))
    b.n_bias = int(blk.get("n_bias", len(bias)))
    b.use_allowed = 1 if blk.get("allowed") is not None else 0
    b.stop_free_len = int(blk.get("stop_free_len", 0))
    stops = list(blk.get("stop_ids", ()))
    for j in range(8):
        b.stop_ids[j] = stops[j] if j < len(stops) else -1
    for j, (i, v) in enumerate(bias):
        b.bias_id[j], b.bias[j] = int(i), float(v)
    return bytes(b)


def _rows(R, V, seed):
    g = np.random.default_rng(seed)
    return (g.standard_normal((R, V)) * 3).astype(np.float32)


def _run(x, rps, blocks, lens=None, ldl=None, off=0, ldo=None, bits_always=False):
    """One launch over rows ``x`` ([S * rps][V]) -> (adjusted [R][V], the whole ``out`` buffer [R][ldo])."""
    n = _native()
    R, V = x.shape
    S = R // rps
    assert S * rps == R and len(blocks) == S
    ldl = V if ldl is None else ldl
    ldo = (V + 3) & ~3 if ldo is None else ldo
    host = np.full(off + (R - 1) * ldl + V + 8, SENT, dtype=np.float32)
    for r in range(R):
        host[off + r * ldl: off + r * ldl + V] = x[r]
    buf = torch.from_numpy(host).to(DEV)
    logits = buf[off:]
    assert (logits.data_ptr() % 16 == 0) == (off % 4 == 0)
    ctl = torch.frombuffer(bytearray(b"".join(_block(n, b) for b in blocks)), dtype=torch.uint8).to(DEV)
    allowed = None
    if bits_always or any(b.get("allowed") is not None for b in blocks):
        words = np.stack([ref.allowed_bits(b.get("allowed") or (), V) for b in blocks])
        allowed = torch.from_numpy(words.view(np.int32)).to(DEV)
    length = None if lens is None else torch.tensor(list(lens), dtype=torch.int32, device=DEV)
    out = torch.full((R, ldo), SENT, dtype=torch.float32, device=DEV)
    n.logit_adjust(logits, ldl, V, S, rps, ctl, allowed, length, out, ldo)
    torch.cuda.synchronize()
    assert torch.equal(buf.cpu().view(torch.int32), torch.from_numpy(host).view(torch.int32))     # the raw rows are left alone
    got = out.cpu().numpy()
    assert np.all(got[:, V:] == SENT)                                        # columns [V, ldo) are not written
    return got[:, :V].copy()


def _check(x, rps, blocks, lens=None, **kw):
    got = _run(x, rps, blocks, lens, **kw)
    want = ref.adjust_slots(x, rps, blocks, lens)
    assert ref.same_bits(got, want), np.argwhere(got.view(np.uint32) != want.view(np.uint32))[:8]
    return got


def _full_block(V, seed):
    """64 entries: ids 0 and V - 1, four ids adjacent in one 16-byte group, a ban, the rest spread; a stop id equal to a biased id."""
    g = np.random.default_rng(seed)
    ids = [0, V - 1] + [i for i in (4, 5, 6, 7) if i < V - 1]
    pool = [i for i in g.permutation(V).tolist() if i not in ids]
    ids = (ids + pool)[:min(64, V)]
    bias = [(i, float(v)) for i, v in zip(ids, g.standard_normal(len(ids)) * 5)]
    bias[1] = (bias[1][0], -np.inf)
    return dict(bias=bias, stop_ids=[ids[0], ids[-1], min(9, V - 1)], stop_free_len=10 ** 6)


# rows 1, 16 and 64 with 1, 4 and 16 rows per slot at every vocabulary; 64 slots of one row where the indexing is cheap to check
SHAPES = [(V, R, rps) for V in (9, 33, 65, 32000, 128256) for R, rps in ((1, 1), (16, 4), (64, 16))] + [(9, 64, 1), (65, 64, 1)]


@pytest.mark.parametrize("V,R,rps", SHAPES)
def test_vocabularies_and_row_counts(V, R, rps):
    S = R // rps
    x = _rows(R, V, V + R)
    g = np.random.default_rng(R)
    blocks = []
    for b in range(S):
        blk = _full_block(V, 100 + b)
        if b % 2 == 0:
            blk["allowed"] = sorted(set(g.integers(0, V, size=max(3, V // 3)).tolist() + [0, V - 1, blk["bias"][2][0]]))
        blk["stop_free_len"] = 50 + (b % 3)              # lens below: the boundary falls inside some slots' rows
        blocks.append(blk)
    lens = [48 + (b % 4) for b in range(S)]
    _check(x, rps, blocks, lens)


@pytest.mark.parametrize("V", [33, 32000])
def test_layouts_odd_stride_unaligned_base_wide_out(V):
    x = _rows(8, V, 5)
    blocks = [_full_block(V, 7), dict(_full_block(V, 8), allowed=list(range(0, V, 3)))]
    lens = [3, 4]
    want = _check(x, 4, blocks, lens)
    for kw in (dict(ldl=V + 1), dict(ldl=V + 3, off=1), dict(off=3), dict(ldo=((V + 3) & ~3) + 8), dict(ldl=V + 5, off=2, ldo=V + 12 - V % 4)):
        assert ref.same_bits(_check(x, 4, blocks, lens, **kw), want), kw


def test_bias_table_sizes_and_skipped_ids():
    V = 32000
    x = _rows(2, V, 11)
    x[0, 17] = -np.inf
    x[0, 18] = np.nan
    x[1, 0] = np.nan
    x[1, V - 1] = -np.inf
    one = dict(bias=[(17, 2.5)])
    none = dict(bias=[(5, 1.0)], n_bias=0)
    got = _check(x, 1, [none, one])
    assert ref.same_bits(got[0], x[0]) and got[1, 17] == x[1, 17] + np.float32(2.5)
    # -inf and NaN inputs: x + bias keeps them; a -inf bias bans; ids outside the vocabulary are skipped
    blk = dict(bias=[(17, 1.0), (18, 1.0), (19, -np.inf), (V, 3.0), (-1, 3.0), (2 ** 24, 3.0), (0, 0.5), (V - 1, 0.5)])
    got = _check(x, 1, [blk, blk])
    assert got[0, 17] == -np.inf and np.isnan(got[0, 18]) and got[0, 19] == -np.inf and np.isnan(got[1, 0]) and got[1, V - 1] == -np.inf
    # n_bias = 1000 in the block: clamped to the 64 entries of the table
    full = _full_block(V, 3)
    assert len(full["bias"]) == 64
    got = _check(x, 1, [dict(full, n_bias=1000), dict(full, n_bias=-5)])
    assert ref.same_bits(got[1], ref.adjust(x[1], (), None, full["stop_ids"], True))
    # negative n_bias: no entry applied, the stop ids still held back


def test_allow_lists():
    V = 65
    x = _rows(3, V, 13)
    x[0, 40] = np.nan
    got = _check(x, 1, [dict(allowed=[64]), dict(allowed=list(range(V))), dict(allowed=[1, 32, 63], bias=[(2, 9.0), (32, -1.0)])])
    assert np.isfinite(got[0]).sum() == 1 and got[0, 64] == x[0, 64] and got[0, 40] == -np.inf          # a disallowed NaN is -inf
    assert ref.same_bits(got[1], x[1])
    assert got[2, 2] == -np.inf and got[2, 32] == x[2, 32] + np.float32(-1.0) and np.isfinite(got[2]).sum() == 3
    # use_allowed = 0 with a bitmap present (all zero): everything stays allowed; a null bitmap with use_allowed set: too
    assert ref.same_bits(_run(x, 1, [dict(), dict(), dict()], bits_always=True), x)
    n = _native()
    ctl = torch.frombuffer(bytearray(_block(n, dict(allowed=[1]))), dtype=torch.uint8).to(DEV)
    out = torch.empty((1, 68), dtype=torch.float32, device=DEV)
    n.logit_adjust(torch.from_numpy(x[:1].copy()).to(DEV), V, V, 1, 1, ctl, None, None, out, 68)
    assert ref.same_bits(out.cpu().numpy()[:, :V], x[:1])


def test_stop_boundary_inside_a_step_and_between_slots():
    V, rps = 32000, 4
    x = _rows(3 * rps, V, 17)
    stop = [5, 31999, 700]
    blk = dict(stop_ids=stop, bias=[(700, 4.0)])             # (a stop id equal to a biased id)
    # slot 0: len 10, free at 12 -> rows 0 and 1 held, 2 and 3 free (between i = 1 and i = 2); slot 1: held on no row (never);
    # slot 2: held on every row
    blocks = [dict(blk, stop_free_len=12), dict(blk, stop_free_len=0), dict(blk, stop_free_len=10 ** 9)]
    got = _check(x, rps, blocks, [10, 10, 10])
    held = np.array([[got[b * rps + i, 5] == -np.inf and got[b * rps + i, 700] == -np.inf and got[b * rps + i, 31999] == -np.inf
                      for i in range(rps)] for b in range(3)])
    assert held.tolist() == [[True, True, False, False], [False] * 4, [True] * 4]
    assert got[2, 700] == x[2, 700] + np.float32(4.0)
    # the boundary at rows (b, 0) of two different slots: slot 0 still held at its row 0, slot 1 free from its row 0 on
    blocks = [dict(blk, stop_free_len=11), dict(blk, stop_free_len=11), dict(blk, stop_free_len=11)]
    got = _check(x, rps, blocks, [10, 11, 12])
    assert [got[b * rps, 5] == -np.inf for b in range(3)] == [True, False, False] and got[1, 5] == x[1, 5]
    # len null reads as 0
    got = _check(x, rps, [dict(blk, stop_free_len=2)] * 3, None)
    assert [got[i, 5] == -np.inf for i in range(rps)] == [True, True, False, False]


def test_a_slot_depends_on_its_own_block_alone():
    V, rps = 32000, 4
    x = _rows(2 * rps, V, 19)
    a = dict(_full_block(V, 1), allowed=list(range(100, 9000)), stop_free_len=7)
    b = dict(bias=[(3, -np.inf)], stop_ids=[4], stop_free_len=100)
    both = _check(x, rps, [a, b], [5, 98])
    assert ref.same_bits(both[:rps], _check(x[:rps], rps, [a], [5]))
    assert ref.same_bits(both[rps:], _check(x[rps:], rps, [b], [98]))
    swapped = _check(np.concatenate([x[rps:], x[:rps]]), rps, [b, a], [98, 5])        # ... and not on the slot index
    assert ref.same_bits(swapped[:rps], both[rps:]) and ref.same_bits(swapped[rps:], both[:rps])


def test_argument_errors():
    n = _native()
    lib = n.load()
    V = 64
    x = torch.zeros((2, V), dtype=torch.float32, device=DEV)
    out = torch.zeros((2, V), dtype=torch.float32, device=DEV)
    ctl = torch.zeros(2 * ctypes.sizeof(n.LogitCtl), dtype=torch.uint8, device=DEV)
    ok = [x.data_ptr(), V, V, 2, 1, ctl.data_ptr(), None, None, out.data_ptr(), V, None]
    for i, bad in ((0, None), (5, None), (8, None), (3, 0), (3, 65), (4, 17), (4, 0), (2, 0), (2, 1 << 24), (1, V - 1), (9, V - 4), (9, V + 2),
                   (8, out.data_ptr() + 4), (0, x.data_ptr() + 2), (8, x.data_ptr())):
        args = list(ok)
        args[i] = bad
        assert lib.pc_logit_adjust(*args) == -1001, (i, bad)
        assert b"pc_logit_adjust" in lib.pc_last_error_string()
    assert lib.pc_logit_adjust(*ok) == 0
