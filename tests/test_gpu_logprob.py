"""pc_token_logprobs (csrc/pc_logprob.hip) on the GPU, through ctypes, against the float64 reference of tests/logprob_ref.py.

Token ids and alternative ids are EXACT: they come from comparisons, no arithmetic.  Log-probabilities are within 2e-4 absolute
of float64 for |logit| <= 64 and V <= 131 072.  Derivation, in fp32: the sum of V terms runs over >= 256 lanes, a relative error
of at most about (V / 256 + 11) * 2^-24 = 3e-5 at V = 128 256; the exponent argument's rounding and v_exp_f32 add at most about
1.5e-5; the three roundings of the final subtractions at magnitude <= 128 add at most about 2.3e-5.  Worst case about 7e-5: the
tolerance leaves under 3x over it.  A dropped element must not hide under it: a +20 spike over zeros moves every other
entry by log(e^20 + V - 1) - log(V - 1) when lost (more than 10 up to V = 22 026, 8.2 at V = 128 256) and changes the first id, the range row loses its whole maximum, and the ids of the tie rows are exact."""
import ctypes

import numpy as np
import pytest
import torch

from tests import logprob_ref as ref

pytestmark = pytest.mark.gpu
TOL = ref.TOL


def _launch(rows, tokens, top_n, ldl=None, offset=0, tok="i64", stride=1):
    """rows [R][V] fp32 -> (ids [R][1 + top_n], lp [R][1 + top_n]) from one launch; the logits base sits ``offset`` floats past an
    aligned allocation, rows ``ldl`` floats apart; row r's token at ``tokens_dev[r * stride]``."""
    from promptcache_amd import _native
    rows = np.asarray(rows, dtype=np.float32)
    R, V = rows.shape
    ldl = V if ldl is None else ldl
    buf = torch.full((offset + R * ldl + 8,), 99.0, dtype=torch.float32, device="cuda")    # (the gaps hold a value that would win)
    view = buf[offset:offset + R * ldl].view(R, ldl)
    view[:, :V].copy_(torch.from_numpy(rows))
    dt = torch.int64 if tok == "i64" else torch.int32
    tk = torch.full((R * stride,), 7, dtype=dt, device="cuda")
    tk[::stride] = torch.tensor([int(t) for t in tokens], dtype=dt, device="cuda")
    ids = torch.full((R, 1 + top_n), -7, dtype=torch.int32, device="cuda")
    lp = torch.full((R, 1 + top_n), 123.0, dtype=torch.float32, device="cuda")
    _native.token_logprobs(view, ldl, V, R, tk, stride, top_n, ids, lp)
    torch.cuda.synchronize()
    return ids.cpu().numpy(), lp.cpu().numpy()


def _check(rows, tokens, top_n, ids, lp, what=""):
    want_ids, want_lp = ref.records(rows, tokens, top_n)
    assert np.array_equal(ids, want_ids), (what, np.argwhere(ids != want_ids)[:5], ids[ids != want_ids][:5], want_ids[ids != want_ids][:5])
    nan = np.isnan(want_lp)
    assert np.array_equal(np.isnan(lp), nan), (what, "NaN pattern")
    inf = np.isneginf(want_lp)
    assert np.array_equal(np.isneginf(lp), inf), (what, "-inf pattern")
    fin = ~(nan | inf)
    err = np.abs(lp[fin].astype(np.float64) - want_lp[fin])
    worst = float(err.max()) if err.size else 0.0
    print(f"[logprob] {what}: max |lp - float64| = {worst:.3e} over {int(fin.sum())} entries")
    assert worst <= TOL, (what, worst)


@pytest.mark.parametrize("V,top_n,ldl_extra,offset", [(9, 8, 0, 0), (33, 8, 0, 0), (33, 0, 0, 0), (33, 1, 0, 0), (33, 2, 0, 0),
                                                     (33, 3, 0, 0), (1000, 8, 0, 0), (1000, 5, 0, 0), (1027, 8, 2, 1),
                                                     (32000, 8, 0, 0)])
def test_every_row_kind_and_every_chosen_token_case(V, top_n, ldl_extra, offset):
    """All row kinds of ``case_rows`` in one launch per chosen-token case: the top-1, a token outside the top-n, index V - 1, and
    two tokens out of range (NaN and id -1 in entry 0, the alternatives still right).  V = 1 027: odd ldl, base 4 bytes past a
    16-byte boundary, so rows alternate between the aligned 16-byte loads and the scalar path."""
    cases = ref.case_rows(V)
    names, rows = list(cases), np.stack(list(cases.values()))
    assert len(rows) <= 64
    assert (V + ldl_extra) % 2 == 1 or ldl_extra == 0
    for c in range(5):
        tokens = [ref.case_tokens(x, top_n)[c] for x in rows]
        ids, lp = _launch(rows, tokens, top_n, ldl=V + ldl_extra, offset=offset, tok="i64" if c % 2 == 0 else "i32")
        _check(rows, tokens, top_n, ids, lp, f"V={V} n={top_n} case {c}")
    assert "nothing_finite" in names and np.all(ids[names.index("nothing_finite")] == -1)


def test_largest_vocabulary_once():
    V = 128256
    cases = ref.case_rows(V)
    keep = ["normal", "normal_wide", f"spike@{V - 1}", f"spike@{V - 9}", "spike@0", "quarters", "range", "constant", "nan"]
    rows = np.stack([cases[k] for k in keep])
    tokens = [ref.case_tokens(x, 8)[i % 3] for i, x in enumerate(rows)]
    ids, lp = _launch(rows, tokens, 8)
    _check(rows, tokens, 8, ids, lp, "V=128256")


@pytest.mark.parametrize("R", [1, 16, 64])
def test_row_counts_token_strides_and_widths(R):
    """rows 1, 16 and 64; tok64 with a stride of k + 1 = 4 (the lookup loops' ids array) and tok32 (their row scratch)."""
    V, rng = 1000, np.random.default_rng(R)
    rows = np.clip(rng.standard_normal((R, V)) * 4.0, -64, 64).astype(np.float32)
    rows[R // 2] = np.round(rows[R // 2] * 4) / 4
    tokens = rng.integers(0, V, R)
    for tok, stride in (("i64", 4), ("i64", 1), ("i32", 1), ("i32", 3)):
        ids, lp = _launch(rows, tokens, 8, tok=tok, stride=stride)
        _check(rows, tokens, 8, ids, lp, f"R={R} {tok} stride {stride}")


def test_a_row_depends_on_that_row_alone():
    V, R, rng = 1027, 16, np.random.default_rng(5)
    rows = np.clip(rng.standard_normal((R, V)) * 4.0, -64, 64).astype(np.float32)
    tokens = rng.integers(0, V, R)
    ids0, lp0 = _launch(rows, tokens, 8, ldl=V + 2, offset=1)
    other = rows.copy()
    other[np.arange(R) != 5] = np.clip(rng.standard_normal((R - 1, V)) * 9.0, -64, 64).astype(np.float32)
    other[0] = np.nan
    tok2 = np.where(np.arange(R) == 5, tokens, (tokens + 17) % V)
    ids1, lp1 = _launch(other, tok2, 8, ldl=V + 2, offset=1)
    assert np.array_equal(ids0[5], ids1[5]) and np.array_equal(lp0[5].view(np.uint32), lp1[5].view(np.uint32))
    assert not np.array_equal(ids0[6], ids1[6])


def test_nothing_but_the_two_output_arrays_is_written():
    """The logits (gaps between rows included) and the tokens are bit-equal after the launch."""
    from promptcache_amd import _native
    V, R, ldl = 1027, 4, 1031
    rng = np.random.default_rng(11)
    buf = torch.from_numpy(rng.standard_normal(R * ldl + 5).astype(np.float32)).cuda()
    tk = torch.from_numpy(rng.integers(0, V, R * 4)).cuda()
    before, tk0 = buf.clone(), tk.clone()
    ids = torch.zeros((R, 9), dtype=torch.int32, device="cuda")
    lp = torch.zeros((R, 9), dtype=torch.float32, device="cuda")
    _native.token_logprobs(buf[1:], ldl, V, R, tk, 4, 8, ids, lp)
    torch.cuda.synchronize()
    assert torch.equal(buf.view(torch.int32), before.view(torch.int32)) and torch.equal(tk, tk0)


def test_argument_errors():
    from promptcache_amd import _native
    lib = _native.load()
    x = torch.zeros(4 * 64, dtype=torch.float32, device="cuda")
    t64 = torch.zeros(4, dtype=torch.int64, device="cuda")
    t32 = torch.zeros(4, dtype=torch.int32, device="cuda")
    ids = torch.zeros(4 * 9, dtype=torch.int32, device="cuda")
    lp = torch.zeros(4 * 9, dtype=torch.float32, device="cuda")
    P = lambda t: ctypes.c_void_p(t.data_ptr())
    good = dict(logits=P(x), ldl=64, vocab=64, rows=4, tok64=P(t64), tok32=None, stride=1, top_n=8, ids=P(ids), lp=P(lp))

    def call(**kw):
        a = {**good, **kw}
        return lib.pc_token_logprobs(a["logits"], a["ldl"], a["vocab"], a["rows"], a["tok64"], a["tok32"], a["stride"], a["top_n"],
                                     a["ids"], a["lp"], None)
    assert call() == 0
    torch.cuda.synchronize()
    for bad in (dict(logits=None), dict(ids=None), dict(lp=None), dict(tok64=None), dict(tok32=P(t32)), dict(rows=0), dict(rows=65),
                dict(top_n=-1), dict(top_n=9), dict(vocab=8, ldl=8), dict(vocab=1 << 24, ldl=1 << 24), dict(ldl=63), dict(stride=0),
                dict(logits=ctypes.c_void_p(x.data_ptr() + 2))):
        assert call(**bad) == -1001, bad
        assert b"pc_token_logprobs" in lib.pc_last_error_string()
    assert call(tok64=None, tok32=P(t32)) == 0
    torch.cuda.synchronize()
