"""The many-row attention kernels pinned where Gaussian operands under a tolerance cannot see: one key too many or too few
(``test_key_census``), and the running-max paths after the first tile (``test_running_max_profiles``).

Kernels: attn_fwd_kernel in its plain and HP forms, attn_fwd32_kernel (pc_attn.hip), attn_ring_kernel (pc_attn_ring.hip),
attn_wide_kernel with its own-rows ring partial and attn_combine_kernel (pc_attn_wide.hip).  The routes, the dispatch rule that
selects each, the census operands and the score profiles are in tests/attn_ref.py; tests/test_attn_ref_cpu.py checks from the
reference alone that the census threshold is decisive and that every profile has the property it is named for.

Every launch: K, V and the residual planes NaN behind the valid rows, slack rows in the arena, outputs and workspace NaN-filled.
Each profile case prints an ``ATTN_PIN`` line (collected in profiles/attn_pins.json).
"""
import numpy as np
import pytest
import torch

from tests import attn_ref as ar

pytestmark = pytest.mark.gpu

DEV = "cuda"
NAN = float("nan")
ENV_SWITCHES = ("PC_ATTN_NO_RING", "PC_ATTN_NO_WIDE", "PC_ATTN_WIDE_MIN")


def _n():
    from promptcache_amd import _native
    return _native


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _padded(valid, rows, axis):
    """``valid`` with its ``axis`` grown to ``rows``, NaN behind the valid rows."""
    shape = list(valid.shape)
    shape[axis] = rows
    t = torch.full(shape, NAN, dtype=torch.float16, device=DEV)
    t.narrow(axis, 0, valid.shape[axis]).copy_(_dev(valid))
    return t


def _route_env(monkeypatch, r, **extra):
    """The per-call switches of the route: nothing for most; PC_ATTN_WIDE_MIN for the wide routes; PC_ATTN_NO_RING=1 for the
    64-row HP form at head_dim 128 (>= 33 split-precision rows would go to the ring kernel)."""
    for k in ENV_SWITCHES:
        monkeypatch.delenv(k, raising=False)
    if r.kind == "wide":
        monkeypatch.setenv("PC_ATTN_WIDE_MIN", ar.WIDE_MIN)
    if r.kind == "hp64" and r.D == 128:
        monkeypatch.setenv("PC_ATTN_NO_RING", "1")
    for k, v in extra.items():
        monkeypatch.setenv(k, v)


class Launch:
    """Device operands of one (route, operands) pair; ``run`` launches pc_attn and returns float64 [B, T, H * D] (hi + lo)."""

    def __init__(self, r, ops, frag=False):
        self.r, self.frag = r, frag
        B, T, H, Hkv, D = r.B, r.q_len, r.H, r.Hkv, r.D
        self.hp = ar.split_precision(r)
        self.q = _dev(ops["q"].reshape(B, T, H * D))
        self.q_lo = _dev(ops["q_lo"].reshape(B, T, H * D)) if self.hp else None
        self.kv_lo = self.prefix = self.past_lens = None
        self.past_arg = max(ar.pasts(r))
        if r.kind == "ring_prefix":
            rows = T + 7
            self.k, self.v = _padded(ops["k"], rows, 2), _padded(ops["v"], rows, 2)
            self.k_lo, self.v_lo = _padded(ops["k_lo"], rows, 2), _padded(ops["v_lo"], rows, 2)
            self.kv_bs, self.kv_hs = Hkv * rows * D, rows * D
            self.kv_lo = (self.k_lo, self.v_lo, Hkv * rows * D, rows * D, 0)
            # (trunk rows behind the longest prefix: NaN)
            tk, tv, tkl, tvl = (ops[x].copy() for x in ("trunk_k", "trunk_v", "trunk_k_lo", "trunk_v_lo"))
            for a in (tk, tv, tkl, tvl):
                a[:, self.past_arg:] = np.nan
            self.trunk = [_dev(a) for a in (tk, tv, tkl, tvl)]
            self.prefix = (*self.trunk, ar.N_TRUNK * D)
            self.past_lens = torch.tensor(ar.pasts(r), dtype=torch.int32, device=DEV)
            self.inputs = [self.q, self.q_lo, self.k, self.v, self.k_lo, self.v_lo, *self.trunk]
        else:
            S = r.past + T
            cap = S + 7
            self.k, self.v = _padded(ops["k"], cap, 2), _padded(ops["v"], cap, 2)
            self.kv_bs, self.kv_hs = Hkv * cap * D, cap * D
            self.inputs = [self.q, self.k, self.v] + ([self.q_lo] if self.hp else [])
            if r.lo_mode == "own":       # compact planes of the pass's own rows (lo_row0 = -1 -> past_len), 5 slack rows
                self.k_lo, self.v_lo = _padded(ops["k_lo"][:, :, r.past:], T + 5, 2), _padded(ops["v_lo"][:, :, r.past:], T + 5, 2)
                self.kv_lo = (self.k_lo, self.v_lo, Hkv * (T + 5) * D, (T + 5) * D, -1)
            elif r.lo_mode == "all":     # arena-shaped planes: every key
                self.k_lo, self.v_lo = _padded(ops["k_lo"], cap, 2), _padded(ops["v_lo"], cap, 2)
                self.kv_lo = (self.k_lo, self.v_lo, Hkv * cap * D, cap * D, 0)
            if self.kv_lo:
                self.inputs += [self.k_lo, self.v_lo]
        self.before = [t.clone() for t in self.inputs]
        self.ws = None

    def run(self):
        n, r = _n(), self.r
        B, T, H, Hkv, D = r.B, r.q_len, r.H, r.Hkv, r.D
        # (sized under the switches of this very call: PC_ATTN_WIDE_MIN is read per call)
        ws_bytes = n.attn_workspace_bytes(B, H, D, T, self.past_arg + T)
        self.ws = torch.full((max(ws_bytes, 4) // 4,), NAN, dtype=torch.float32, device=DEV)
        scale = 1.0 / np.sqrt(D)
        kw = dict(q_lo=self.q_lo, kv_lo=self.kv_lo, past_lens=self.past_lens, prefix=self.prefix)
        if self.frag:
            mt = (B * T + 15) // 16
            oh = torch.full((mt, H * D // 32, 64, 8), NAN, dtype=torch.float16, device=DEV)
            ol = torch.full_like(oh, NAN)
            n.attn_fwd(self.q, T * H * D, H * D, self.k, self.v, self.kv_bs, self.kv_hs, None, 0, 0, B, H, Hkv, D, T, self.past_arg,
                       scale, self.ws, out_frag=(oh, ol), **kw)
            torch.cuda.synchronize()
            full = (oh.double() + ol.double()).view(mt, H * D // 32, 4, 16, 8).permute(0, 3, 1, 2, 4).reshape(mt * 16, H * D)
            return full[:B * T].view(B, T, H * D).cpu().numpy()
        out = torch.full((B, T, H * D), NAN, dtype=torch.float16, device=DEV)
        out_lo = torch.full_like(out, NAN) if self.hp else None
        n.attn_fwd(self.q, T * H * D, H * D, self.k, self.v, self.kv_bs, self.kv_hs, out, T * H * D, H * D, B, H, Hkv, D, T, self.past_arg,
                   scale, self.ws, out_lo=out_lo, **kw)
        torch.cuda.synchronize()
        return (out.double() + (out_lo.double() if self.hp else 0.0)).cpu().numpy()

    def inputs_unchanged(self):
        return all(torch.equal(a.view(torch.int16), b.view(torch.int16)) for a, b in zip(self.inputs, self.before))

    def workspace_written(self):
        return not bool(torch.isnan(self.ws).all())


_OPS = {}


def _census(r, design):
    """(operands, count, n) -- built once per (route, design), shared by the tests, never modified."""
    key = (r.name, design)
    if key not in _OPS:
        ops = ar.census_operands(r, design)
        _OPS[key] = (ops, *ar.census_counts(r, ops))
    return _OPS[key]


CENSUS_CASES = [(r.name, frag) for r in ar.ROUTES for frag in ((False, True) if ar.split_precision(r) and r.kind != "ring_prefix" else (False,))]


@pytest.mark.parametrize("design", ["zero", "equal"])
@pytest.mark.parametrize("name,frag", CENSUS_CASES, ids=[f"{n}{'-frag' if f else ''}" for n, f in CENSUS_CASES])
def test_key_census(name, frag, design, monkeypatch):
    """One-hot V, scores equal along the key axis: out[i, h, c] * n_i is the number of visible keys in column c.  A correct kernel
    is off by fp16 output rounding (<= count * 2^-11 <= 0.05); a key wrongly dropped or admitted moves its column by > 0.9."""
    r = ar.ROUTE[name]
    ops, count, nvis = _census(r, design)
    _route_env(monkeypatch, r)
    L = Launch(r, ops, frag)
    got = L.run().reshape(r.B, r.q_len, r.H, r.D)
    assert not np.isnan(got).any(), f"{int(np.isnan(got).sum())} NaN outputs"
    rep = r.H // r.Hkv
    diff = got * nvis[:, :, None, None] - np.repeat(count, rep, axis=2)
    bad = np.argwhere(np.abs(diff) > 0.25)
    if len(bad):
        lines = []
        for b, i, h, c in bad[:6]:
            seen, unseen = ar.census_keys(r, ops, b, h // rep, c, nvis[b, i])
            d = diff[b, i, h, c]
            keys = unseen[:3] if d > 0 else seen[-3:]
            lines.append(f"  batch {b} row {i} head {h} column {c}: got * n - count = {d:+.3f} (n = {nvis[b, i]}, count = {count[b, i, h // rep, c]}); "
                         f"{'admitted beyond the mask' if d > 0 else 'dropped'}: key {keys} (staged keys end at {ar.pasts(r)[b]})")
        pytest.fail(f"{len(bad)} census entries off by more than 0.25 on {name} ({r.rule}):\n" + "\n".join(lines))
    assert L.inputs_unchanged(), "the launch wrote to Q, the arena or a residual plane"


@pytest.mark.parametrize("name", [r.name for r in ar.ROUTES])
def test_splits_really_ran(name, monkeypatch):
    """The routes that claim KV splits (attn_ref.ROUTES) leave partials in the workspace; the others leave it all NaN.  Holds the
    census to the route it names when choose_nsplit / ring_nsplit / wide_nsplit are retuned."""
    r = ar.ROUTE[name]
    ops, _, _ = _census(r, "equal")
    _route_env(monkeypatch, r)
    L = Launch(r, ops)
    L.run()
    assert L.workspace_written() == r.splits, (name, r.rule, int(L.ws.numel()))


PROFILE_CASES = [(rn, pn) for rn in ar.PROFILE_ROUTES for pn in ar.PROFILES]


@pytest.mark.parametrize("rname,pname", PROFILE_CASES, ids=[f"{a}-{b}" for a, b in PROFILE_CASES])
def test_running_max_profiles(rname, pname, monkeypatch):
    """Score profiles with large late jumps, early spikes, single rows that move and steps on both sides of the wide kernel's
    deferral, against float64 attention on the very operands (hi + lo planes), at the project's own tolerances:
    split-precision 64-row: max|d| < 2e-5; ring / wide: < 2e-5, <= 2 err(64-row kernel, PC_ATTN_NO_RING=1) + 1e-6 and within
    4e-6 of that launch; wide within 2e-6 of the ring kernel alone (PC_ATTN_NO_WIDE=1); plain fp16: atol 4e-3, rtol 1e-2.
    A missed or doubled rescale is an O(1) error under any of them.  Two launches give the same bits."""
    r = ar.ROUTE[rname]
    ops = ar.profile_operands(pname, r)
    ref = ar.reference(r, ops)
    _route_env(monkeypatch, r)
    L = Launch(r, ops)
    got = L.run()
    err = float(np.abs(got - ref).max()) if not np.isnan(got).any() else NAN
    print(f"ATTN_PIN route={rname} profile={pname} err={err:.4e} n_max={r.past + r.q_len}", end="")
    assert not np.isnan(got).any()
    if r.kind in ("ring", "wide"):
        _route_env(monkeypatch, r, PC_ATTN_NO_RING="1")
        old = Launch(r, ops).run()
        err_old, d_old = float(np.abs(old - ref).max()), float(np.abs(got - old).max())
        print(f" err_64row={err_old:.4e} d_64row={d_old:.4e}", end="")
        d_ring = 0.0
        if r.kind == "wide":
            _route_env(monkeypatch, r, PC_ATTN_NO_WIDE="1")
            d_ring = float(np.abs(got - Launch(r, ops).run()).max())
            print(f" d_ring={d_ring:.4e}", end="")
        print()
        assert err < 2e-5 and err <= 2.0 * err_old + 1e-6, (err, err_old)
        assert d_old < 4e-6, d_old
        assert d_ring < 2e-6, d_ring
    elif r.kind == "hp64":
        print()
        assert err < 2e-5, err
    else:
        print()
        np.testing.assert_allclose(got, ref, atol=4e-3, rtol=1e-2)
    _route_env(monkeypatch, r)
    assert np.array_equal(got, L.run()), "two launches of the same call differ"
    assert L.inputs_unchanged()
