"""Reference for pc_token_logprobs (csrc/pc_logprob.hip): the float64 log-softmax of a raw logits row, the order of its
alternatives, a float32 restatement of the kernel's arithmetic, and the rows the GPU test feeds the kernel.

Conventions of the entry point, restated: NaN counts as -inf everywhere; -inf contributes nothing to the denominator; a row
whose maximum is not finite has no distribution (NaN log-probabilities, ids -1); the alternatives are ordered by (value
descending, index ascending)."""
import numpy as np

TOL = 2e-4            # |lp - float64 lp|, for |logit| <= 64 and V <= 131 072 (derivation: tests/test_gpu_logprob.py)
MAX_TOP = 8           # PC_LOGPROBS_MAX_TOP
LANES = 1024          # threads of the kernel's workgroup: the lanes its sum runs over


def clean(x) -> np.ndarray:
    """The row as the kernel reads it: float64, NaN -> -inf."""
    x = np.asarray(x, dtype=np.float64).copy()
    x[np.isnan(x)] = -np.inf
    return x


def log_softmax(x) -> np.ndarray:
    """float64 log-softmax of one raw row ([V]); all NaN where the row's maximum is not finite."""
    x = clean(x)
    m = x.max()
    if not np.isfinite(m):
        return np.full(x.shape, np.nan)
    with np.errstate(divide="ignore"):
        return (x - m) - np.log(np.exp(x - m).sum())


def order(x) -> np.ndarray:
    """All indices of the row by (value descending, index ascending)."""
    x = clean(x)
    return np.lexsort((np.arange(len(x)), -x))


def record(x, token: int, top_n: int):
    """-> (ids int64 [1 + top_n], lp float64 [1 + top_n]): what pc_token_logprobs writes for one row."""
    lp = log_softmax(x)
    if np.isnan(lp).all():
        return np.full(1 + top_n, -1, dtype=np.int64), np.full(1 + top_n, np.nan)
    top = order(x)[:top_n]
    ok = 0 <= token < len(lp)
    ids = np.concatenate([[token if ok else -1], top]).astype(np.int64)
    return ids, np.concatenate([[lp[token] if ok else np.nan], lp[top]])


def records(rows, tokens, top_n: int):
    """``record`` per row -> (ids [R][1 + top_n], lp [R][1 + top_n])."""
    out = [record(x, int(t), top_n) for x, t in zip(rows, tokens)]
    return np.stack([o[0] for o in out]), np.stack([o[1] for o in out])


def log_softmax_f32(x, lanes: int = LANES) -> np.ndarray:
    """The kernel's arithmetic in float32: the maximum, exp(x - m) per element, one running sum per lane over the elements
    the lane visits (groups of four tokens, lane after lane), a pairwise tree over the lanes, then (x - m) - log(s) with each
    subtraction rounded.  Not bit-for-bit the device (its exp is the hardware's), but the same sums in the same precision."""
    x = np.asarray(x, dtype=np.float32).copy()
    x[np.isnan(x)] = -np.inf
    m = x.max()
    if not np.isfinite(m):
        return np.full(x.shape, np.nan, dtype=np.float32)
    e = np.exp((x - m).astype(np.float32)).astype(np.float32)
    G = (len(x) + 3) // 4
    pad = np.zeros(G * 4, dtype=np.float32)
    pad[:len(x)] = e
    groups = pad.reshape(G, 4)
    part = np.zeros(lanes, dtype=np.float32)
    for g0 in range(0, G, lanes):                         # group g belongs to lane g % lanes; a lane adds its tokens in index order
        blk = groups[g0:g0 + lanes]
        for c in range(4):
            part[:len(blk)] = (part[:len(blk)] + blk[:, c]).astype(np.float32)
    while len(part) > 1:
        part = (part[0::2] + part[1::2]).astype(np.float32)
    logs = np.float32(np.log(part[0]))
    with np.errstate(invalid="ignore"):
        return ((x - m).astype(np.float32) - logs).astype(np.float32)


# ---- the rows of the GPU test -----------------------------------------------------------------------------------------------------
def spike_positions(V: int):
    """Index 0 and each of the last nine indices (every tail length of the 4-token groups and the 16-byte path)."""
    return [0] + [V - 1 - j for j in range(min(9, V - 1))]


def case_rows(V: int, seed: int = 0):
    """name -> fp32 row of V logits, |logit| <= 64.  A dropped spike moves every other entry of its row by
    log(e^20 + V - 1) - log(V - 1) (more than 10 up to V = 22 026, 8.2 at V = 128 256) and changes the first id; the range row loses
    its whole maximum; the ids of the tie rows are exact."""
    rng = np.random.default_rng(1000 + V + seed)
    rows = {}
    rows["normal"] = np.clip(rng.standard_normal(V) * 3.0, -64, 64).astype(np.float32)
    rows["normal_wide"] = np.clip(rng.standard_normal(V) * 12.0, -64, 64).astype(np.float32)
    for p in spike_positions(V):
        x = np.zeros(V, dtype=np.float32)
        x[p] = 20.0
        rows[f"spike@{p}"] = x
    rows["quarters"] = (np.round(np.clip(rng.standard_normal(V) * 1.5, -64, 64) * 4) / 4).astype(np.float32)
    x = np.clip(rng.standard_normal(V) * 2.0, -64, 64).astype(np.float32)
    x[rng.random(V) < 0.3] = -np.inf
    x[min(3, V - 1)] = 1.5                                 # (something finite stays)
    rows["neg_inf"] = x
    x = np.clip(rng.standard_normal(V) * 2.0, -64, 64).astype(np.float32)
    x[rng.random(V) < 0.3] = np.nan
    x[min(5, V - 1)] = 0.25
    rows["nan"] = x
    x = np.full(V, -np.inf, dtype=np.float32)
    x[::3] = np.nan
    rows["nothing_finite"] = x
    x = np.full(V, -64.0, dtype=np.float32)
    x[V // 2] = 64.0
    rows["range"] = x
    rows["constant"] = np.full(V, 1.25, dtype=np.float32)
    return rows


def case_tokens(x, top_n: int):
    """The chosen-token cases of one row: the top-1, one outside the top-n, index V - 1, and two out of range."""
    V = len(x)
    o = order(x)
    return [int(o[0]), int(o[min(top_n + 3, V - 1)]), V - 1, V, -1]
