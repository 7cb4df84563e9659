"""The sampling front end of ``GenerationEngine`` (reference generation_engine.py:32-42, :149-168) on the CPU: the product's
logits-processor chain and the numpy oracle against the fixture the REFERENCE's own chain produced
(tests/golden/sampling_chain.npz, made by ``oracle/gen_golden.py --sampling-only``)."""
import os

import numpy as np
import torch

from oracle import sampling_oracle as so
from promptcache_amd.generation_engine import GenerationParameters

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sampling_chain.npz")


def _cases():
    z = np.load(GOLD)
    for i, (t, rp, tp, tk) in enumerate(z["params"]):
        yield float(t), float(rp), float(tp), int(tk), z["logits"][i], z["history"][i], z["processed"][i]


def test_processor_chain_and_oracle_match_reference_fixture():
    n = 0
    for t, rp, tp, tk, logits, hist, want in _cases():
        params = GenerationParameters(temperature=t, repetition_penalty=rp, top_p=tp, top_k=tk)
        chain = params.get_logits_processor()
        h = torch.as_tensor([hist.tolist()]) if rp > 1.0 else None
        got = chain(h, torch.from_numpy(logits[None].copy()))[0].numpy()
        orc = so.process_logits(logits, hist, t, rp, tp, tk)
        keep = np.isfinite(want)
        assert np.array_equal(np.isfinite(got), keep) and np.array_equal(np.isfinite(orc), keep), (t, rp, tp, tk)
        np.testing.assert_allclose(got[keep], want[keep], rtol=0, atol=0)
        np.testing.assert_allclose(orc[keep], want[keep], rtol=1e-6, atol=1e-6)
        assert params.greedy == so.is_greedy(t, tp)
        n += 1
    assert n == 10


def test_greedy_rule_and_defaults():
    assert GenerationParameters(temperature=0.0).greedy and GenerationParameters(top_p=0.0).greedy
    assert not GenerationParameters().greedy
    assert len(GenerationParameters().get_logits_processor()) == 0          # all defaults: empty chain (:32-42)
    assert len(GenerationParameters(temperature=0.7, repetition_penalty=1.1, top_p=0.9, top_k=3).get_logits_processor()) == 4


def test_processor_chain_and_oracle_reproduce_the_vocab_fixture():
    """The reference's chain at V = 1001 .. 128 256 (tests/golden/sampling_chain_vocab.npz): ties, signed zeros, -inf / NaN /
    +inf rows, top-k at V - 1 .. V + 1 and inside tie runs, top-p down to 1e-8.  The product's chain keeps exactly the
    reference's set; the oracle keeps the same count of every value, at the highest indices of a tie run (tie_canonical), with
    values bit-equal to the chain's."""
    from tests import sample_ref as sr
    n, rows, sizes, ties = 0, set(), set(), 0
    for c in sr.vocab_cases():
        x, hist, t, rp, tp, tk = c["logits"], c["history"], c["T"], c["rp"], c["top_p"], c["top_k"]
        params = GenerationParameters(temperature=t, repetition_penalty=rp, top_p=tp, top_k=tk)
        h = torch.as_tensor(hist[None]) if rp > 1.0 else None
        got = params.get_logits_processor()(h, torch.from_numpy(x[None].copy()))[0].numpy()
        orc = so.process_logits(x, hist, t, rp, tp, tk)
        pre = so.process_logits(x, hist, t, rp, 1.0, -1)
        want = c["kept"]
        assert np.array_equal(got != -np.inf, want), (c["row"], c["family"], x.size, t, rp, tp, tk)
        canon = sr.tie_canonical(pre, want)
        ties += int(np.sum(canon != want))
        assert np.array_equal(orc != -np.inf, canon), (c["row"], c["family"], x.size, t, rp, tp, tk,
                                                       int(want.sum()), int((orc != -np.inf).sum()))
        k = want & canon
        assert np.array_equal(got[k].view(np.uint32), orc[k].view(np.uint32)), (c["row"], t, rp)
        assert np.array_equal(pre[k].view(np.uint32), orc[k].view(np.uint32))
        n += 1
        rows.add(c["row"])
        sizes.add(x.size)
    assert n >= 200 and len(rows) >= 30 and sizes == {1001, 32000, 32016, 50432, 65024, 65537, 128256}
    assert ties > 0            # the fixture does hold boundaries inside tie runs that torch's sort orders otherwise
    print(f"[sampling_chain_vocab] {n} cases over {len(rows)} rows; tokens the tie reading moves: {ties}")
