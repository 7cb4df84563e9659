"""Numpy reference of the prompt-lookup step over int8 K / V images (csrc/pc_slots_q8.hip: pc_rope_append_slots_rows_q8 /
pc_attn_verify_slots_q8).  Test infrastructure only; built on tests/kv_q8_ref.py and tests/lookup_slots_ref.verify_attend.

The step computes what the one-token loop over images computes token by token: the token at position p attends to rows [0, p) as
IMAGE rows -- ``float32(code) * scale``, no fp16 rounding -- and to its own row p exactly.  So draft row i of a slot with length
``len`` sees the image rows [0, len), the rows len .. len + i - 1 of THIS step quantised (``kv_q8_ref.quantise``), and row len + i
in fp16.  Where a step's boundaries fall, and how many drafts were accepted, does not enter."""
import numpy as np

from tests import kv_q8_ref as q8
from tests import lookup_slots_ref as lsr
from tests.slot_kv_q8_ref import dequant32

F32 = np.float32


def step_keys(codes: np.ndarray, scale: np.ndarray, new16: np.ndarray, length: int, i: int) -> np.ndarray:
    """The ``length + i + 1`` keys (or values) draft row i sees, fp32 ``[Hkv][length + i + 1][D]``: ``codes`` / ``scale`` = the image
    rows in front of the step (``[Hkv][>= length][D]`` int8, ``[Hkv][>= length]`` fp32), ``new16`` fp16 ``[Hkv][k + 1][D]`` = the
    step's own rows."""
    assert new16.dtype == np.float16
    c, s = q8.quantise(new16[:, :i])
    return np.concatenate([dequant32(codes[:, :length], scale[:, :length]), dequant32(c, s), new16[:, i:i + 1].astype(F32)], axis=1)


def verify_attend_q8(q, codes_k, scale_k, codes_v, scale_v, k_new16, v_new16, length: int, k: int) -> np.ndarray:
    """One slot: q ``[k + 1][H][D]`` (RoPE applied) -> ``[k + 1][H][D]`` float64.  Row i is ``verify_attend``'s single row over
    ``step_keys(.., i)``: every key in front of its own quantised, its own exact."""
    q = np.asarray(q)
    out = np.zeros(q.shape, dtype=np.float64)
    for i in range(k + 1):
        K = step_keys(codes_k, scale_k, k_new16, length, i)
        V = step_keys(codes_v, scale_v, v_new16, length, i)
        out[i] = lsr.verify_attend(q[i:i + 1], K, V, length + i, 0)[0]
    return out
