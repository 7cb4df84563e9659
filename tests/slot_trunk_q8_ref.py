"""Numpy reference of the shared-trunk slot attention over int8 K / V images (csrc/pc_slots_q8.hip:
pc_attn_decode_slots_trunk_q8).  Test infrastructure only.

A member with T shared rows attends over rows [0, T) of its LEADER's image, rows [T, len) of its own image and the row that was
just appended, exact from its fp16 arena: ``slot_kv_q8_ref.attend`` over the concatenation.  Its own image rows [0, T) do not
enter.  T = 0 (a slot on its own) is ``slot_kv_q8_ref.attend`` on the slot's own image."""
import numpy as np

from tests import slot_kv_q8_ref as ref


def attend(q: np.ndarray, T: int, leader_k, leader_v, own_k, own_v, k_new16: np.ndarray, v_new16: np.ndarray) -> np.ndarray:
    """One slot.  q ``[H][D]`` fp32; ``leader_k`` / ``leader_v`` / ``own_k`` / ``own_v``: (codes ``[Hkv][>= len][D]`` int8, scales
    ``[Hkv][>= len]`` fp32) of layer and plane, of which rows [0, T) of the leader's and rows [T, len) of the slot's own are used
    (``len`` = the rows ``own_k`` is cut to by the caller: pass exactly ``len`` rows); ``k_new16`` / ``v_new16`` ``[Hkv][D]`` fp16.
    -> ``[H][D]`` fp32."""
    (lkc, lks), (lvc, lvs), (okc, oks), (ovc, ovs) = leader_k, leader_v, own_k, own_v
    assert 0 <= T <= okc.shape[1] and (T == 0 or T <= lkc.shape[1])
    cat = lambda a, b: np.concatenate([a[:, :T], b[:, T:]], axis=1)
    return ref.attend(q, cat(lkc, okc), cat(lks, oks), cat(lvc, ovc), cat(lvs, ovs), k_new16, v_new16)
