"""Numpy reference of the shared-trunk verify attention (csrc/pc_lookup_slots.hip, pc_attn_verify_slots_trunk): the k + 1 draft rows
of one slot over a TRUNK of keys (read from the group leader's arena, visible to every draft row) and the slot's OWN keys (masked
per draft row), each part reduced to the partial record the kernels leave and merged as the merge launch merges them, trunk
first.  Built on tests/trunk_ref.py; imports nothing of the product."""
import numpy as np

from tests import trunk_ref as tr


def verify_attend_trunk(q, K_trunk, V_trunk, K_own, V_own, length, k):
    """q [k+1][H][D] fp32; K_trunk / V_trunk [Hkv][T][D]: keys [0, T); K_own / V_own [Hkv][>= length + k + 1 - T][D]: keys T.. of
    the slot's own arena (rows length - T .. length - T + k are this step's own).  Row i sees the whole trunk and own keys
    [T, length + i].  -> [k+1][H][D] fp32."""
    T = K_trunk.shape[1]
    assert q.shape[0] == k + 1 and 0 <= T <= length and K_own.shape[1] >= length + k + 1 - T
    out = np.empty(q.shape, np.float32)
    for i in range(k + 1):
        n_own = length + i + 1 - T
        out[i] = tr.merge([tr.partial(q[i], K_trunk, V_trunk), tr.partial(q[i], K_own[:, :n_own], V_own[:, :n_own])])
    return out
