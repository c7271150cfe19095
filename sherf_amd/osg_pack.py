"""Packing of the OSG path's weights into the fp32 block `sherf_osg_decoder` (sherf_amd/csrc/osg.hip) reads; the layout is documented at the entry
point in include/sherf_hip.h.  Like mlp_pack.stream_index the layout is stated ONCE as an index map -- slot i of the block = element src[i] of the flat
vector of `flat_sizes()` (or zero where src[i] < 0) -- which the renderer applies on the device with one gather every time a parameter changes
(ImportanceRenderer._pack_osg).  The gains of the FullyConnectedLayers are folded into the flat vector, not into the map.
Reference: renderer.py:423-424, 949-993, triplane.py:242-265, networks_stylegan2.py:96-131."""
import functools

import numpy as np

HEAD_FLOATS = 3524            # wbp 1152 + h0 2048 + hb0 64 + h1 256 + hb1 4: what a workgroup keeps in LDS
TRANS_FLOATS = 8416
# the transformer's parameters in block order; (name under transformer.layers.0, shape, stored transposed)
TRANS_PARAMS = (('0.fn.norm.weight', (32,), False), ('0.fn.norm.bias', (32,), False), ('0.fn.fn.to_qkv.weight', (144, 32), False),
                ('0.fn.fn.to_out.0.weight', (32, 48), True), ('0.fn.fn.to_out.0.bias', (32,), False), ('1.fn.norm.weight', (32,), False),
                ('1.fn.norm.bias', (32,), False), ('1.fn.fn.net.0.weight', (32, 32), False), ('1.fn.fn.net.0.bias', (32,), False),
                ('1.fn.fn.net.3.weight', (32, 32), True), ('1.fn.fn.net.3.bias', (32,), False))


def flat_sizes(use_trans):
    """(name, shape) of the flat vector's pieces, in order: W_b [32, 32] (columns 32..63 of the effective reprojection matrix), the head's two layers
    WITH their gains applied, then the transformer's parameters as stored."""
    out = [('W_b', (32, 32)), ('net.0.weight', (64, 32)), ('net.0.bias', (64,)), ('net.2.weight', (4, 64)), ('net.2.bias', (4,))]
    if use_trans:
        out += [(n, s) for n, s, _ in TRANS_PARAMS]
    return out


def pe5_feature(L, slot):
    """The PE5(rgb) feature lane L of a sample's four holds in slot `slot` (csrc/osg.hip), or -1: PE5 = [rgb, sin(2^q rgb), cos(2^q rgb), q = 0..4]
    (renderer.py:875-916) cut to 32 features; angle n = 3 q + a has its sine at 3 + 6 q + a and its cosine at 6 + 6 q + a."""
    if slot == 8:
        return L if L < 3 else -1
    n = L + 4 * (slot // 2)
    if n > 14:
        return -1
    q, a = divmod(n, 3)
    f = (3 if slot % 2 == 0 else 6) + 6 * q + a
    return f if f < 32 else -1


@functools.lru_cache(None)
def block_index(use_trans):
    """-> src int64 [HEAD_FLOATS (+ TRANS_FLOATS)]: element of the flat vector per block slot, -1 = zero."""
    el, off = {}, 0
    for name, shape in flat_sizes(use_trans):
        n = int(np.prod(shape))
        el[name] = np.arange(off, off + n, dtype=np.int64).reshape(shape)
        off += n
    wbp = np.full((9, 8, 4, 4), -1, np.int64)
    for s in range(9):
        for L in range(4):
            f = pe5_feature(L, s)
            if f >= 0:
                wbp[s, :, L, :] = el['W_b'][:, f].reshape(8, 4)
    # every one of the 32 kept features is held by exactly one (lane, slot)
    held = sorted(pe5_feature(L, s) for s in range(9) for L in range(4) if pe5_feature(L, s) >= 0)
    assert held == list(range(32)), held
    W0, b0, W1, b1 = el['net.0.weight'], el['net.0.bias'], el['net.2.weight'], el['net.2.bias']
    h0 = W0.reshape(4, 16, 8, 4).transpose(1, 2, 0, 3)           # [L][i][k/4][k%4] -> [i][k/4][L][k%4]
    hb0 = b0.reshape(4, 16).T                                    # [i][L]
    h1 = W1.reshape(4, 4, 16).transpose(2, 1, 0)                 # [o][L][i] -> [i][L][o]
    parts = [wbp.reshape(-1), h0.reshape(-1), hb0.reshape(-1), h1.reshape(-1), b1.reshape(-1)]
    assert sum(p.size for p in parts) == HEAD_FLOATS
    if use_trans:
        for name, shape, transposed in TRANS_PARAMS:
            parts.append((el[name].T if transposed else el[name]).reshape(-1))
        assert sum(p.size for p in parts) == HEAD_FLOATS + TRANS_FLOATS
    return np.concatenate(parts), off
