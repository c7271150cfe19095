"""CPU check of the backward ORCHESTRATION of the dense stage on the OSG path (sherf_amd/backward_osg.py) against float64 autograd through the
per-sample function of that path (tests.test_hipcpu_osg.osg_reference: the reference's formulas), with the C entry points replaced by their torch
emulation (tests/bwd_emulator.py + tests/bwd_emulator_osg.py).  No build, no GPU."""
import numpy as np
import pytest
import torch

from sherf_amd.backward_dense import Mat
from sherf_amd.backward_osg import HEAD, osg_dense_backward
from tests.bwd_emulator_osg import OsgEmuOps
from tests.test_hipcpu_osg import _random_params, osg_reference

N = 203                     # not a multiple of anything the kernels tile by
LR_MUL = 2.0                # decoder_lr_mul = 2: weight gains 2 / sqrt(fan_in), bias gains 2 (networks_stylegan2.py:105-113)
T = 'renderer.transformer.layers.0.'
HEAD_KEYS = ('net.0.weight', 'net.0.bias', 'net.2.weight', 'net.2.bias')


def _rel(a, b):
    a, b = torch.as_tensor(a).double(), torch.as_tensor(b).double()
    return float((a - b).abs().max() / b.abs().max())


@pytest.mark.parametrize('use_trans', [True, False])
def test_osg_dense_backward_orchestration(use_trans):
    """d_tin, dWb_pe, the four head gradients (w.r.t. the STORED parameters under non-unit gains) and the transformer's gradients.  Bound 1e-4 of each
    gradient's largest entry: the emulation is fp32 (eps 6e-8) over sums of 203 samples and chains of a few hundred operations -- 1e-5 at the very
    most -- while any error of the orchestration (a slot, a transposition, a gain, a missing term) is of order one."""
    rs = np.random.RandomState(5)
    p = _random_params(rs)                                           # the head's weights as the module stores them under lr_mul = 1 ...
    stored = {k: p[k] / LR_MUL for k in HEAD_KEYS}                   # ... and under lr_mul = 2: the same effective layers from half the parameters
    tok = torch.from_numpy(rs.standard_normal((N, 3, 32)).astype(np.float32))
    rgb = torch.from_numpy(rs.uniform(0, 1, (N, 3)).astype(np.float32))
    d_sample = torch.from_numpy(rs.standard_normal((N, 4)).astype(np.float32))
    # ---- float64 autograd: osg_reference applies the lr_mul = 1 gains itself, so it is fed LR_MUL x the stored parameters ----
    leaves = {k: v.double().requires_grad_(True) for k, v in p.items() if k not in HEAD_KEYS}
    leaves.update({k: v.double().requires_grad_(True) for k, v in stored.items()})
    tok64 = tok.double().requires_grad_(True)
    fed = {k: (v * LR_MUL if k in HEAD_KEYS else v) for k, v in leaves.items()}
    out = osg_reference(tok64, rgb, fed, torch.float64, use_trans)  # [n, 4] = (r, g, b, sigma): d_sample's columns
    (out * d_sample.double()).sum().backward()
    # ---- the orchestration on the emulated entry points ----
    Wr = torch.zeros(32, 96, 1)
    Wr[:, 32:64, 0] = p['W_b']
    state = {'renderer.conv1d_reprojection.weight': Wr}
    state.update({'decoder.' + k: v for k, v in stored.items()})
    if use_trans:
        state.update({T + k: v for k, v in p.items() if k[0] in '01'})
    gains = {'decoder.net.0': (LR_MUL / np.sqrt(32), LR_MUL), 'decoder.net.2': (LR_MUL / np.sqrt(64), LR_MUL)}
    ext = torch.zeros(N, 12)
    ext[:, 6:9] = rgb
    with torch.no_grad():
        d_tin, grads, dWb_pe = osg_dense_backward(OsgEmuOps(), state, Mat(tok.reshape(-1).clone(), N, 96), Mat(ext.reshape(-1).clone(), N, 12),
                                                  Mat(d_sample.reshape(-1).clone(), N, 4), use_trans, gains)
    # the completion adds a term to token 2 that does not depend on the tokens: d_tin == d_tok
    assert (d_tin.rows, d_tin.cols) == (N, 96) and _rel(d_tin.tensor().reshape(N, 3, 32), tok64.grad) < 1e-4
    assert float(tok64.grad[:, 2].abs().max()) > 0                   # (all three slots carry gradient on this path)
    assert dWb_pe.shape == (32, 32) and _rel(dWb_pe, leaves['W_b'].grad) < 1e-4
    want = {'decoder.' + k: leaves[k].grad for k in HEAD_KEYS}
    if use_trans:
        want.update({T + k: v.grad for k, v in leaves.items() if k[0] in '01'})
    assert set(want) == set(grads), set(want) ^ set(grads)
    assert {name + s for name, _ in HEAD for s in ('.weight', '.bias')} <= set(grads)
    for k, g in want.items():
        assert tuple(grads[k].shape) == tuple(g.shape), k
        assert _rel(grads[k], g) < 1e-4, (k, _rel(grads[k], g))
