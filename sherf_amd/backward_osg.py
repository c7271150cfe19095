"""Backward of the per-sample dense stage on the OSGDecoder path (use_NeRF_decoder=False): slot-2 rgb encoding, transformer, OSGDecoder head.

The counterpart of backward_dense.dense_backward, with the same contract, built from the same pieces (backward_dense._Stage: the slot-2
completion, the transformer's recompute and backward, the rgb encoding's weight gradient) around ONE fused kernel for the head
(sherf_bwd_osg_head, csrc/bwd_dense.hip: forward recompute, data gradient and the four parameter gradients of the 32 -> 64 -> 4 head in a launch).
Two things differ from the NeRF path: the head reads the MEAN of all three tokens, so the slot-2 completion runs -- and dWb_pe is non-zero --
without a transformer too, and the transformer's backward receives a gradient in all three slots.
Checked on the CPU against float64 autograd over a torch emulation of the entry points (tests/test_backward_osg.py), the kernel from its source on
the host and on the MI355X (tests/test_hipcpu_osg_backward.py, tests/test_gpu_osg_backward.py).
"""
import torch

from .backward_dense import Mat, _Stage

HEAD = (('decoder.net.0', (64, 32)), ('decoder.net.2', (4, 64)))


def head_gains(decoder):
    """{'decoder.net.0': (weight_gain, bias_gain), 'decoder.net.2': ...}: the run-time gains of the head's FullyConnectedLayers
    (networks_stylegan2.py:96-131); 1 for a layer that has none."""
    return {name: (float(getattr(decoder.net[i], 'weight_gain', 1.0)), float(getattr(decoder.net[i], 'bias_gain', 1.0)))
            for (name, _), i in zip(HEAD, (0, 2))}


def osg_dense_backward(ops, state, tok, ext, d_sample, use_trans, gains):
    """tok [n,96], ext [n,12], d_sample [n,4], state: as dense_backward.  gains: head_gains(decoder).

    Returns (d_tokens_in Mat [n,96], grads {name: tensor}, dWb_pe [32,32]): dense_backward's contract; the head's gradients come under the reference's
    names (decoder.net.0.weight ...), w.r.t. the STORED parameters (the gains multiplied back in)."""
    n, dev = tok.rows, tok.buf.device
    st = _Stage(ops, state, n, dev)
    # ---- forward recompute: the completion always (the mean reads token 2), the transformer when there is one ----
    tin, pe_rgb = st.complete_tokens(tok, ext)
    trans = st.transformer_forward(tin) if use_trans else None
    z96 = trans['z96'] if use_trans else tin
    # ---- the head, forward and backward, in one launch ----
    folded, sums = [], []
    for name, shape in HEAD:
        wg, bg = gains[name]
        f = lambda t, g: Mat.of(t.detach().to(dtype=torch.float32) * g)
        folded += [f(state[name + '.weight'], wg), f(state[name + '.bias'], bg)]
        sums += [st.Z(*shape), st.Z(1, shape[0])]
    d_z = st.E(n, 96)                                                # (the kernel writes every row in full)
    ops.osg_head(z96, d_sample, *folded, d_z, *sums)
    for (name, shape), dWg, dbg in zip(HEAD, sums[0::2], sums[1::2]):
        wg, bg = gains[name]
        st.grads[name + '.weight'] = dWg.tensor().view(shape) * wg
        st.grads[name + '.bias'] = dbg.tensor().view(-1) * bg
    # ---- transformer (all three slots of d_z carry gradient), the rgb encoding's weight ----
    d_tin = st.transformer_backward(trans, d_z) if use_trans else d_z
    return d_tin, st.grads, st.dWb_pe(d_tin, pe_rgb)
