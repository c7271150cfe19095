"""The backward of the OSGDecoder path (use_NeRF_decoder=False) on the HOST build of the unchanged kernel sources (tests/hipcpu): the `check_*` bodies
below are shared with tests/test_gpu_osg_backward.py, which runs them on the MI355X.  The fused head kernel (sherf_bwd_osg_head, csrc/bwd_dense.hip)
is compared with float64 autograd of the head; whole training steps with recorded gradients of the UNMODIFIED reference
(tools/make_golden_osg_grad.py -> tests/golden/grad_tiny_ri_osg*.npz)."""
import ctypes
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import sherf_oracle as O
from sherf_amd import _lib
from tests import gpu_common as G
from tests import test_hipcpu_osg as OSG
from tests.test_hipcpu_frame import cpu_product          # noqa: F401  (the host builds behind sherf_amd._lib, CPU tensors)

#        golden tag      use_trans  clamp_mode
CASES = {'osg':          (True,     'relu'),
         'osg_notrans':  (False,    'relu'),
         'osg_softplus': (True,     'softplus')}
HEAD_KEYS = ('net.0.weight', 'net.0.bias', 'net.2.weight', 'net.2.bias')
SENTINEL = -7.5
LDZ, LDD = 100, 104


def _dev(a):
    return G.dev_tensor(torch.from_numpy(np.ascontiguousarray(a)))


def _sync():
    if not G.CPU_SHIM:
        torch.cuda.synchronize()


# ---- 1. the kernel alone, through the C ABI ---------------------------------------------------------------------------------------
def _head(z, W0g, b0g, W1g, b1g):
    """OSGDecoder.forward (triplane.py:253-265) on the gain-folded layers: z [n,3,32] -> [n,4] = (r, g, b, sigma), d_sample's columns."""
    a = z.mean(1) @ W0g.t() + b0g
    y = F.softplus(a) @ W1g.t() + b1g
    return torch.cat((torch.sigmoid(y[:, 1:]) * (1 + 2 * 0.001) - 0.001, y[:, 0:1]), -1), a


def _head_grads(dtype, z, d, params):
    """Autograd of sum(head * d) at `dtype`: (d_z [n,96], dW0g, db0g, dW1g, db1g) as float64, and the pre-activations a."""
    leaves = [t.to(dtype).clone().requires_grad_(True) for t in (z, *params)]
    out, a = _head(*leaves)
    (out * d.to(dtype)).sum().backward()
    return [leaves[0].grad.reshape(z.shape[0], 96).double()] + [t.grad.double() for t in leaves[1:]], a.detach()


def _call_head(z_buf, d, params, dz_buf, sums, n, max_blocks):
    P = lambda t: ctypes.c_void_p(t.data_ptr())
    rc = _lib.lib_bwd().sherf_bwd_osg_head(P(z_buf), LDZ, P(d), n, *[P(t) for t in params], P(dz_buf), LDD, *[P(t) for t in sums], max_blocks, _lib.stream())
    assert rc == 0, _lib.lib_bwd().sherf_bwd_last_error()
    _sync()


NAMES = ('d_z', 'dW0g', 'db0g', 'dW1g', 'db1g')


def check_head_kernel():
    """n = 1, 37, 1000 under max_blocks = 2 (eight trips per workgroup, the last one ragged) and 1000 under the default grid; ldz = 100 / ldd = 104 with
    NaN in the padding of z and a sentinel in that of d_z; sample 0 has hidden units above softplus's threshold 20.  Per output, relative to its largest
    entry: ours <= 2 x (fp32 torch autograd's distance from float64 autograd on the same inputs) + 1e-3 (the rule of
    tests/test_gpu_backward.py::_full_size_backward).  A second call ADDS to the four parameter sums and rewrites d_z; the padding stays bit for bit.
    One more case off the 16-byte path: n = 37 from a z / d_z shifted by one float (the dword accesses)."""
    rs = np.random.RandomState(43)
    p = OSG._random_params(rs)
    params = [p['net.0.weight'] * np.float32(1 / np.sqrt(32)), p['net.0.bias'], p['net.2.weight'] * np.float32(1 / np.sqrt(64)), p['net.2.bias']]
    NMAX = 1000
    z = torch.from_numpy(rs.standard_normal((NMAX, 3, 32)).astype(np.float32))
    z[0] = 30.0 * params[0][5] / float(params[0][5].square().sum())                     # a[5] = 30 for sample 0 (every token the same: so is the mean)
    d = torch.from_numpy(rs.standard_normal((NMAX, 4)).astype(np.float32))
    a64 = _head(z.double(), *[t.double() for t in params])[1]
    assert bool((a64[0] > 20).any()) and bool((a64[1:] < 20).all()) and float((a64 - 20).abs().min()) > 1e-3      # (no unit near the switch: fp32 takes the same side)
    dev_params = [_dev(t.numpy()) for t in params]
    pad = torch.full((NMAX, LDD - 96), SENTINEL).view(torch.int32)
    for n, max_blocks, shift in ((1, 0, 0), (37, 0, 0), (1000, 2, 0), (1000, 0, 0), (37, 0, 1)):
        truth, _ = _head_grads(torch.float64, z[:n], d[:n], params)
        f32, _ = _head_grads(torch.float32, z[:n], d[:n], params)
        zb = torch.full((n * LDZ + shift,), float('nan'))
        zb[shift:].view(n, LDZ)[:, :96] = z[:n].reshape(n, 96)
        z_buf, dz_buf = _dev(zb.numpy()), _dev(np.full(n * LDD + shift, SENTINEL, np.float32))
        sums = [_dev(np.zeros(t.shape, np.float32)) for t in params]
        for calls in (1, 2):
            _call_head(z_buf[shift:], _dev(d[:n].numpy()), dev_params, dz_buf[shift:], sums, n, max_blocks)
            got = G.plain(dz_buf)[shift:].view(n, LDD)
            assert torch.equal(got[:, 96:].contiguous().view(torch.int32), pad[:n]), (n, max_blocks, 'padding of d_z touched')
            ours = [got[:, :96].double()] + [G.plain(t).double() / calls for t in sums]
            for name, o, t, f in zip(NAMES, ours, truth, f32):
                big = float(t.abs().max())
                e_k, e_f = float((o - t).abs().max()) / big, float((f - t).abs().max()) / big
                print(f'osg head n={n} max_blocks={max_blocks} shift={shift} call {calls} {name}: ours {e_k:.3e}, fp32 torch {e_f:.3e} (of the largest entry, {big:.3e})')
                assert e_k <= 2 * e_f + 1e-3, (n, max_blocks, shift, calls, name, e_k, e_f)
        assert bool(torch.isfinite(G.plain(dz_buf)).all())


# ---- 2. ABI -----------------------------------------------------------------------------------------------------------------------------
def check_head_abi():
    """Declared and exported; null pointers, n < 0, ldz / ldd < 96, max_blocks < 0 are argument errors before anything is launched (the buffers are far
    too small for a launch to survive, and stay untouched); n == 0 returns 0 and launches nothing."""
    assert 'sherf_bwd_osg_head' in _lib.parse_header(_lib.HEADER_BWD)
    assert hasattr(ctypes.CDLL(_lib.LIB_BWD_PATH), 'sherf_bwd_osg_head')
    l = _lib.lib_bwd()
    one = _dev(np.full(8, 3.0, np.float32))
    p = ctypes.c_void_p(one.data_ptr())
    good = [p, 96, p, 1, p, p, p, p, p, 96, p, p, p, p, 0, None]
    for i in (0, 2, 4, 5, 6, 7, 8, 10, 11, 12, 13):                 # every pointer in turn
        args = list(good)
        args[i] = None
        assert l.sherf_bwd_osg_head(*args) == -1 and b'bad argument' in l.sherf_bwd_last_error(), i
    for i, v in ((3, -1), (1, 95), (9, 95), (14, -1), (1, 0), (9, -96)):
        args = list(good)
        args[i] = v
        assert l.sherf_bwd_osg_head(*args) == -1 and b'bad argument' in l.sherf_bwd_last_error(), (i, v)
    args = list(good)
    args[3] = 0
    assert l.sherf_bwd_osg_head(*args) == 0                           # n == 0
    _sync()
    assert bool((G.plain(one) == 3.0).all())


# ---- 3. the training step against the unmodified reference's gradients ----------------------------------------------------------------
def osg_grad_frame(rend, dec, clamp_mode='relu'):
    """A grad-enabled forward of `tiny_ri` through the OSG path with the three feature inputs as leaves -> (rgb, depth, acc, leaves)."""
    from sherf_amd.voxel import SparseConvTensor
    fx = G.fixture('tiny_ri')
    sp_input = G.oracle_render('tiny_ri')['sp_input']
    d = G.to_cuda(fx['input_data'])
    leaf = lambda k: (torch.from_numpy(fx[k]) if G.CPU_SHIM else torch.from_numpy(fx[k]).cuda()).requires_grad_(True)
    leaves = {'input.planes': leaf('planes'), 'input.obs_feat': leaf('obs_feat'), 'input.vertex_feat': leaf('vertex_feat')}
    sp = SparseConvTensor(leaves['input.vertex_feat'], G.dev_tensor(sp_input['coord']), sp_input['out_sh'], 1)
    spi = dict(coord=G.dev_tensor(sp_input['coord']), out_sh=sp_input['out_sh'], batch_size=1, bounds=G.dev_tensor(sp_input['bounds'])[None])
    opts = dict(fx['options'], mlp_precision='f16x3', clamp_mode=clamp_mode)
    with torch.enable_grad():
        rgb, depth, acc = rend(leaves['input.planes'], d['obs_img_all'][:, 0], leaves['input.obs_feat'], sp, None, spi, dec, d['ray_o_all'][:, 0],
                               d['ray_d_all'][:, 0], d['near_all'][:, 0], d['far_all'][:, 0], d, opts)
    return rgb, depth, acc, leaves


def check_full_backward(tag):
    """Forward with both switches on, stub loss, loss.backward() on `tiny_ri` (628 valid samples) against tests/golden/grad_tiny_ri_<tag>.npz: the set of
    gradient names equals the golden's; every gradient within 1e-2 on the norm and 5e-2 on the fingerprint's entries (the bounds of
    tests/test_gpu_backward.py::test_full_backward_against_reference_gradients); the four decoder gradients IN FULL within 1e-2 of their norm.
    The loss: the image is within 1e-4 of its largest entry (tests/test_hipcpu_osg.py::check_frame), so each squared difference moves by at most
    4e-4 and the loss (1.6) by 5e-4 of itself; bound 1e-3."""
    use_trans, clamp_mode = CASES[tag]
    ref = np.load(os.path.join(G.GOLDEN, f'grad_tiny_ri_{tag}.npz'))
    rend, dec = OSG.osg_modules('f16x3', use_trans, fresh=True)       # fresh: the step moves running statistics and leaves .grad behind
    assert (rend.transformer is not None) == use_trans
    rend.enable_autograd = rend.enable_osg_autograd = True
    try:
        rgb, depth, acc, leaves = osg_grad_frame(rend, dec, clamp_mode)
        assert rgb.requires_grad and acc.requires_grad and not depth.requires_grad
        assert int(rend.last['ws']['counters'][0]) == 628
        loss = O.stub_loss(rgb[0], acc[0, :, 0])
        loss.backward()
        _sync()
    finally:
        del rend.enable_autograd, rend.enable_osg_autograd
    e_loss = abs(float(loss.detach()) - float(ref['loss'])) / float(ref['loss'])
    print(f'osg backward {tag}: loss {float(loss.detach()):.6f} vs the reference\'s {float(ref["loss"]):.6f} ({e_loss:.2e})')
    assert e_loss < 1e-3
    grads = {k: v.grad for k, v in leaves.items()}
    for mod, pre in ((rend, 'renderer.'), (dec, 'decoder.')):
        for name, p_ in mod.named_parameters():
            if p_.grad is not None:
                assert p_.grad.shape == p_.shape, pre + name
                grads[pre + name] = p_.grad
    names = [k for k in ref.files if k != 'loss' and not k.startswith('full.')]
    assert set(names) == set(grads), set(names) ^ set(grads)
    worst = [0.0, 0.0, '', '']
    for k in names:
        ours, r = O.grad_fingerprint(G.plain(grads[k]).float()), ref[k]
        en, ev = abs(ours[2] - r[2]) / (r[2] + 1e-30), np.linalg.norm(ours[3:] - r[3:]) / (np.linalg.norm(r[3:]) + 1e-30)
        if en > worst[0]:
            worst[0], worst[2] = en, k
        if ev > worst[1]:
            worst[1], worst[3] = ev, k
        assert en < 1e-2, (k, ours[2], r[2])
        assert ev < 5e-2, (k, ev)
    print(f'osg backward {tag}: {len(names)} gradients, worst norm error {worst[0]:.3e} ({worst[2]}), worst fingerprint error {worst[1]:.3e} ({worst[3]})')
    for k in HEAD_KEYS:
        full = torch.from_numpy(ref['full.decoder.' + k]).double()
        e = float((G.plain(grads['decoder.' + k]).double() - full).norm() / full.norm())
        print(f'osg backward {tag}: decoder.{k} in full, {e:.3e} of its norm')
        assert e < 1e-2, (k, e)


# ---- 4. the switch ------------------------------------------------------------------------------------------------------------------------
def check_switch():
    """enable_autograd alone: NotImplementedError naming the OSG path and the new switch; with enable_osg_autograd beside it the forward is recorded; a
    second forward before the first frame's backward makes that backward refuse (the workspace is the second frame's)."""
    from sherf_amd.renderer import ImportanceRenderer
    assert ImportanceRenderer.enable_osg_autograd is False
    rend, dec = OSG.osg_modules('f16x3', use_trans=False, fresh=True)
    rend.enable_autograd = True
    try:
        with pytest.raises(NotImplementedError, match='OSG') as ei:
            osg_grad_frame(rend, dec)
        assert 'enable_osg_autograd' in str(ei.value)
        rend.enable_osg_autograd = True
        rgb1, _, acc1, _ = osg_grad_frame(rend, dec)
        assert rgb1.requires_grad and rgb1.grad_fn is not None
        rgb2, _, acc2, leaves2 = osg_grad_frame(rend, dec)
        with pytest.raises(RuntimeError, match='workspace has been overwritten'):
            O.stub_loss(rgb1[0], acc1[0, :, 0]).backward()
        O.stub_loss(rgb2[0], acc2[0, :, 0]).backward()               # the latest frame's backward is fine
        _sync()
        assert float(G.plain(leaves2['input.planes'].grad).abs().max()) > 0 and float(G.plain(dec.net[0].weight.grad).abs().max()) > 0
        with torch.no_grad():                                        # without grad mode nothing is recorded, whatever the switches say
            out = OSG.osg_render_with_grad(rend, dec)
        assert not out[0].requires_grad
    finally:
        del rend.enable_autograd
        if 'enable_osg_autograd' in rend.__dict__:
            del rend.enable_osg_autograd


# ---- the host build ----------------------------------------------------------------------------------------------------------------
def test_osg_head_kernel_against_float64_autograd(cpu_product):
    check_head_kernel()


def test_osg_head_abi(cpu_product):
    check_head_abi()


@pytest.mark.parametrize('tag', list(CASES))
def test_osg_training_step_against_reference_gradients(cpu_product, tag):
    check_full_backward(tag)


def test_osg_autograd_switch(cpu_product):
    check_switch()
