"""The OSGDecoder path (use_NeRF_decoder=False) on the HOST build of the unchanged kernel sources (tests/hipcpu): the `check_*` bodies below are shared
with tests/test_gpu_osg.py, which runs them on the MI355X.  Frames are compared with recorded outputs of the UNMODIFIED reference
(tools/make_golden_osg.py -> tests/golden/renderer_tiny_ri_osg*.npz); the kernel alone with a float64 torch evaluation of the reference's formulas.

Measured (per-sample rgb / activated sigma / image, relative to the largest entry; host build | MI355X): see DESIGN section 5.4."""
import ctypes
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import fixtures
from sherf_amd import _lib, osg_pack
from tests import gpu_common as G
from tests.test_hipcpu_frame import cpu_product          # noqa: F401  (the host builds behind sherf_amd._lib, CPU tensors)

#        golden tag          use_trans  branches              clamp_mode
CASES = {'osg':              (True,     (True, True, True),   'relu'),
         'osg_notrans':      (False,    (True, True, True),   'relu'),
         'osg_softplus':     (True,     (True, True, True),   'softplus'),
         'osg_notrans_f101': (False,    (True, False, True),  'relu'),
         'osg_f100':         (True,     (True, False, False), 'relu')}
DEC_KEYS = {'net.0.weight': (64, 32), 'net.0.bias': (64,), 'net.2.weight': (4, 64), 'net.2.bias': (4,)}


def golden(tag):
    return np.load(os.path.join(G.GOLDEN, f'renderer_tiny_ri_{tag}.npz'))


def _dev(a):
    return G.dev_tensor(torch.from_numpy(np.ascontiguousarray(a)))


# ---- renderer + decoder pairs on the OSG path ----------------------------------------------------------------------------------
_MODULES = {}


def osg_modules(precision='f16x3', use_trans=True, branches=(True, True, True), fresh=False):
    """(renderer, OSGDecoder): the renderer with the reference-init weights of `tiny_ri`, the decoder with the parameters recorded in the goldens
    (the same in all five files).  One pair per configuration and build (host / device) unless `fresh`."""
    from sherf_amd.renderer import ImportanceRenderer
    from sherf_amd.triplane import OSGDecoder
    key = (G.CPU_SHIM, precision, use_trans, tuple(branches))
    if not fresh and key in _MODULES:
        return _MODULES[key]
    rend = ImportanceRenderer(*branches, use_trans=use_trans, use_NeRF_decoder=False, smpl=G.smpl(), mlp_precision=precision)
    dec = OSGDecoder(32, {'decoder_lr_mul': 1, 'decoder_output_dim': 3})
    fixtures.load_seeded_state(rend, 'renderer.', 'ri')
    g = golden('osg')
    dec.load_state_dict({k: torch.from_numpy(g['decoder.' + k]) for k in DEC_KEYS})
    if G.CPU_SHIM:
        rend._side = lambda dev, idx=0: type('HostStream', (), {'cuda_stream': 8 + 8 * idx})()
    pair = (G.dev_module(rend).train(), G.dev_module(dec).train())
    if not fresh:
        _MODULES[key] = pair
    return pair


def osg_render(precision='f16x3', use_trans=True, branches=(True, True, True), options=None, modules=None):
    """sherf_amd.ImportanceRenderer.forward on `tiny_ri` through the OSG path (tests.gpu_common.hip_render with the other decoder)."""
    from sherf_amd.voxel import SparseConvTensor
    fx = G.fixture('tiny_ri')
    rend, dec = modules or osg_modules(precision, use_trans, branches)
    sp_input = G.oracle_render('tiny_ri')['sp_input']
    d = G.to_cuda(fx['input_data'])
    sp = SparseConvTensor(G.to_cuda(fx['vertex_feat']), G.dev_tensor(sp_input['coord']), sp_input['out_sh'], 1)
    spi = dict(coord=G.dev_tensor(sp_input['coord']), out_sh=sp_input['out_sh'], batch_size=1, bounds=G.dev_tensor(sp_input['bounds'])[None])
    opts = dict(fx['options'], mlp_precision=precision)
    opts.update(options or {})
    with torch.no_grad():
        rgb, depth, acc = rend(G.to_cuda(fx['planes']), d['obs_img_all'][:, 0], G.to_cuda(fx['obs_feat']), sp, None, spi, dec,
                               d['ray_o_all'][:, 0], d['ray_d_all'][:, 0], d['near_all'][:, 0], d['far_all'][:, 0], d, opts)
    if not G.CPU_SHIM:
        torch.cuda.synchronize()
    return dict(rgb=G.plain(rgb[0]), depth=G.plain(depth[0, :, 0]), acc=G.plain(acc[0, :, 0]), last=rend.last, rend=rend, dec=dec)


# ---- 1. the kernel alone, through the C ABI ---------------------------------------------------------------------------------------
def _random_params(rs):
    """Weights at the scales of the reference's constructors (kaiming-uniform linears, LayerNorm around (1, 0), unit-variance FullyConnectedLayers)."""
    u = lambda *sh: rs.uniform(-1, 1, sh) / np.sqrt(sh[-1])
    p = {'W_b': u(32, 32) * np.sqrt(32 / 96),
         '0.fn.norm.weight': 1 + 0.1 * rs.standard_normal(32), '0.fn.norm.bias': 0.1 * rs.standard_normal(32),
         '0.fn.fn.to_qkv.weight': u(144, 32), '0.fn.fn.to_out.0.weight': u(32, 48), '0.fn.fn.to_out.0.bias': u(32, 48)[:, 0],
         '1.fn.norm.weight': 1 + 0.1 * rs.standard_normal(32), '1.fn.norm.bias': 0.1 * rs.standard_normal(32),
         '1.fn.fn.net.0.weight': u(32, 32), '1.fn.fn.net.0.bias': u(32, 32)[:, 0], '1.fn.fn.net.3.weight': u(32, 32), '1.fn.fn.net.3.bias': u(32, 32)[:, 0],
         'net.0.weight': rs.standard_normal((64, 32)), 'net.0.bias': 0.3 * rs.standard_normal(64),
         'net.2.weight': rs.standard_normal((4, 64)), 'net.2.bias': 0.3 * rs.standard_normal(4)}
    return {k: torch.from_numpy(np.asarray(v, np.float32)) for k, v in p.items()}


def osg_reference(tok, rgb, p, dtype, use_trans):
    """The per-sample function of the OSG path in torch at `dtype`, from the reference's formulas: the slot-2 completion (renderer.py:423-424 with
    PositionalEncoding, :900-916), the transformer (:920-993), OSGDecoder.forward (triplane.py:253-265) with FullyConnectedLayer's gains
    (networks_stylegan2.py:96-131; lr_multiplier 1).  tok [n,3,32], rgb [n,3] -> [n,4] = (r, g, b, sigma)."""
    P = {k: v.to(dtype) for k, v in p.items()}
    x, c = tok.to(dtype).clone(), rgb.to(dtype)
    freqs = torch.repeat_interleave(2.0 ** torch.linspace(0.0, 4.0, 5), 2).to(dtype).view(1, -1, 1)
    phases = torch.zeros(10, dtype=dtype)
    phases[1::2] = torch.pi * 0.5
    embed = torch.sin(torch.addcmul(phases.view(1, -1, 1), c.unsqueeze(1).repeat(1, 10, 1), freqs)).view(c.shape[0], -1)
    pe = torch.cat((c, embed), -1)[:, :32]
    x[:, 2] = x[:, 2] + pe @ P['W_b'].t()
    if use_trans:
        ln = F.layer_norm(x, (32,), P['0.fn.norm.weight'], P['0.fn.norm.bias'], 1e-5)
        q, k, v = [t.view(-1, 3, 3, 16).permute(0, 2, 1, 3) for t in (ln @ P['0.fn.fn.to_qkv.weight'].t()).chunk(3, dim=-1)]      # b h n d
        attn = (torch.einsum('bhid,bhjd->bhij', q, k) * 16 ** -0.5).softmax(-1)
        o = torch.einsum('bhij,bhjd->bhid', attn, v).permute(0, 2, 1, 3).reshape(-1, 3, 48)
        x = o @ P['0.fn.fn.to_out.0.weight'].t() + P['0.fn.fn.to_out.0.bias'] + x
        ln = F.layer_norm(x, (32,), P['1.fn.norm.weight'], P['1.fn.norm.bias'], 1e-5)
        h = F.gelu(ln @ P['1.fn.fn.net.0.weight'].t() + P['1.fn.fn.net.0.bias'])
        x = h @ P['1.fn.fn.net.3.weight'].t() + P['1.fn.fn.net.3.bias'] + x
    m = x.mean(1)
    h = F.softplus(torch.addmm(P['net.0.bias'].unsqueeze(0), m, (P['net.0.weight'] * (1 / np.sqrt(32))).t()))
    y = torch.addmm(P['net.2.bias'].unsqueeze(0), h, (P['net.2.weight'] * (1 / np.sqrt(64))).t())
    return torch.cat((torch.sigmoid(y[:, 1:]) * (1 + 2 * 0.001) - 0.001, y[:, 0:1]), -1)


def pack_block(p, use_trans):
    """The weight block of sherf_osg_decoder from a dict of parameters (osg_pack's index map applied with numpy)."""
    flat = [p['W_b'].reshape(-1), p['net.0.weight'].reshape(-1) * np.float32(1 / np.sqrt(32)), p['net.0.bias'],
            p['net.2.weight'].reshape(-1) * np.float32(1 / np.sqrt(64)), p['net.2.bias']]
    if use_trans:
        flat += [p[n].reshape(-1) for n, _, _ in osg_pack.TRANS_PARAMS]
    flat = torch.cat(flat + [torch.zeros(1)])
    src, n_flat = osg_pack.block_index(use_trans)
    assert flat.numel() == n_flat + 1 and src.size == osg_pack.HEAD_FLOATS + (osg_pack.TRANS_FLOATS if use_trans else 0)
    return flat[torch.from_numpy(np.where(src >= 0, src, n_flat))].contiguous()


SENTINEL = -7.5
CAP = 128                     # four tiles


def _run_kernel(tokens, extras, block, n, flags, out=None):
    counters = _dev(np.array([n, 0, 0, 0, 0, 0, 0, 0], np.int32))
    out = _dev(np.full((CAP, 4), SENTINEL, np.float32)) if out is None else out
    P = _lib.ptr
    _lib.call('sherf_osg_decoder', P(counters), P(tokens), P(extras), P(block), flags, CAP, P(out), _lib.stream())
    if not G.CPU_SHIM:
        torch.cuda.synchronize()
    return G.plain(out)


def check_kernel():
    """n in {0, 1, 31, 32, 33, 77} valid samples of 128 (four tiles), both transformer settings: rows < n within twice the fp32 torch evaluation's own
    distance from the float64 one, plus 1e-6; rows >= n keep the sentinel bit for bit (n = 0: every row); tokens / extras beyond n are NaN, so a
    sample read as valid would show."""
    rs = np.random.RandomState(41)
    p = _random_params(rs)
    tok = torch.from_numpy(rs.standard_normal((CAP, 3, 32)).astype(np.float32))
    ex = torch.from_numpy(rs.standard_normal((CAP, 12)).astype(np.float32))
    ex[:, 6:9] = torch.from_numpy(rs.uniform(0, 1, (CAP, 3)).astype(np.float32))
    sentinel = torch.full((CAP, 4), SENTINEL).view(torch.int32)
    for use_trans in (True, False):
        truth = osg_reference(tok, ex[:, 6:9], p, torch.float64, use_trans)
        f32 = osg_reference(tok, ex[:, 6:9], p, torch.float32, use_trans).double()
        block = _dev(pack_block(p, use_trans).numpy())
        for n in (0, 1, 31, 32, 33, 77):
            t, e = tok.clone(), ex.clone()
            t[n:], e[n:] = float('nan'), float('nan')
            tokens = _dev(t.view(CAP // 32, 32, 3, 8, 4).permute(0, 2, 3, 1, 4).contiguous().numpy())
            extras = _dev(e.view(CAP // 32, 32, 12).permute(0, 2, 1).contiguous().numpy())
            out = _run_kernel(tokens, extras, block, n, 0 if use_trans else 1)
            assert torch.equal(out[n:].contiguous().view(torch.int32), sentinel[n:]), (use_trans, n)
            if n == 0:
                continue
            e_f32 = float((f32[:n] - truth[:n]).abs().max())
            e_k = float((out[:n].double() - truth[:n]).abs().max())
            print(f'osg kernel use_trans={use_trans} n={n}: kernel {e_k:.3e}, fp32 torch {e_f32:.3e} (max |.| against float64; outputs up to {float(truth[:n].abs().max()):.2f})')
            assert e_k <= 2 * e_f32 + 1e-6, (use_trans, n, e_k, e_f32)


# ---- 2. the frame against the unmodified reference's ------------------------------------------------------------------------------
def check_frame(tag):
    """The one-call frame against tests/golden/renderer_tiny_ri_<tag>.npz at the bounds of tests/test_hipcpu_frame.py::check_feature_branch_switches /
    tests/test_hipcpu_softplus.py::check_frame: per-sample rgb, per-sample activated sigma, image rgb / acc within 1e-4 of the largest entry, depth within
    rtol 1e-3 / atol 1e-4 under 'f16x3'; the image within 2e-3 under 'f16'."""
    use_trans, branches, clamp_mode = CASES[tag]
    g = golden(tag)
    act = (lambda x: F.softplus(torch.as_tensor(x).double() - 1)) if clamp_mode == 'softplus' else (lambda x: torch.as_tensor(x).double().clamp(min=0))
    h = osg_render('f16x3', use_trans, branches, options=dict(clamp_mode=clamp_mode))
    assert h['last']['mlp_precision'] == 'f16x3' and h['last']['table_precision'] == 'f32'
    nv = int(h['last']['ws']['counters'][0])
    assert nv == int(g['n_valid'])
    so = G.plain(h['last']['ws']['sample_out'][:nv])
    e_rgb, e_sig = G.rel(so[:, :3], g['sample_rgb']), G.rel(act(so[:, 3]), act(g['sample_sigma']))
    e_img = max(G.rel(h['rgb'], g['rgb']), G.rel(h['acc'], g['acc'][:, 0]))
    print(f'osg frame {tag}: per-sample rgb {e_rgb:.2e} activated sigma {e_sig:.2e}, image {e_img:.2e}, depth {float((h["depth"] - torch.from_numpy(g["depth"][:, 0])).abs().max()):.2e}')
    assert e_rgb < 1e-4 and e_sig < 1e-4 and e_img < 1e-4, (tag, e_rgb, e_sig, e_img)
    assert torch.allclose(h['depth'], torch.from_numpy(g['depth'][:, 0]), rtol=1e-3, atol=1e-4)
    h16 = osg_render('f16', use_trans, branches, options=dict(clamp_mode=clamp_mode))
    assert h16['last']['mlp_precision'] == 'f16' and h16['last']['table_precision'] == 'f16'
    e16 = G.rel(h16['rgb'], g['rgb'])
    print(f'osg frame {tag}: fp16 tables, image {e16:.2e}')
    assert e16 < 2e-3, (tag, e16)


# ---- 3. use_trans=False runs the slot-2 completion --------------------------------------------------------------------------------
def check_completion_without_transformer():
    """The NeRF kernel skips W_b . PE5(rgb) without a transformer (its decoder never reads token 2); the OSG mean reads all three tokens.  The
    `osg_notrans` frame must differ from the one rendered with W_b zeroed by more than 1e-3."""
    h = osg_render('f16x3', use_trans=False)
    rend, dec = osg_modules('f16x3', use_trans=False, fresh=True)
    with torch.no_grad():
        rend.conv1d_reprojection.weight[:, 32:64] = 0
    z = osg_render('f16x3', use_trans=False, modules=(rend, dec))
    d = G.rel(h['rgb'], z['rgb'])
    print(f'osg_notrans: image moves by {d:.2e} when W_b is zeroed')
    assert d > 1e-3, d
    assert G.rel(h['rgb'], golden('osg_notrans')['rgb']) < 1e-4


# ---- 4. no state left behind ------------------------------------------------------------------------------------------------------
def check_no_state_left_behind():
    """NeRF frame, OSG frame on a second renderer, NeRF frame again: the two NeRF frames are bit-identical.  mlp_precision='auto' under OSG renders
    no calibration or tuning frame: every forward enqueues the frame exactly once (a fresh workspace's sampler probe, phase 4, apart) and reports
    the fp32-grade configuration."""
    before = G.hip_render('tiny_ri', precision='f16x3')
    o = osg_render('f16x3')
    after = G.hip_render('tiny_ri', precision='f16x3')
    assert after['rend'] is before['rend'] and o['rend'] is not before['rend']
    for k in ('rgb', 'depth', 'acc'):
        assert torch.equal(after[k], before[k]), k
    assert G.rel(o['rgb'], before['rgb']) > 1e-3                 # (another decoder: another image)
    phases, call = [], _lib.call

    def counting(name, *args):
        if name == 'sherf_render_frame':
            phases.append(int(args[1]))
        return call(name, *args)
    _lib.call = counting
    try:
        modules = osg_modules('auto', fresh=True)
        a1 = osg_render('auto', modules=modules)
        first = list(phases)
        del phases[:]
        a2 = osg_render('auto', modules=modules)
    finally:
        _lib.call = call
    assert [p for p in first if p != 4] == [3] and phases == [3], (first, phases)
    rend = a1['rend']
    assert a1['last']['mlp_precision'] == 'f16x3' and a2['last']['mlp_precision'] == 'f16x3' and a2['last']['table_precision'] == 'f32'
    assert getattr(rend, 'auto_report', None) is None and getattr(rend, 'form_report', None) is None
    for k in ('rgb', 'depth', 'acc'):
        assert torch.equal(a1[k], o[k]) and torch.equal(a2[k], o[k]), k


# ---- 5. construction and names ------------------------------------------------------------------------------------------------------
def check_construction():
    from sherf_amd.triplane import NeRFDecoder, OSGDecoder, TriPlaneGenerator
    stub = torch.nn.Identity
    gen = TriPlaneGenerator(512, 0, 48, True, True, True, True, False, img_resolution=128, img_channels=3, rendering_kwargs=dict(decoder_lr_mul=2),
                            backbone=stub(), encoder_2d=stub(), encoder_2d_feature=stub(), smpl={})
    assert isinstance(gen.decoder, OSGDecoder) and not gen.renderer.use_NeRF_decoder
    g = golden('osg')
    sd = gen.decoder.state_dict()
    assert {k: tuple(v.shape) for k, v in sd.items()} == DEC_KEYS == {k[len('decoder.'):]: tuple(g[k].shape) for k in g.files if k.startswith('decoder.')}
    # FullyConnectedLayer's initialisation under decoder_lr_mul (networks_stylegan2.py:105-113): randn / lr_mul, zero bias, gains lr_mul / sqrt(in), lr_mul
    l0, l2 = gen.decoder.net[0], gen.decoder.net[2]
    assert abs(float(l0.weight.detach().std()) - 0.5) < 0.05 and bool((l0.bias == 0).all()) and bool((l2.bias == 0).all())
    assert (l0.weight_gain, l0.bias_gain, l2.weight_gain) == (2 / np.sqrt(32), 2, 2 / np.sqrt(64))
    with pytest.raises(RuntimeError, match='sherf_osg_decoder'):
        gen.decoder(torch.zeros(1, 3, 4, 32), torch.zeros(1, 4, 3))
    # the module's gains reach the weight block
    rend, dec = osg_modules('f16x3', use_trans=False)
    dec2 = OSGDecoder(32, {'decoder_lr_mul': 2, 'decoder_output_dim': 3})
    with torch.no_grad():
        for (_, a), (_, b) in zip(dec2.named_parameters(), dec.named_parameters()):
            a.copy_(G.plain(b) / 2)
    assert torch.equal(G.plain(rend._pack_osg(G.dev_module(dec2), dec.net[0].weight.device)), G.plain(rend._pack_osg(dec, dec.net[0].weight.device)))
    # the autograd path names what it lacks; a decoder of the other kind is refused
    rend.enable_autograd = True
    try:
        with torch.enable_grad(), pytest.raises(NotImplementedError, match='OSG'):
            osg_render_with_grad(rend, dec)
    finally:
        del rend.enable_autograd
    with pytest.raises(TypeError, match='use_NeRF_decoder=False'):
        osg_render('f16x3', use_trans=False, modules=(rend, G.dev_module(NeRFDecoder(32))))
    nerf_rend, _ = G.hip_modules('f16x3', 'ri')
    with pytest.raises(TypeError, match='use_NeRF_decoder=True'):
        osg_render('f16x3', modules=(nerf_rend, dec))


def osg_render_with_grad(rend, dec):
    from sherf_amd.voxel import SparseConvTensor
    fx = G.fixture('tiny_ri')
    sp_input = G.oracle_render('tiny_ri')['sp_input']
    d = G.to_cuda(fx['input_data'])
    sp = SparseConvTensor(G.to_cuda(fx['vertex_feat']), G.dev_tensor(sp_input['coord']), sp_input['out_sh'], 1)
    spi = dict(coord=G.dev_tensor(sp_input['coord']), out_sh=sp_input['out_sh'], batch_size=1, bounds=G.dev_tensor(sp_input['bounds'])[None])
    return rend(G.to_cuda(fx['planes']), d['obs_img_all'][:, 0], G.to_cuda(fx['obs_feat']), sp, None, spi, dec, d['ray_o_all'][:, 0],
                d['ray_d_all'][:, 0], d['near_all'][:, 0], d['far_all'][:, 0], d, dict(fx['options']))


# ---- 6. ABI ---------------------------------------------------------------------------------------------------------------------------
def check_abi():
    """The entry point is declared and exported; unknown flag bits, null pointers and a non-positive capacity are argument errors before anything is
    launched (the buffers are far too small for a launch to survive, and stay untouched); SHERF_MLP_OSG_DECODER without a weight block likewise."""
    assert 'sherf_osg_decoder' in _lib.parse_header()
    l = _lib.lib()
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), 'sherf_osg_decoder')
    assert (_lib.MLP_NO_TRANSFORMER, _lib.MLP_OSG_DECODER) == (256, 512)
    src = open(_lib.HEADER).read()
    assert '#define SHERF_MLP_OSG_DECODER 512' in src and '#define SHERF_MLP_NO_TRANSFORMER 256' in src
    one, cnt = _dev(np.full(8, 3.0, np.float32)), _dev(np.array([1, 0, 0, 0, 0, 0, 0, 0], np.int32))
    p, c = ctypes.c_void_p(one.data_ptr()), ctypes.c_void_p(cnt.data_ptr())
    for flags in (2, 4, 256, 512, 1 << 16, -1):
        assert l.sherf_osg_decoder(c, p, p, p, flags, 32, p, None) == -1 and b'bad argument' in l.sherf_last_error()
    for args in ((None, p, p, p), (c, None, p, p), (c, p, None, p), (c, p, p, None)):
        assert l.sherf_osg_decoder(*args, 1, 32, p, None) == -1
    assert l.sherf_osg_decoder(c, p, p, p, 1, 32, None, None) == -1
    assert l.sherf_osg_decoder(c, p, p, p, 1, 0, p, None) == -1 and l.sherf_osg_decoder(c, p, p, p, 0, -5, p, None) == -1
    # the NeRF entry points do not take the frame's OSG bit
    assert l.sherf_nerf_mlp(c, p, p, p, p, 1 | 512, 32, p, None) == -1
    fr = _lib.Frame()
    fr.mlp_prec = 1 | _lib.MLP_OSG_DECODER
    lv = (_lib.VoxLevel * 3)()
    assert l.sherf_render_frame(ctypes.byref(fr), 3, lv, None, ctypes.c_void_p(8), None) == -1 and b'wstream' in l.sherf_last_error()
    assert bool((G.plain(one) == 3.0).all()) and G.plain(cnt).tolist() == [1, 0, 0, 0, 0, 0, 0, 0]


# ---- the host build ----------------------------------------------------------------------------------------------------------------
def test_osg_kernel_against_float64(cpu_product):
    check_kernel()


@pytest.mark.parametrize('tag', list(CASES))
def test_osg_frame_against_reference_golden(cpu_product, tag):
    check_frame(tag)


def test_osg_completion_runs_without_transformer(cpu_product):
    check_completion_without_transformer()


def test_osg_leaves_no_state_behind(cpu_product):
    check_no_state_left_behind()


def test_osg_construction_and_names(cpu_product):
    check_construction()


def test_osg_abi(cpu_product):
    check_abi()


def test_osg_block_index_is_a_permutation_of_the_parameters():
    """Every parameter element lands in the block exactly once (W_b: the 32 kept PE5 features once each; nothing dropped, nothing doubled)."""
    for use_trans in (False, True):
        src, n_flat = osg_pack.block_index(use_trans)
        used = np.sort(src[src >= 0])
        assert np.array_equal(used, np.arange(n_flat)), use_trans
        assert src.size == osg_pack.HEAD_FLOATS + (osg_pack.TRANS_FLOATS if use_trans else 0) and int((src < 0).sum()) == 1152 - 1024
