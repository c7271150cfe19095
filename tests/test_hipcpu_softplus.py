"""clamp_mode='softplus' and the differentiable dense MipRayMarcher2 on the HOST build of the unchanged kernel sources (tests/hipcpu): the
`check_*` bodies below are shared with tests/test_gpu_softplus.py, which runs them on the MI355X.  Every expected value is a recorded output
of the UNMODIFIED reference (tools/make_golden_softplus.py -> tests/golden/marcher_softplus.npz, renderer_tiny_ri_softplus.npz,
grad_tiny_nv_softplus.npz)."""
import ctypes
import os

import numpy as np
import pytest
import torch

from oracle import sherf_oracle as O
from sherf_amd import _lib
from tests import gpu_common as G
from tests.test_hipcpu_frame import cpu_product          # noqa: F401  (the host builds behind sherf_amd._lib, CPU tensors)

MODES = ('relu', 'softplus')
CASES = ('', 's2_')                                      # R = 300 (crosses one 256-thread block), S = 5 and S = 2


def _marcher_golden():
    return np.load(os.path.join(G.GOLDEN, 'marcher_softplus.npz'))


def _dev(a):
    return G.dev_tensor(torch.from_numpy(np.ascontiguousarray(a)))


def check_dense_forward():
    """sherf_amd.MipRayMarcher2 under softplus against the reference's outputs, at the tolerances tests/test_gpu_parity.py::
    test_units_ray_sampler_and_dense_marcher uses under relu; the all-rejected ray (sigma = -80 throughout) has weights of exactly 0 and the
    global maximum depth."""
    from sherf_amd.ray_marcher import MipRayMarcher2
    g = _marcher_golden()
    for tag in CASES:
        assert (g[tag + 'dens'][0, 0] == -80).all() and g[tag + 'dens'][0, 1].min() > 21 and (g[tag + 'dens'] < 0).any()
        assert (g[tag + 'depths'][0, 2] == g[tag + 'depths'][0, 2, 0]).all()
        for wb in (0, 1):
            with torch.no_grad():
                rgb, dep, w = MipRayMarcher2()(_dev(g[tag + 'colors']), _dev(g[tag + 'dens']), _dev(g[tag + 'depths']), _dev(g[tag + 'rd']),
                                               dict(clamp_mode='softplus', white_back=bool(wb)))
            rgb, dep, w = G.plain(rgb), G.plain(dep), G.plain(w)
            assert w.shape == g[f'{tag}w_{wb}'].shape and w.dim() == 4 and w.shape[-1] == 1
            assert torch.allclose(rgb, torch.from_numpy(g[f'{tag}rgb_{wb}']), atol=2e-6), (tag, wb)
            assert torch.allclose(w, torch.from_numpy(g[f'{tag}w_{wb}']), atol=1e-6), (tag, wb)
            assert torch.allclose(dep, torch.from_numpy(g[f'{tag}depth_{wb}']), atol=1e-5), (tag, wb)
            assert bool((w[0, 0] == 0).all()) and float(dep[0, 0, 0]) == float(g[tag + 'depths'].max())


def _expected_grad(g, key):
    """The reference's gradient of the fixed loss (sum of each output times a seeded tensor).  Where a ray's depth was replaced (empty ray:
    0 / 0 -> nan_to_num) autograd hands its quotient a ZERO upstream gradient and the quotient's backward makes 0 / 0 = NaN of it; the kernel
    drops the depth term there instead (the documented contract), so on exactly the entries where the reference is not finite the expected
    value is the reference's gradient of the same loss WITHOUT its depth term."""
    full, nodepth = torch.from_numpy(g[key]), torch.from_numpy(g[key.replace('d_', 'nodepth_d_', 1)])
    assert bool(torch.isfinite(nodepth).all())
    return torch.where(torch.isfinite(full), full, nodepth), int((~torch.isfinite(full)).sum())


def check_dense_backward():
    """torch.autograd.grad through sherf_amd.MipRayMarcher2, both clamp modes, white_back both ways, S = 5 and S = 2, against autograd through
    the unmodified reference class -- at the kernel-alone tolerances of tests/test_gpu_backward.py::test_composite_backward_kernel (1e-5 of the
    largest entry for the colours, 2e-4 for the density).  A loss that reads only the depth map leaves exactly zero on the empty ray and on
    every ray whose depth the global clamp moved; a `depths` that requires grad is refused."""
    from sherf_amd.ray_marcher import MipRayMarcher2
    g = _marcher_golden()
    n_nan = 0
    for tag in CASES:
        for wb in (0, 1):
            for mode in MODES:
                c, s = _dev(g[tag + 'colors']).requires_grad_(True), _dev(g[tag + 'dens']).requires_grad_(True)
                rgb, dep, w = MipRayMarcher2()(c, s, _dev(g[tag + 'depths']), _dev(g[tag + 'rd']), dict(clamp_mode=mode, white_back=bool(wb)))
                assert rgb.requires_grad and dep.requires_grad and w.requires_grad and w.shape == s.shape
                loss = (rgb * _dev(g[tag + 'g_rgb'])).sum() + (dep * _dev(g[tag + 'g_depth'])).sum() + (w * _dev(g[tag + 'g_w'])).sum()
                dc, ds = torch.autograd.grad(loss, (c, s))
                dc, ds = G.plain(dc), G.plain(ds)
                assert dc.shape == c.shape and ds.shape == s.shape and bool(torch.isfinite(dc).all()) and bool(torch.isfinite(ds).all())
                ec, _ = _expected_grad(g, f'{tag}d_colors_{mode}_{wb}')
                es, k = _expected_grad(g, f'{tag}d_dens_{mode}_{wb}')
                n_nan += k
                e_c, e_s = G.rel(dc, ec), G.rel(ds, es)
                print(f'dense backward {tag or "s5_"}{mode} wb={wb}: colours {e_c:.2e}, density {e_s:.2e} (of the largest entry)')
                assert e_c < 1e-5 and e_s < 2e-4, (tag, mode, wb, e_c, e_s)
                if mode == 'softplus':                   # no sigma > 0 mask: negative sigma takes a gradient
                    assert float(ds[(torch.from_numpy(g[tag + 'dens']) < 0) & (torch.from_numpy(g[tag + 'dens']) > -20)].abs().max()) > 0
    assert n_nan > 0                                     # (the empty ray is in the golden, and is where the two definitions part)
    # upstream gradient on the depth alone, the entry point itself with a NARROWED clamp range so that the clamp does move rays
    col, sig, dep_in, rd = (_dev(g[k]) for k in ('colors', 'dens', 'depths', 'rd'))
    N, S = sig.shape[1], sig.shape[2]
    t = G.plain(dep_in).view(N, S)
    lo, hi = float(t.quantile(0.35)), float(t.quantile(0.65))
    dmm = _dev(np.array([lo, hi], np.float32))
    dev = col.device
    P = _lib.ptr
    for mode in MODES:
        bits = _lib.composite_bits(False, mode)
        rgb, dep, w = torch.empty(N, 3, device=dev), torch.empty(N, device=dev), torch.empty(N, S, device=dev)
        _lib.call('sherf_composite_dense', P(col), P(sig), P(dep_in), P(rd), N, S, bits, P(dmm), P(rgb), P(dep), P(w), _lib.stream())
        d_dep = _dev(g['g_depth']).reshape(N).contiguous()
        d_c, d_s = torch.full((N, S, 3), 7.0, device=dev), torch.full((N, S), 7.0, device=dev)
        _lib.call('sherf_composite_dense_bwd', P(col), P(sig), P(dep_in), P(rd), N, S, bits, P(dmm), None, P(d_dep), None, P(d_c), P(d_s), _lib.stream())
        dep, d_c, d_s = G.plain(dep), G.plain(d_c), G.plain(d_s)
        moved = (dep == lo) | (dep == hi)
        empty = G.plain(w).sum(1) == 0
        assert bool(empty[0]) and bool(moved[0]) and 20 < int(moved.sum()) < N - 20
        assert bool((d_s[moved] == 0).all()) and bool((d_c == 0).all())          # (colours reach the depth through no path at all)
        assert int((d_s[~moved].abs().amax(1) > 0).sum()) > int((~moved).sum()) // 4      # (the other rays do take a depth gradient)
    with pytest.raises(RuntimeError, match='depths'):
        MipRayMarcher2()(_dev(g['colors']).requires_grad_(True), _dev(g['dens']), _dev(g['depths']).requires_grad_(True), _dev(g['rd']),
                         dict(clamp_mode='softplus', white_back=False))


def _depths_like_the_kernel(near, far, S):
    """depth_at of csrc/composite.hip, rounding for rounding: near + fl(fl(k / (S - 1)) * fl(far - near))."""
    step = torch.arange(S, dtype=torch.float32) / torch.tensor(float(S - 1), dtype=torch.float32)
    return near[:, None] + step[None, :] * (far - near)[:, None]


def check_rejected_samples_skip_exactly():
    """The compact kernel walks a ray's valid samples only.  Under softplus a rejected sample (rgb 0, sigma -80 in the reference, renderer.py:364-368)
    has density softplus(-81) ~ 6.6e-36, not 0 -- the kernels' header argues that alpha, the transmittance factor and the weight are still exactly
    what skipping gives.  Tested: a `tiny` frame's compact samples scattered into dense [R,S] buffers (-80 / zeros elsewhere) and composited by
    sherf_composite_dense give bit for bit the rgb / depth / acc of sherf_composite_compact on the compact samples."""
    h = G.hip_render('tiny', options=dict(clamp_mode='softplus'))
    last, fx = h['last'], G.fixture('tiny')
    ws, R, S = last['ws'], last['R'], last['S']
    nv = int(ws['counters'][0])
    assert 100 < nv < R * S // 2
    d = G.to_cuda(fx['input_data'])
    f32 = lambda x, *shape: x.detach().to(torch.float32).contiguous().view(*shape)
    ray_d, near, far = f32(d['ray_d_all'][:, 0], R, 3), f32(d['near_all'][:, 0], R), f32(d['far_all'][:, 0], R)
    dev = ray_d.device
    bits = _lib.composite_bits(False, 'softplus')
    P = _lib.ptr
    out_c = [torch.empty(R, 3, device=dev), torch.empty(R, device=dev), torch.empty(R, device=dev)]
    _lib.call('sherf_composite_compact', P(ws['counters']), P(ws['ray_base']), P(ws['ray_cnt']), P(ws['cs_idx']), P(ws['sample_out']), P(ray_d), P(near),
              P(far), R, S, bits, *[P(o) for o in out_c], _lib.stream())
    # dense buffers on the host, then to the device
    idx = G.plain(ws['cs_idx'][:nv]).long()
    so = G.plain(ws['sample_out'][:nv])
    assert bool((so[:, 3] < 0).any()) and bool((so[:, 3] > 0).any())           # raw sigma reaches the compositing kernel: negatives count under softplus
    colors, sigma = torch.zeros(R * S, 3), torch.full((R * S,), -80.0)
    colors[idx], sigma[idx] = so[:, :3], so[:, 3]
    depths = _depths_like_the_kernel(G.plain(near), G.plain(far), S)
    cnt = G.plain(ws['counters'])[1:3].to(torch.int32)
    dmm = torch.where(cnt >= 0, cnt, cnt ^ 0x7FFFFFFF).view(torch.float32)          # (csrc/common.h: ord2f)
    assert float(dmm[0]) == float(depths.min()) and float(dmm[1]) == float(depths.max())
    col_d, sig_d, dep_d, dmm_d = (G.dev_tensor(x.contiguous()) for x in (colors.view(R, S, 3), sigma.view(R, S), depths, dmm))
    rgb, dep, w = torch.empty(R, 3, device=dev), torch.empty(R, device=dev), torch.empty(R, S, device=dev)
    _lib.call('sherf_composite_dense', P(col_d), P(sig_d), P(dep_d), P(ray_d), R, S, bits, P(dmm_d), P(rgb), P(dep), P(w), _lib.stream())
    w = G.plain(w)
    acc = w[:, 0].clone()
    for k in range(1, S):                                                            # the kernel's own order of summation
        acc = acc + w[:, k]
    rejected = torch.ones(R * S, dtype=torch.bool); rejected[idx] = False
    assert bool((w.reshape(-1)[rejected] == 0).all())
    assert torch.equal(G.plain(rgb), G.plain(out_c[0])) and torch.equal(G.plain(dep), G.plain(out_c[1])) and torch.equal(acc, G.plain(out_c[2]))
    # ... and that is the frame's own image
    assert torch.equal(G.plain(out_c[0]), h['rgb']) and torch.equal(G.plain(out_c[1]), h['depth']) and torch.equal(G.plain(out_c[2]), h['acc'])


def check_frame():
    """The one-call frame under softplus against the unmodified reference's (tests/golden/renderer_tiny_ri_softplus.npz), at the bounds of
    tests/test_hipcpu_frame.py::check_feature_branch_switches; the mode changes the image; a relu frame rendered afterwards on the same renderer is
    the relu frame rendered before, bit for bit (no mode left behind in the descriptor, no `auto` choice carried from one mode to the other)."""
    g = np.load(os.path.join(G.GOLDEN, 'renderer_tiny_ri_softplus.npz'))
    softplus = lambda x: torch.nn.functional.softplus(torch.as_tensor(x).double() - 1)
    before = G.hip_render('tiny_ri', precision='f16x3')
    h = G.hip_render('tiny_ri', precision='f16x3', options=dict(clamp_mode='softplus'))
    nv = int(h['last']['ws']['counters'][0])
    assert nv == int(g['n_valid'])
    so = G.plain(h['last']['ws']['sample_out'][:nv])
    e_rgb, e_sig = G.rel(so[:, :3], g['sample_rgb']), G.rel(softplus(so[:, 3]), softplus(g['sample_sigma']))
    e_img = max(G.rel(h['rgb'], g['rgb']), G.rel(h['acc'], g['acc'][:, 0]))
    print(f'softplus frame: per-sample rgb {e_rgb:.2e} softplus(sigma - 1) {e_sig:.2e}, image {e_img:.2e}')
    assert e_rgb < 1e-4 and e_sig < 1e-4 and e_img < 1e-4, (e_rgb, e_sig, e_img)
    assert torch.allclose(h['depth'], torch.from_numpy(g['depth'][:, 0]), rtol=1e-3, atol=1e-4)
    assert G.rel(h['rgb'], before['rgb']) > 1e-3
    h16 = G.hip_render('tiny_ri', precision='f16', options=dict(clamp_mode='softplus'))
    assert G.rel(h16['rgb'], g['rgb']) < 2e-3
    after = G.hip_render('tiny_ri', precision='f16x3')
    assert after['rend'] is h['rend'] and after['last']['bwd']['clamp_mode'] == 'relu' and h['last']['bwd']['clamp_mode'] == 'softplus'
    for k in ('rgb', 'depth', 'acc'):
        assert torch.equal(after[k], before[k]), k
    # mlp_precision='auto': the choice belongs to the mode it was measured under -- each mode calibrates once, neither disturbs the other's
    G.hip_modules.cache_clear()
    try:
        r1 = G.hip_render('tiny_ri', precision='auto')                   # relu: the calibration frame (fp32-grade)
        r2 = G.hip_render('tiny_ri', precision='auto')                   # relu on its choice
        rend = r2['rend']
        assert r1['last']['mlp_precision'] == 'f16x3' and r2['last']['mlp_precision'] == rend.auto_report['choice']
        s1 = G.hip_render('tiny_ri', precision='auto', options=dict(clamp_mode='softplus'))
        assert s1['rend'] is rend and s1['last']['mlp_precision'] == 'f16x3'                      # softplus calibrates for itself
        choice_s = rend.auto_report['choice']
        s2 = G.hip_render('tiny_ri', precision='auto', options=dict(clamp_mode='softplus'))
        assert s2['last']['mlp_precision'] == choice_s and G.rel(s2['rgb'], g['rgb']) < 2e-3
        r3 = G.hip_render('tiny_ri', precision='auto')                   # back under relu: its kept choice, no third calibration
        assert r3['last']['mlp_precision'] == r2['last']['mlp_precision'] and not rend.auto_report.get('recalibrations')
        for k in ('rgb', 'depth', 'acc'):
            assert torch.equal(r3[k], r2[k]), k
        s3 = G.hip_render('tiny_ri', precision='auto', options=dict(clamp_mode='softplus'))
        assert s3['last']['mlp_precision'] == choice_s and torch.equal(s3['rgb'], s2['rgb'])
    finally:
        G.hip_modules.cache_clear()


def check_whole_chain_backward():
    """renderer.enable_autograd under softplus: forward recorded as one autograd node, the stub loss of BASELINE config 5, loss.backward()
    through the HIP backward pipeline -- every gradient against the fingerprints of the UNMODIFIED reference's under the same option
    (tests/golden/grad_tiny_nv_softplus.npz), under the rule and bounds of tests/test_gpu_backward.py::
    test_full_backward_against_reference_gradients (L2 norm within 1e-2, the 64 strided entries within 5e-2 of their norm)."""
    from sherf_amd.voxel import SparseConvTensor
    cfg = 'tiny_nv'
    fx = G.fixture(cfg)
    ref = np.load(os.path.join(G.GOLDEN, f'grad_{cfg}_softplus.npz'))
    rend, dec = G.hip_modules.__wrapped__()                                # fresh modules: this updates running statistics and .grad
    rend.enable_autograd = True
    d = G.to_cuda(fx['input_data'])
    spi = G.oracle_render(cfg)['sp_input']
    planes, obs_feat, vfeat = (G.to_cuda(fx[k]).requires_grad_(True) for k in ('planes', 'obs_feat', 'vertex_feat'))
    sp = SparseConvTensor(vfeat, G.dev_tensor(spi['coord']), spi['out_sh'], 1)
    spd = dict(coord=G.dev_tensor(spi['coord']), out_sh=spi['out_sh'], batch_size=1, bounds=G.dev_tensor(spi['bounds'])[None])
    opts = dict(fx['options'], clamp_mode='softplus')
    rgb, depth, acc = rend(planes, d['obs_img_all'][:, 0], obs_feat, sp, None, spd, dec, d['ray_o_all'][:, 0], d['ray_d_all'][:, 0],
                           d['near_all'][:, 0], d['far_all'][:, 0], d, opts)
    assert rgb.requires_grad and acc.requires_grad and not depth.requires_grad and rend.last['bwd']['clamp_mode'] == 'softplus'
    loss = O.stub_loss(rgb[0], acc[0, :, 0])
    assert abs(float(loss.detach()) - float(ref['loss'])) < 1e-4 * float(ref['loss']), (float(loss.detach()), float(ref['loss']))
    loss.backward()
    grads = {'input.planes': planes.grad, 'input.obs_feat': obs_feat.grad, 'input.vertex_feat': vfeat.grad}
    for mod, pre in ((rend, 'renderer.'), (dec, 'decoder.')):
        grads.update({pre + n: p.grad for n, p in mod.named_parameters() if p.grad is not None})
    names = [k for k in ref.files if k not in ('loss', 'ref_cpu_seconds')]
    assert set(names) == set(grads), set(names) ^ set(grads)
    worst = [0.0, 0.0]
    for k in names:
        ours, r = O.grad_fingerprint(G.plain(grads[k].float())), ref[k]
        en, ev = abs(ours[2] - r[2]) / (r[2] + 1e-30), np.linalg.norm(ours[3:] - r[3:]) / (np.linalg.norm(r[3:]) + 1e-30)
        worst = [max(worst[0], en), max(worst[1], ev)]
        assert en < 1e-2, (k, ours[2], r[2])
        assert ev < 5e-2, (k, ev)
    print(f'softplus gradients vs the reference golden: worst norm error {worst[0]:.3e}, worst fingerprint error {worst[1]:.3e}')
    relu = np.load(os.path.join(G.GOLDEN, f'grad_{cfg}.npz'))
    assert abs(float(relu['loss']) - float(ref['loss'])) > 2e-4 * float(ref['loss'])            # (the loss check above tells the two modes' frames apart)


def check_abi():
    """The new entry point is exported and declared; a mode bit nobody defined is an argument error before anything is launched (the buffers
    are far too small for a launch to survive, and stay untouched); a clamp mode nobody defined fails as the reference's marcher does."""
    from sherf_amd.ray_marcher import MipRayMarcher2
    assert 'sherf_composite_dense_bwd' in _lib.parse_header()
    l = _lib.lib()
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), 'sherf_composite_dense_bwd')
    assert (_lib.COMPOSITE_WHITE_BACK, _lib.COMPOSITE_SOFTPLUS) == (1, 2) and _lib.composite_bits(True, 'softplus') == 3
    # (sizes and buffers that even a launch would survive: one ray, two samples, no compact sample -- a launch would overwrite the 3.0s)
    one, zero = _dev(np.full(8, 3.0, np.float32)), _dev(np.zeros(8, np.int32))
    p, z = ctypes.c_void_p(one.data_ptr()), ctypes.c_void_p(zero.data_ptr())
    for bits in (4, 8, 1 << 16, -1):
        assert l.sherf_composite_dense(p, p, p, p, 1, 2, bits, p, p, p, p, None) == -1 and b'bad argument' in l.sherf_last_error()
        assert l.sherf_composite_dense_bwd(p, p, p, p, 1, 2, bits, p, p, p, p, p, p, None) == -1
        assert l.sherf_composite_compact(z, z, z, z, p, p, p, p, 1, 2, bits, p, p, p, None) == -1
        assert l.sherf_composite_compact_cap(z, z, z, z, p, p, p, p, 1, 2, bits, 2, p, p, p, None) == -1
        assert l.sherf_composite_compact_bwd(z, z, z, p, p, p, p, 1, 2, bits, p, p, p, None) == -1
    fr = _lib.Frame()
    fr.white_back = 4
    lv = (_lib.VoxLevel * 3)()
    assert l.sherf_render_frame(ctypes.byref(fr), 3, lv, None, ctypes.c_void_p(8), None) == -1 and b'white_back' in l.sherf_last_error()
    assert bool((G.plain(one) == 3.0).all()) and bool((G.plain(zero) == 0).all())
    x = _dev(np.zeros((1, 4, 3, 3), np.float32))
    with pytest.raises(AssertionError, match='clamp_mode'):
        MipRayMarcher2()(x, x[..., :1], x[..., :1], x[:, :, 0], dict(clamp_mode='tanh', white_back=False))
    with pytest.raises(AssertionError, match='clamp_mode'):
        G.hip_render('tiny', options=dict(clamp_mode='tanh'))


# ---- the host build --------------------------------------------------------------------------------------------------------
def test_dense_marcher_softplus_forward(cpu_product):
    check_dense_forward()


def test_dense_marcher_backward_both_modes(cpu_product):
    check_dense_backward()


def test_rejected_samples_skip_exactly_under_softplus(cpu_product):
    check_rejected_samples_skip_exactly()


def test_frame_under_softplus(cpu_product):
    check_frame()


def test_whole_chain_backward_under_softplus(cpu_product, monkeypatch):
    monkeypatch.setattr(torch.Tensor, 'is_cuda', property(lambda self: True))
    check_whole_chain_backward()


def test_softplus_abi(cpu_product):
    check_abi()
