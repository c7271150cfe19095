"""Reuse of the encoded observation across the frames of a camera / pose sweep (rendering option `reuse_observation`, SHERF_FRAME_REUSE_OBSERVATION,
TriPlaneGenerator's cache_observation / use_cached_observation) on the HOST build of the unchanged kernel sources (tests/hipcpu): the `check_*`
bodies below are shared with tests/test_gpu_observation_cache.py, which runs them on the MI355X.

Scenes: synthdata.make_input_data with another `theta_tgt` keeps the observation and moves the target camera; the `_ri` weights.  The frames of a
sweep are issued back to back on worst-case token buffers (no host wait anywhere in a frame) and compared only after the last one, so that a
missing stream ordering between an encoding frame and the frames that reuse its tables would show.

1. camera sweeps bit-identical to the same sweep without the option, with the native counters; 2. a pose sweep; 3. a reused frame against the
unmodified reference's golden image; 4. everything that must invalidate; 5. BatchNorm running statistics; 6. grad-recorded forwards ignore the
option; 7. two-phase frames; 8. the generator's cache; 9. the ABI."""
import ctypes
import os

import numpy as np
import pytest
import torch

from oracle import sherf_oracle as O
from synthdata import fixtures, synth
from sherf_amd import _lib
from tests import gpu_common as G
from tests import test_hipcpu_branch_backward as B
from tests import test_hipcpu_osg as OSG
from tests.test_hipcpu_frame import cpu_product          # noqa: F401  (the host builds behind sherf_amd._lib, CPU tensors)

THETAS = (1.3, 0.4, 2.6)
TARGET_KEYS = ('params', 'vertices', 'ray_o_all', 'ray_d_all', 'near_all', 'far_all', 'mask_at_box_all')
EINVAL = -1


def _sync():
    if not G.CPU_SHIM:
        torch.cuda.synchronize()


# ---- one observation, many targets ----------------------------------------------------------------------------------------------------------
class Observation:
    """The device tensors of a configuration's observation, built ONCE: every frame of a sweep hands the renderer these very objects (its key is on
    identity, address and version).  `target()` gives an input_data dict whose target side (pose, vertices, rays, depth range) is new and whose
    observation side is this object's."""

    def __init__(self, cfg):
        from sherf_amd.voxel import SparseConvTensor
        self.cfg, self.fx = cfg, G.fixture(cfg)
        fx = self.fx
        self.d0 = G.to_cuda(fx['input_data'])
        self.planes, self.feat, self.img = G.to_cuda(fx['planes']), G.to_cuda(fx['obs_feat']), self.d0['obs_img_all'][:, 0]
        # the voxelisation the oracle (and so the golden image) uses: _render_from_fixture's own three calls
        d = fixtures.to_torch(fx['input_data'])
        op = d['obs_params']
        obs_s = torch.matmul(d['obs_vertices'].view(-1, 3) - op['Th'].view(1, 3), op['R'].view(3, 3))
        _, ovid = O.nearest_vertex(obs_s, obs_s)
        can, _ = O.target_to_canonical(O.smpl_tensors(fx['smpl']), op, d['t_params'], obs_s, obs_s, None, ovid)
        spi = O.prepare_sp_input(d['t_vertices'].view(-1, 3), can)
        self.sp = SparseConvTensor(G.to_cuda(fx['vertex_feat']), G.dev_tensor(spi['coord']), spi['out_sh'], 1)
        self.spi = dict(coord=self.sp.indices, out_sh=spi['out_sh'], batch_size=1, bounds=G.dev_tensor(spi['bounds'])[None])
        self._targets = {}

    def target(self, theta=None, pose_seed=None):
        c = self.fx['cfg']
        theta = c['theta_tgt'] if theta is None else theta
        key = (theta, pose_seed)
        if key not in self._targets:
            if theta == c['theta_tgt'] and pose_seed is None:
                d = self.d0                                      # the fixture's own frame (what the goldens hold)
            else:
                other = synth.make_input_data(self.fx['smpl'], H=c['H'], W=c['W'], seed=1 if pose_seed is None else pose_seed, theta_tgt=theta,
                                              theta_obs=c['theta_obs'], novel_pose=c['novel_pose'] or pose_seed is not None, fill=c.get('fill', 2.2))
                d = dict(self.d0)
                d.update({k: G.to_cuda(other[k]) for k in TARGET_KEYS})
            self._targets[key] = d
        return self._targets[key]


_OBS = {}


def observation(cfg, fresh=False):
    key = (G.CPU_SHIM, cfg)
    if fresh or key not in _OBS:
        _OBS[key] = Observation(cfg)
    return _OBS[key]


def modules(kind='nerf', variant='ri'):
    """A fresh (renderer, decoder) pair in train mode: a sweep moves running statistics and leaves keys in the workspace."""
    if kind == 'osg':
        return OSG.osg_modules('f16x3', True, (True, True, True), fresh=True)
    return G._hip_modules.__wrapped__('f16x3', variant, True, (True, True, True))


def render(pair, obs, d, reuse, **options):
    """One frame, not waited for -> device tensors (rgb, depth, acc)."""
    rend, dec = pair
    opts = dict(obs.fx['options'], mlp_precision='f16x3', token_capacity='worst', reuse_observation=reuse)
    opts.update(options)
    with torch.no_grad():
        return rend(obs.planes, obs.img, obs.feat, obs.sp, None, obs.spi, dec, d['ray_o_all'][:, 0], d['ray_d_all'][:, 0], d['near_all'][:, 0],
                    d['far_all'][:, 0], d, opts)


def sweep(pair, obs, targets, reuse, **options):
    """The frames of `targets` back to back, then one wait -> ([frame], native stats delta, [observation_reused per frame])."""
    n0 = _lib.frame_observation_stats()
    frames, flags = [], []
    for d in targets:
        frames.append(render(pair, obs, d, reuse, **options))
        flags.append(pair[0].last['observation_reused'])
    _sync()
    n1 = _lib.frame_observation_stats()
    return frames, (n1[0] - n0[0], n1[1] - n0[1]), flags


def assert_same_frames(a, b, label):
    for i, (fa, fb) in enumerate(zip(a, b)):
        for name, x, y in zip(('rgb', 'depth', 'acc'), fa, fb):
            assert torch.equal(G.plain(x), G.plain(y)), (label, i, name)


# ---- 1. camera sweep ------------------------------------------------------------------------------------------------------------------------
SWEEPS = {'tiny_ri': ('tiny_ri', 'nerf'), 'tiny_nv': ('tiny_nv_ri', 'nerf'), 'tiny_ri_osg': ('tiny_ri', 'osg')}


def check_camera_sweep(case, aux):
    cfg, kind = SWEEPS[case]
    obs = observation(cfg)
    targets = [obs.target(t) for t in THETAS]
    on, off = modules(kind), modules(kind)
    f_on, n_on, r_on = sweep(on, obs, targets, True, aux_stream=aux)
    f_off, n_off, r_off = sweep(off, obs, targets, False, aux_stream=aux)
    assert n_on == (1, 2) and r_on == [False, True, True], (n_on, r_on)
    assert n_off == (3, 0) and r_off == [False, False, False], (n_off, r_off)
    assert on[0].observation_stats() == (1, 2) and off[0].observation_stats() == (3, 0)
    assert_same_frames(f_on, f_off, (case, aux))
    assert float(G.plain(f_on[1][2]).max()) > 0.5 and not torch.equal(G.plain(f_on[0][0]), G.plain(f_on[1][0]))       # (frames with a subject, not one frame thrice)
    return on, off


# ---- 2. pose sweep --------------------------------------------------------------------------------------------------------------------------
def check_pose_sweep():
    """Same observation, two other target poses (new params, vertices, rays, near / far) on the token buffers the renderer sizes itself."""
    obs = observation('tiny_ri')
    targets = [obs.target(0.9, pose_seed=2), obs.target(0.9, pose_seed=3)]
    assert not torch.equal(G.plain(targets[0]['params']['poses']), G.plain(targets[1]['params']['poses']))
    on, off = modules(), modules()
    f_on, n_on, r_on = sweep(on, obs, targets, True, token_capacity='auto')
    f_off, n_off, _ = sweep(off, obs, targets, False, token_capacity='auto')
    assert n_on == (1, 1) and r_on == [False, True] and n_off == (2, 0), (n_on, r_on, n_off)
    assert_same_frames(f_on, f_off, 'pose sweep')
    assert not torch.equal(G.plain(f_on[0][0]), G.plain(f_on[1][0]))


# ---- 3. pinned to the reference -------------------------------------------------------------------------------------------------------------
def check_reused_frame_against_golden(cfg):
    """theta = 1.3 encodes, the fixture's own frame (theta = 0.4) reuses -- and meets tests/golden/renderer_<cfg>.npz at what
    tests/test_gpu_parity.py::test_end_to_end_vs_oracle_and_reference_golden and tests/test_hipcpu_frame.py::test_stage_by_stage_parity apply to a
    frame against its golden: rgb and acc within 1e-3 of the image's largest entry, PSNR above 60 dB, |dPSNR| <= 0.05 dB against the fixed target."""
    obs = observation(cfg)
    assert obs.fx['cfg']['theta_tgt'] == 0.4
    g = np.load(os.path.join(G.GOLDEN, f'renderer_{cfg}.npz'))
    on = modules()
    frames, n, flags = sweep(on, obs, [obs.target(1.3), obs.target()], True, token_capacity='auto')
    assert n == (1, 1) and flags == [False, True], (n, flags)
    rgb, acc = G.plain(frames[1][0][0]), G.plain(frames[1][2][0, :, 0])
    ref_rgb = torch.from_numpy(g['rgb'])
    e_rgb, e_acc, psnr = G.rel(rgb, ref_rgb), G.rel(acc, torch.from_numpy(g['acc'][:, 0])), O.psnr(rgb, ref_rgb)
    print(f'{cfg}: reused frame vs the reference: rgb {e_rgb:.2e}, acc {e_acc:.2e}, PSNR {psnr:.1f} dB')
    assert e_rgb < 1e-3 and e_acc < 1e-3 and psnr > 60.0
    target = torch.from_numpy(np.random.RandomState(5).uniform(-1, 1, tuple(ref_rgb.shape)).astype(np.float32))
    assert abs(O.psnr(rgb, target) - O.psnr(ref_rgb, target)) <= 0.05


# ---- 4. invalidation ------------------------------------------------------------------------------------------------------------------------
def fold_sources(rend, dec):
    """Which parameters feed a fold (Wa_t / Wb_t / the fold matrices / tok_bias), read off ImportanceRenderer._weights: every parameter is nudged in
    turn and the packed tensors are compared.  -> the names ('renderer.' / 'decoder.' prefixed) whose nudge moved one of them."""
    dev = next(rend.parameters()).device
    packed = lambda: [G.plain(t).clone() for t in (lambda wc: [wc['Wa_t'], wc['Wb_t'], wc['tok_bias']] + list(wc['fold']))(rend._weights(dec, dev, 'f16x3'))]
    base, out = packed(), []
    named = [('renderer.' + n, p) for n, p in rend.named_parameters() if not n.startswith('encoder_3d.')] + [('decoder.' + n, p) for n, p in dec.named_parameters()]
    for name, p in named:
        with torch.no_grad():
            keep = p.detach().clone()
            p.view(-1)[:1].add_(0.25)
            moved = any(not torch.equal(a, b) for a, b in zip(base, packed()))
            p.copy_(keep)
        if moved:
            out.append(name)
    return out


def check_invalidation():
    """Between two frames of a sweep each of the changes below yields a miss and the image of the renderer that never reuses; every miss records its
    own key, so the next change is again applied to a renderer that would otherwise reuse.  The two renderers are changed alike."""
    obs = observation('tiny_ri', fresh=True)                    # (its image and planes are edited below)
    on, off = modules(), modules()
    other = modules(variant='seeded')                           # a second renderer with other weights, through `on`'s workspaces
    state = dict(options={}, k=0)
    thetas = (1.3, 0.4, 2.6, 0.9, 2.0)

    def frame_pair(expect_reused, label):
        d = obs.target(thetas[state['k'] % len(thetas)])
        state['k'] += 1
        a, b = render(on, obs, d, True, **state['options']), render(off, obs, d, False, **state['options'])
        assert on[0].last['observation_reused'] is expect_reused, (label, 'reused' if not expect_reused else 'missed')
        assert not off[0].last['observation_reused']
        _sync()
        assert_same_frames([a], [b], label)

    def nudge(get):
        for pair in (on, off):
            with torch.no_grad():
                get(*pair).view(-1)[3:7].add_(0.05)             # (an in-place update: the version counter moves)

    # no decoder parameter feeds a fold: the folds are built from conv1d_projection / conv1d_reprojection alone
    feeds = fold_sources(*on)
    assert sorted(feeds) == ['renderer.conv1d_projection.bias', 'renderer.conv1d_projection.weight', 'renderer.conv1d_reprojection.bias',
                             'renderer.conv1d_reprojection.weight'], feeds

    def edit_image():
        obs.img.mul_(0.5)

    def new_planes():
        obs.planes = obs.planes * 1.25

    def table_precision():
        state['options'] = dict(table_precision='f16')

    def eval_mode():
        on[0].encoder_3d.eval(); off[0].encoder_3d.eval()

    def second_renderer():
        other[0]._ws = on[0]._ws
        render(other, obs, obs.target(0.4), True)
        assert not other[0].last['observation_reused']          # (other weights: `on`'s tables are not its own)

    changes = [('in-place edit of obs_input_img', edit_image), ('a new planes tensor', new_planes),
               ('conv1d_reprojection weight', lambda: nudge(lambda r, d: r.conv1d_reprojection.weight)),
               ('encoder_3d conv weight', lambda: nudge(lambda r, d: r.encoder_3d.conv1[0].weight)),
               ('conv1d_projection weight (feeds the voxel folds)', lambda: nudge(lambda r, d: r.conv1d_projection.weight)),
               # (feeds no fold -- but the weight cache is keyed on the decoder too and rebuilds the fold matrices: the frame misses all the same)
               ('decoder weight', lambda: nudge(lambda r, d: d.pts_linears[0].weight)),
               ('table_precision', table_precision), ('encoder_3d.eval()', eval_mode), ('a frame of a second renderer through the workspace', second_renderer)]
    frame_pair(False, 'first frame')
    frame_pair(True, 'second frame')
    for label, change in changes:
        change()
        frame_pair(False, label)              # (it would have reused but for the change: the frame before it recorded its key)
    frame_pair(True, 'the frame after the last change')


# ---- 5. running statistics ------------------------------------------------------------------------------------------------------------------
def _buffers(rend):
    return {k: G.plain(v).clone() for k, v in rend.encoder_3d.named_buffers()}


def _same_bits(a, b):
    return a.dtype == b.dtype and torch.equal(a.reshape(-1).contiguous().view(torch.uint8), b.reshape(-1).contiguous().view(torch.uint8))


def check_running_statistics():
    """Train mode: after the three-frame sweep every encoder_3d buffer is bit-equal with and without the option (and has moved: three updates).
    Eval mode: untouched in both."""
    on, off = check_camera_sweep('tiny_ri', True)
    b_on, b_off = _buffers(on[0]), _buffers(off[0])
    fresh = _buffers(modules()[0])
    assert set(b_on) == set(b_off) and len(b_on) >= 39
    for k in b_on:
        assert _same_bits(b_on[k], b_off[k]), k
    tracked = [k for k in b_on if k.endswith('num_batches_tracked') and int(fresh[k]) != int(b_on[k])]
    assert tracked and all(int(b_on[k]) == int(fresh[k]) + 3 for k in tracked)
    assert any(not _same_bits(b_on[k], fresh[k]) for k in b_on if k.endswith('running_mean'))
    obs = observation('tiny_ri')
    targets = [obs.target(t) for t in THETAS]
    for pair in (on, off):
        pair[0].eval(); pair[1].eval()
    f_on, n_on, _ = sweep(on, obs, targets, True)
    f_off, n_off, _ = sweep(off, obs, targets, False)
    assert n_on == (1, 2) and n_off == (3, 0)
    assert_same_frames(f_on, f_off, 'eval mode')
    for pair, before in ((on, b_on), (off, b_off)):
        after = _buffers(pair[0])
        for k in before:
            assert _same_bits(after[k], before[k]), k


# ---- 6. autograd ----------------------------------------------------------------------------------------------------------------------------
def check_autograd_ignores_the_option():
    """A no-grad frame records the key; the grad-recorded frame on the very same input objects encodes all the same (native counters, last[...]),
    and its loss and gradients are those of the renderer without the option: the loss to the bit (the forward is deterministic), the gradients within
    1e-4 of their norm (the bound tests/test_hipcpu_branch_backward.py::check_degenerate_switches gives two runs of the same kernels on the same
    inputs: fp32 atomics in another order)."""
    from sherf_amd.voxel import SparseConvTensor
    obs = observation('tiny_ri')
    d = obs.target()
    out = {}
    for name, reuse in (('on', True), ('off', False)):
        rend, dec = pair = modules()
        leaf = lambda t: G.dev_tensor(G.plain(t).clone()).requires_grad_(True)
        leaves = dict(planes=leaf(obs.planes), feat=leaf(obs.feat), vfeat=leaf(obs.sp.features))
        sp = SparseConvTensor(leaves['vfeat'], obs.sp.indices, obs.sp.spatial_shape, 1)
        opts = dict(obs.fx['options'], mlp_precision='f16x3', reuse_observation=reuse)
        call = lambda: rend(leaves['planes'], obs.img, leaves['feat'], sp, None, obs.spi, dec, d['ray_o_all'][:, 0], d['ray_d_all'][:, 0],
                            d['near_all'][:, 0], d['far_all'][:, 0], d, opts)
        with torch.no_grad():
            call()
            call()
        assert rend.last['observation_reused'] is reuse          # (the same objects: without autograd the second frame reuses)
        n0 = _lib.frame_observation_stats()
        with B.autograd_on(rend, 'nerf'), torch.enable_grad():
            rgb, depth, acc = call()
            assert rgb.requires_grad and rend.last['observation_reused'] is False
            loss = O.stub_loss(rgb[0], acc[0, :, 0])
            loss.backward()
            _sync()
        n1 = _lib.frame_observation_stats()
        assert (n1[0] - n0[0], n1[1] - n0[1]) == (1, 0)
        grads = {k: G.plain(v.grad).double() for k, v in leaves.items()}
        grads.update({'renderer.' + k: G.plain(p.grad).double() for k, p in rend.named_parameters() if p.grad is not None})
        grads.update({'decoder.' + k: G.plain(p.grad).double() for k, p in dec.named_parameters() if p.grad is not None})
        out[name] = (float(loss.detach()), grads)
        with torch.no_grad():
            call()
        assert rend.last['observation_reused'] is False          # (and nothing a recorded frame left is reused behind it)
    assert out['on'][0] == out['off'][0]
    assert set(out['on'][1]) == set(out['off'][1]) and len(out['on'][1]) > 60
    for k, a in out['off'][1].items():
        e = float((out['on'][1][k] - a).norm() / (a.norm() + 1e-30))
        assert e < 1e-4, (k, e)


# ---- 7. two-phase frames --------------------------------------------------------------------------------------------------------------------
def check_two_phase_frames():
    """depth_range given (phase 1, the range written into the counters, phase 2) with density_noise = 0, under reuse: bit-identical to uncached."""
    obs = observation('tiny_ri')
    targets = [obs.target(t) for t in THETAS]
    on, off = modules(), modules()
    calls = []
    with B.recorded_calls() as calls:
        f_on, n_on, r_on = sweep(on, obs, targets, True, depth_range=[2.0, 3.5], density_noise=0)
    assert [c[1][1] for c in calls if c[0] == 'sherf_render_frame'] == [1, 2, 1, 2, 1, 2]
    f_off, n_off, _ = sweep(off, obs, targets, False, depth_range=[2.0, 3.5], density_noise=0)
    assert n_on == (1, 2) and r_on == [False, True, True] and n_off == (3, 0)
    assert_same_frames(f_on, f_off, 'two-phase')
    plain, _, _ = sweep(off, obs, targets[:1], False)
    assert not torch.equal(G.plain(plain[0][1]), G.plain(f_off[0][1]))        # (the supplied range does reach the depth image)


# ---- 8. the generator -----------------------------------------------------------------------------------------------------------------------
GLUE_CALLS = ('sherf_vertex_features', 'sherf_voxelize', 'sherf_smpl_bones', 'sherf_smpl_offsets', 'sherf_smpl_t2c_table')


def generator():
    """TriPlaneGenerator with its own producers at a narrow width (the shape of tests/test_hipcpu_frame.py::check_whole_generator), the `_ri` renderer."""
    from sherf_amd.triplane import TriPlaneGenerator
    fx = G.fixture('tiny_ri')
    rend, dec = modules()
    torch.manual_seed(0)
    gen = TriPlaneGenerator(512, 0, 48, True, True, True, True, True, img_resolution=32, img_channels=3, mapping_kwargs=dict(num_layers=2),
                            rendering_kwargs=dict(fx['options'], mlp_precision='f16x3', token_capacity='worst'), smpl=G.smpl(), channel_base=512,
                            channel_max=16, num_fp16_res=0, conv_clamp=None, fused_modconv_default='inference_only')
    gen.renderer, gen.decoder = rend, dec
    gen.graph_producers = False
    gen = G.dev_module(gen)
    gen.eval(); rend.train(); dec.train()
    return gen


def check_generator_cache():
    """forward(cache_observation=True), then forward(use_cached_observation=True) on other rays: the images of plain forward calls to the bit, no producer,
    glue or voxelisation call on the served frame; a changed observation image recomputes; gradient recording disables both; snapshots drop the cache.
    (Bit-equality with a PLAIN call needs the plain call itself to be reproducible: on the device the library's default convolution algorithms are not
    -- ResNet-18's code moves by 1e-7 from run to run -- so the test selects the deterministic ones, as `torch.backends.cudnn.deterministic` does.)"""
    was = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True
    try:
        _check_generator_cache()
    finally:
        torch.backends.cudnn.deterministic = was


def _check_generator_cache():
    obs = observation('tiny_ri', fresh=True)
    gen = generator()
    c0 = G.dev_tensor(torch.zeros(1, 25))
    d1, d2, d3 = obs.target(), obs.target(1.3), obs.target(2.6)
    counts = {}
    hooks = []
    for name, m in (('encoder_2d', gen.encoder_2d), ('mapping', gen.backbone.mapping), ('backbone.synthesis', gen.backbone.synthesis),
                    ('encoder_2d_feature', gen.encoder_2d_feature)):
        hooks.append(m.register_forward_hook(lambda mod, a, o, name=name: counts.__setitem__(name, counts.get(name, 0) + 1)))
    fwd = lambda d, **kw: gen(d, None, c0, use_sr_module=False, test_flag=True, noise_mode='const', **kw)
    keys = ('image', 'image_raw', 'image_depth', 'weights_image')
    try:
        with torch.no_grad():
            plain1, plain2 = fwd(d1), fwd(d2)
            assert counts == {'encoder_2d': 2, 'mapping': 2, 'backbone.synthesis': 2, 'encoder_2d_feature': 2}
            assert gen.observation_cache_stats == dict(hits=0, misses=0) and gen.renderer.observation_stats() == (2, 0)
            counts.clear()
            filled = fwd(d1, cache_observation=True)
            assert counts == {'encoder_2d': 1, 'mapping': 1, 'backbone.synthesis': 1, 'encoder_2d_feature': 1}
            oc = gen._obs_cache
            assert set(oc) >= {'ws', 'planes', 'obs_input_feature', 'vertex_features', 'mask', 'canonical_obs_vertices', 'sp_input', 'sp'}
            counts.clear()
            n0 = _lib.frame_observation_stats()
            with B.recorded_calls() as calls:
                served = fwd(d2, use_cached_observation=True)
            _sync()
            n1 = _lib.frame_observation_stats()
            names = [c[0] for c in calls]
            assert counts == {}, counts                                      # no producer ran
            assert not [n for n in names if n in GLUE_CALLS], names          # nor the glue, nor the voxelisation
            assert names.count('sherf_render_frame') == 1 and (n1[0] - n0[0], n1[1] - n0[1]) == (0, 1)
            assert gen.renderer.last['observation_reused'] and gen.observation_cache_stats == dict(hits=1, misses=0)
            for k in keys:
                assert torch.equal(G.plain(filled[k]), G.plain(plain1[k])) and torch.equal(G.plain(served[k]), G.plain(plain2[k])), k
            assert not torch.equal(G.plain(plain1['image_raw']), G.plain(plain2['image_raw']))
            # a changed observation image: recomputed (and the cache refilled), not served
            d1['obs_img_all'].mul_(0.8)
            counts.clear()
            changed = fwd(d3, use_cached_observation=True)
            assert counts == {'encoder_2d': 1, 'mapping': 1, 'backbone.synthesis': 1, 'encoder_2d_feature': 1}
            assert gen.observation_cache_stats == dict(hits=1, misses=1) and not gen.renderer.last['observation_reused']
            again = fwd(d2, use_cached_observation=True)
            assert gen.observation_cache_stats == dict(hits=2, misses=1) and gen.renderer.last['observation_reused']
            plain3, plain2b = fwd(d3), fwd(d2)
            for k in keys:
                assert torch.equal(G.plain(changed[k]), G.plain(plain3[k])) and torch.equal(G.plain(again[k]), G.plain(plain2b[k])), k
            assert not torch.equal(G.plain(plain2b['image_raw']), G.plain(plain2['image_raw']))
        # gradient recording disables both the fill and the use
        gen.__dict__.pop('_obs_cache')
        before = gen.observation_cache_stats
        with torch.enable_grad():
            fwd(d2, cache_observation=True, use_cached_observation=True)
        assert '_obs_cache' not in gen.__dict__ and gen.observation_cache_stats == before
        # and the cache does not travel with a snapshot
        with torch.no_grad():
            fwd(d2, cache_observation=True)
        assert '_obs_cache' in gen.__dict__ and '_obs_cache' not in gen.__getstate__()
    finally:
        for h in hooks:
            h.remove()


# ---- 9. ABI ---------------------------------------------------------------------------------------------------------------------------------
def check_abi():
    """The header declares the flag and sherf_frame_observation_stats, the library exports the function; a short stats array and a reusing frame
    whose `levels` are not its plan's are argument errors before anything is launched or counted."""
    src = open(_lib.HEADER).read()
    assert '#define SHERF_FRAME_REUSE_OBSERVATION 256' in src and _lib.FRAME_REUSE_OBSERVATION == 256
    assert 'sherf_frame_observation_stats' in _lib.parse_header(_lib.HEADER)
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), 'sherf_frame_observation_stats')
    l = _lib.lib()
    s = (ctypes.c_int64 * 2)()
    assert l.sherf_frame_observation_stats(s, 1) == EINVAL and l.sherf_frame_observation_stats(None, 2) == EINVAL
    assert l.sherf_frame_observation_stats(s, 2) == 0 and s[0] >= 0 and s[1] >= 0
    n0 = _lib.frame_observation_stats()
    fr, plan, lv = _lib.Frame(), _lib.SvoxPlan(), (_lib.VoxLevel * 3)()
    fr.flags, fr.vox_plan = _lib.FRAME_REUSE_OBSERVATION, ctypes.addressof(plan)
    fr.planes_f = fr.feat_f = fr.img4 = 64
    for phase in (1, 3):
        assert l.sherf_render_frame(ctypes.byref(fr), phase, lv, None, ctypes.c_void_p(8), None) == EINVAL and b'bad argument' in l.sherf_last_error()
    assert _lib.frame_observation_stats() == n0


# ---- the host build -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('aux', (True, False))
@pytest.mark.parametrize('case', list(SWEEPS))
def test_camera_sweep_is_bit_identical(cpu_product, case, aux):
    check_camera_sweep(case, aux)


def test_pose_sweep_is_bit_identical(cpu_product):
    check_pose_sweep()


def test_reused_frame_against_reference_golden(cpu_product):
    check_reused_frame_against_golden('tiny_ri')


def test_every_change_of_the_observation_misses(cpu_product):
    check_invalidation()


def test_running_statistics_evolve_as_without_reuse(cpu_product):
    check_running_statistics()


def test_grad_recorded_forward_ignores_the_option(cpu_product):
    check_autograd_ignores_the_option()


def test_two_phase_frames_reuse(cpu_product):
    check_two_phase_frames()


def test_generator_caches_the_observation_side(cpu_product, monkeypatch):
    monkeypatch.setattr(torch.Tensor, 'is_cuda', property(lambda self: True))       # module parameters are "device" tensors too
    check_generator_cache()


def test_observation_abi(cpu_product):
    check_abi()
