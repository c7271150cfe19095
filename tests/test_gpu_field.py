"""The field query (ImportanceRenderer.query_points, TriPlaneGenerator.sample / sample_mixed, sherf_amd.field.density_grid; csrc/field.hip) on the MI355X.
The `check_*` bodies are shared with tests/test_hipcpu_field.py, which runs them on the host build of the unchanged kernel sources.

Pinned to the UNMODIFIED reference through goldens that already exist: a frame's samples handed in as points (`tiny_ri`: 1024 rays x 16 samples, 628 valid) must
give the recorded mask bit for bit and the recorded per-sample sigma / rgb at the tolerance tests/test_gpu_parity.py::test_per_sample_sigma_rgb applies to the
frame path (restated below), and composited by MipRayMarcher2 the recorded image.  Against the frame path itself the query is bit-identical."""
import ctypes
import functools
import os

import numpy as np
import pytest
import torch

from oracle import fixtures, sherf_oracle as O
from sherf_amd import _lib
from tests import gpu_common as G

gpu = pytest.mark.gpu
CFG = 'tiny_ri'
# tests/test_gpu_parity.py::test_per_sample_sigma_rgb: (activated sigma: max error relative to the largest reference value, rgb: max absolute error) per precision
PER_SAMPLE_TOL = {'f16x3': (1e-3, 1e-3), 'bf16': (5e-2, 5e-2)}
#        golden                    decoder  branches             precision
CASES = {'nerf-f16x3':  ('renderer_tiny_ri',      'nerf', (True, True, True),  'f16x3'),
         'nerf-bf16':   ('renderer_tiny_ri',      'nerf', (True, True, True),  'bf16'),
         'osg':         ('renderer_tiny_ri_osg',  'osg',  (True, True, True),  'f16x3'),
         'f101':        ('renderer_tiny_ri_f101', 'nerf', (True, False, True), 'f16x3')}


def golden(name='renderer_tiny_ri'):
    return np.load(os.path.join(G.GOLDEN, name + '.npz'))


@functools.lru_cache(None)
def _ray_samples():
    """The frame's sample positions as the reference forms them (renderer.py:304: origins + depths * directions in torch fp32; depths: math_utils.linspace as
    oracle.sherf_oracle.depths states it) and the rays' directions repeated per sample -> (points [R*S,3], dirs [R*S,3], depths [R,S], ray dirs [R,3])."""
    fx = G.fixture(CFG)
    d = fx['input_data']
    o, rd = torch.from_numpy(d['ray_o_all'][0, 0]), torch.from_numpy(d['ray_d_all'][0, 0])
    t = O.depths(torch.from_numpy(d['near_all'][0, 0]).reshape(-1), torch.from_numpy(d['far_all'][0, 0]).reshape(-1), fx['options']['depth_resolution'])
    pts = o.unsqueeze(-2) + t.unsqueeze(-1) * rd.unsqueeze(-2)
    return pts.reshape(-1, 3).contiguous(), rd.unsqueeze(-2).expand_as(pts).reshape(-1, 3).contiguous(), t, rd


def _golden_mask():
    g = golden()
    return torch.from_numpy(np.unpackbits(g['mask_bits'])[:int(g['n_samples'])].astype(bool))


def _sp_input():
    g = golden()          # the reference's own voxelisation of the fixture (the same for every golden of `tiny_ri`)
    return dict(coord=torch.from_numpy(g['sp_coord']), out_sh=[int(v) for v in g['sp_out_sh']], bounds=torch.from_numpy(g['sp_bounds'][0]))


_DEV = {}


def _inputs():
    """The fixture's tensors on the device, ONE set per build (host / device): frames and queries on the same objects."""
    if G.CPU_SHIM not in _DEV:
        from sherf_amd.voxel import SparseConvTensor
        fx, spi = G.fixture(CFG), _sp_input()
        d = G.to_cuda(fx['input_data'])
        sp = SparseConvTensor(G.to_cuda(fx['vertex_feat']), G.dev_tensor(spi['coord']), spi['out_sh'], 1)
        sp_input = dict(coord=G.dev_tensor(spi['coord']), out_sh=spi['out_sh'], batch_size=1, bounds=G.dev_tensor(spi['bounds'])[None])
        _DEV[G.CPU_SHIM] = dict(d=d, sp=sp, sp_input=sp_input, planes=G.to_cuda(fx['planes']), obs_feat=G.to_cuda(fx['obs_feat']),
                                obs_img=d['obs_img_all'][:, 0])          # (one view object: the renderer keys its observation on identity)
    return _DEV[G.CPU_SHIM]


def _modules(precision='f16x3', decoder='nerf', branches=(True, True, True)):
    if decoder == 'osg':
        from tests.test_hipcpu_osg import osg_modules
        return osg_modules(precision, True, branches)
    return G.hip_modules(precision, 'ri', True, branches)


def _sync():
    if not G.CPU_SHIM:
        torch.cuda.synchronize()


def query(points, dirs, precision='f16x3', decoder='nerf', branches=(True, True, True), options=None):
    rend, dec = _modules(precision, decoder, branches)
    rend.train(True)
    x = _inputs()
    opts = dict(G.fixture(CFG)['options'], mlp_precision=precision)
    opts.update(options or {})
    out = rend.query_points(x['planes'], x['obs_img'], x['obs_feat'], x['sp'], None, x['sp_input'], dec,
                            G.dev_tensor(points.reshape(1, -1, 3).contiguous()), G.dev_tensor(dirs.reshape(1, -1, 3).contiguous()), x['d'], opts)
    _sync()
    N = points.reshape(-1, 3).shape[0]
    assert out['rgb'].shape == (1, N, 3) and out['sigma'].shape == (1, N, 1) and out['mask'].shape == (1, N) and out['mask'].dtype == torch.bool
    return dict(rgb=G.plain(out['rgb'][0]), sigma=G.plain(out['sigma'][0, :, 0]), mask=G.plain(out['mask'][0]), rend=rend, dec=dec, last=rend.last_query)


def frame(precision='f16x3', options=None):
    """ImportanceRenderer.forward on the same tensor objects (tests.gpu_common.hip_render allocates new ones per call)."""
    rend, dec = _modules(precision)
    rend.train(True)
    x = _inputs()
    d = x['d']
    opts = dict(G.fixture(CFG)['options'], mlp_precision=precision)
    opts.update(options or {})
    with torch.no_grad():
        rgb, depth, acc = rend(x['planes'], x['obs_img'], x['obs_feat'], x['sp'], None, x['sp_input'], dec, d['ray_o_all'][:, 0],
                               d['ray_d_all'][:, 0], d['near_all'][:, 0], d['far_all'][:, 0], d, opts)
    _sync()
    return dict(rgb=G.plain(rgb[0]), depth=G.plain(depth[0, :, 0]), acc=G.plain(acc[0, :, 0]), last=rend.last, rend=rend)


def same(a, b):
    """Bit for bit (NaN-safe, -0.0 != 0.0)."""
    a, b = torch.as_tensor(a), torch.as_tensor(b)
    if a.dtype.is_floating_point:
        return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))
    return torch.equal(a, b)


def same_out(a, b, sel=None):
    pick = (lambda t: t) if sel is None else (lambda t: t[sel])
    return same(a['rgb'], pick(b['rgb'])) and same(a['sigma'], pick(b['sigma'])) and torch.equal(a['mask'], pick(b['mask']))


_FULL = {}


def full(precision='f16x3'):
    """The 16384 ray samples of the fixture queried in one chunk: computed once per build and precision, never modified."""
    key = (G.CPU_SHIM, precision)
    if key not in _FULL:
        pts, dirs, _, _ = _ray_samples()
        _FULL[key] = query(pts, dirs, precision)
    return _FULL[key]


# ---- 1. pinned to the unmodified reference ------------------------------------------------------------------------------------------
def check_reference_golden(case):
    name, decoder, branches, prec = CASES[case]
    g = golden(name)
    pts, dirs, _, _ = _ray_samples()
    q = full(prec) if (decoder, branches) == ('nerf', (True, True, True)) else query(pts, dirs, prec, decoder, branches)
    mask = _golden_mask()
    assert int(g['n_valid']) == int(mask.sum()) == 628
    assert torch.equal(q['mask'], mask)
    sig_ref = torch.relu(torch.from_numpy(g['sample_sigma']))
    e_sig = float((torch.relu(q['sigma'][mask]) - sig_ref).abs().max() / sig_ref.max())
    e_rgb = float((q['rgb'][mask] - torch.from_numpy(g['sample_rgb'])).abs().max())
    print(f'field query {case}: sigma+ rel-to-max err {e_sig:.2e}, rgb max abs err {e_rgb:.2e}')
    tol_sig, tol_rgb = PER_SAMPLE_TOL[prec]
    assert e_sig < tol_sig and e_rgb < tol_rgb, (case, e_sig, e_rgb)
    assert bool((q['sigma'][~mask] == -80.0).all()) and bool((q['rgb'][~mask] == 0.0).all())
    assert q['last']['mlp_precision'] == prec


# ---- 2. same bits as the frame --------------------------------------------------------------------------------------------------------
def check_same_bits_as_frame(prec):
    f = frame(prec)
    ws = f['last']['ws']
    nv = int(ws['counters'][0])
    assert nv == 628
    f_xs, f_out = G.plain(ws['cs_xs'][:nv]).clone(), G.plain(ws['sample_out'][:nv]).clone()
    q = full(prec)
    qws = q['last']['ws']
    assert q['last']['counts'] == [nv]
    assert torch.allclose(G.plain(qws['cs_xs'][:nv]), f_xs, atol=0, rtol=0)                     # the precondition: the same compact inputs
    assert torch.equal(G.plain(qws['cs_idx'][:nv]).long(), torch.nonzero(q['mask'])[:, 0])     # ascending point order == the frame's ray-major order
    assert torch.equal(G.plain(qws['cs_idx'][:nv]), G.plain(ws['cs_idx'][:nv]))
    assert same(q['sigma'][q['mask']], f_out[:, 3]) and same(q['rgb'][q['mask']], f_out[:, :3].contiguous())


# ---- 3. end to end through the dense marcher -----------------------------------------------------------------------------------------
def check_through_the_marcher():
    from sherf_amd.ray_marcher import MipRayMarcher2
    g = golden()
    _, _, t, rd = _ray_samples()
    R, S = t.shape
    q = full('f16x3')
    dv = G.dev_tensor
    rgb, depth, w = MipRayMarcher2()(dv(q['rgb'].view(1, R, S, 3)), dv(q['sigma'].view(1, R, S, 1)), dv(t.reshape(1, R, S, 1).contiguous()),
                                     dv(rd.reshape(1, R, 3).contiguous()), dict(clamp_mode='relu', white_back=False))
    _sync()
    rgb, depth, acc = G.plain(rgb[0]), G.plain(depth[0, :, 0]), G.plain(w[0, :, :, 0]).sum(-1)
    # tests/test_gpu_parity.py::test_end_to_end_vs_oracle_and_reference_golden's bounds on hip_render against this golden
    assert G.rel(rgb, g['rgb']) < 1e-3 and G.rel(acc, g['acc'][:, 0]) < 1e-3
    assert torch.allclose(depth, torch.from_numpy(g['depth'][:, 0]), rtol=1e-3, atol=1e-4)
    assert G.rel(acc, g['weights'].sum(1)) < 1e-3


# ---- 4. per-point indexing --------------------------------------------------------------------------------------------------------------
def check_per_point_indexing():
    pts, dirs, _, _ = _ray_samples()
    ref = full()
    perm = torch.from_numpy(np.random.RandomState(7).permutation(pts.shape[0]))
    q = query(pts[perm], dirs[perm])
    assert same_out(q, ref, perm)
    i = int(torch.nonzero(ref['mask'])[300, 0])
    dup = query(pts[i:i + 1].expand(100, 3), dirs[i:i + 1].expand(100, 3))
    assert bool(dup['mask'].all()) and same_out(dup, ref, torch.full((100,), i, dtype=torch.long))
    # directions are read per POINT: another direction at one valid point moves that point's colour and nothing else
    d2 = dirs.clone()
    d2[i] = torch.tensor([0.0, 1.0, 0.0])
    q2 = query(pts, d2)
    others = torch.arange(pts.shape[0]) != i
    assert same(q2['sigma'], ref['sigma']) and same(q2['rgb'][others], ref['rgb'][others]) and not same(q2['rgb'][i], ref['rgb'][i])


# ---- 5. shapes where the kernels can go wrong --------------------------------------------------------------------------------------------
def check_edge_shapes():
    pts, dirs, _, _ = _ray_samples()
    ref = full()
    valid = torch.nonzero(ref['mask'])[:, 0]
    # N = 1 and around one row: a selection with valid points at its start, its end and across the row boundary
    for n in (1, 63, 64, 65):
        sel = torch.cat([valid[:1], torch.arange(100, 100 + n - 2), valid[7:8]]) if n > 1 else valid[:1]
        q = query(pts[sel], dirs[sel])
        assert same_out(q, ref, sel), n
        assert q['last']['counts'] == [int(ref['mask'][sel].sum())]
    # the posed vertices themselves: every point valid, the token buffers hold exactly the count
    rend = _modules()[0]
    verts = torch.from_numpy(G.fixture(CFG)['input_data']['vertices'][0])
    rend.TOKEN_GRANULE = 1
    try:
        r0 = rend.query_stats()['resizes']
        q = query(verts, dirs[:1].expand_as(verts), options=dict(token_capacity=6890))
        assert q['last']['counts'] == [6890] and q['last']['cap'] == 6890 and rend.query_stats()['resizes'] == r0
        assert bool(q['mask'].all()) and bool(torch.isfinite(q['sigma']).all()) and bool(torch.isfinite(q['rgb']).all()) and bool((q['sigma'] != -80.0).all())
    finally:
        del rend.TOKEN_GRANULE
    # nothing valid
    q = query(pts[:4096] + 10.0, dirs[:4096])
    assert q['last']['counts'] == [0] and not bool(q['mask'].any()) and bool((q['sigma'] == -80.0).all()) and bool((q['rgb'] == 0.0).all())
    # every valid point in the ragged last row
    sel = torch.cat([torch.arange(192), valid[10:27]])
    far = pts[sel].clone()
    far[:192] += 10.0
    q = query(far, dirs[sel])
    assert not bool(q['mask'][:192].any()) and bool(q['mask'][192:].all()) and q['last']['counts'] == [17]
    assert same(q['sigma'][192:], ref['sigma'][sel[192:]]) and same(q['rgb'][192:], ref['rgb'][sel[192:]]) and bool((q['sigma'][:192] == -80.0).all())
    # chunks: 960 points at a time (18 native calls, the last ragged) == one chunk; the observation is encoded once and reused 17 times
    e0, r0 = _lib.frame_observation_stats()
    q = query(pts, dirs, options=dict(query_chunk=1000, token_capacity='worst'))
    e1, r1 = _lib.frame_observation_stats()
    assert q['last']['chunk'] == 960 and len(q['last']['counts']) == 18 and sum(q['last']['counts']) == 628
    assert (e1 - e0, r1 - r0) == (1, 17)
    assert same_out(q, ref)
    # token buffers below the count: the chunk is issued again on buffers of its own count -- finite, the same bits, one re-size
    rend.TOKEN_GRANULE = 64
    try:
        s0 = rend.query_stats()
        q = query(pts, dirs, options=dict(token_capacity=256))
        s1 = rend.query_stats()
        assert s1['resizes'] - s0['resizes'] == 1 and s1['chunks'] - s0['chunks'] == 2 and q['last']['cap'] == 640
        assert bool(torch.isfinite(q['sigma']).all()) and same_out(q, ref)
    finally:
        del rend.TOKEN_GRANULE


# ---- 6. neighbours undisturbed -----------------------------------------------------------------------------------------------------------
def check_neighbours_undisturbed():
    pts, dirs, _, _ = _ray_samples()
    a = frame()
    last_a = a['rend'].last
    cap_a = a['last']['cap']
    full()
    query(pts[:777], dirs[:777])
    assert a['rend'].last is last_a                                        # a query leaves `last` alone
    b = frame()
    assert same(a['rgb'], b['rgb']) and same(a['depth'], b['depth']) and same(a['acc'], b['acc']) and b['last']['cap'] == cap_a
    # a sweep around a query: the frame behind the query still renders from the observation the first frame encoded
    rend = a['rend']
    sweep = dict(reuse_observation=True)
    frame(options=sweep)                                                   # (records the observation key under the option)
    e0, r0 = rend.observation_stats()
    f1 = frame(options=sweep)
    query(pts[:777], dirs[:777])
    f2 = frame(options=sweep)
    e1, r1 = rend.observation_stats()
    assert (e1 - e0, r1 - r0) == (0, 2) and f1['last']['observation_reused'] and f2['last']['observation_reused']
    assert same(f1['rgb'], a['rgb']) and same(f2['rgb'], a['rgb'])


# ---- 7. ABI ------------------------------------------------------------------------------------------------------------------------------
def check_abi_rejects_bad_arguments():
    l = _lib.lib()
    p = ctypes.c_void_p(64)                 # never dereferenced: every call below must be refused before anything is launched
    good = dict(points=p, n=128, Rg=p, Th=p, grid_hdr=p, cell_start=p, cell_pts=p, near_mask=p, capacity=128, counters=p, ray_base=p, ray_cnt=p,
                cs_idx=p, cs_vid=p, cs_xs=p, dense_vid=p, ray_mask=p, scan_ws=p, near_hdr=None, near_list=None, stream=None)
    for bad in (dict(n=0), dict(n=-5), dict(n=1 << 31), dict(cs_idx=None), dict(cs_xs=None), dict(points=None), dict(capacity=0), dict(capacity=-1),
                dict(capacity=127)):
        assert l.sherf_points_mask_nn(*dict(good, **bad).values()) == -1, bad
        assert b'bad argument' in l.sherf_last_error()
    good = dict(counters=p, ray_mask=p, ray_base=p, sample_out=p, n=128, tok_cap=64, rgb=p, sigma=p, mask=p, stream=None)
    for bad in (dict(n=0), dict(n=-1), dict(n=1 << 31), dict(rgb=None), dict(sigma=None), dict(mask=None), dict(tok_cap=0), dict(counters=None)):
        assert l.sherf_field_scatter(*dict(good, **bad).values()) == -1, bad
    fr, q, lv = _lib.Frame(), _lib.FieldQuery(), (_lib.VoxLevel * 3)()
    assert ctypes.sizeof(_lib.FieldQuery) == 48 and _lib.FieldQuery.n.offset == 16 and _lib.FieldQuery.mask.offset == 40
    side = ctypes.c_void_p(8)

    def call(**kw):
        q.points, q.dirs, q.n, q.rgb, q.sigma, q.mask = 64, 64, 128, 64, 64, 64
        fr.capacity, fr.vox_plan = 128, 64
        for k, v in kw.items():
            setattr(fr if k in ('capacity', 'vox_plan') else q, k, v)
        return l.sherf_query_field(ctypes.byref(fr), ctypes.byref(q), lv, None, side, None)
    for bad in (dict(n=0), dict(n=-1), dict(rgb=None), dict(sigma=None), dict(mask=None), dict(points=None), dict(dirs=None), dict(capacity=0),
                dict(capacity=100), dict(vox_plan=None)):
        assert call(**bad) == -1, bad
    assert l.sherf_query_field(None, ctypes.byref(q), lv, None, side, None) == -1 and l.sherf_query_field(ctypes.byref(fr), None, lv, None, side, None) == -1
    q.n = 128
    assert l.sherf_query_field(ctypes.byref(fr), ctypes.byref(q), lv, None, None, None) == -1          # side == main stream


def check_scatter_alone():
    """sherf_field_scatter by itself on hand-made masks: 150 points (two full rows and a ragged one), sample_out holding ten rows fewer than there are valid
    points -> NaN for exactly the points beyond it, flag bit 1, the words behind each output array untouched."""
    rs = np.random.RandomState(3)
    N, GUARD = 150, 16
    bits = rs.uniform(size=N) < 0.4
    bits[[0, 63, 64, 127, 128, 149]] = True
    words = np.zeros(3, np.uint64)
    for i in np.nonzero(bits)[0]:
        words[i >> 6] |= np.uint64(1) << np.uint64(i & 63)
    cnt = np.array([bin(int(w)).count('1') for w in words])
    base = np.concatenate([[0], np.cumsum(cnt)[:-1]]).astype(np.int32)
    nv = int(cnt.sum())
    tok_cap = nv - 10
    sample_out = rs.standard_normal((tok_cap, 4)).astype(np.float32)
    dv = lambda a: G.dev_tensor(torch.from_numpy(np.ascontiguousarray(a)))
    counters = dv(np.array([nv, 0, 0, 0, 0, 0, 0, 0], np.int32))
    rgb, sigma = dv(np.full(N * 3 + GUARD, 7.5, np.float32)), dv(np.full(N + GUARD, 7.5, np.float32))
    mask = dv(np.full(N + GUARD, 77, np.uint8))
    P = _lib.ptr
    d_words, d_base, d_out = dv(words.view(np.int64)), dv(base), dv(sample_out)
    _lib.call('sherf_field_scatter', P(counters), P(d_words), P(d_base), P(d_out), N, tok_cap, P(rgb), P(sigma), P(mask), _lib.stream())
    _sync()
    rgb, sigma, mask, counters = G.plain(rgb), G.plain(sigma), G.plain(mask), G.plain(counters)
    assert bool((rgb[N * 3:] == 7.5).all()) and bool((sigma[N:] == 7.5).all()) and bool((mask[N:] == 77).all())
    c = np.cumsum(bits) - 1
    lost_np = bits & (c >= tok_cap)
    rows = torch.from_numpy(c[bits & ~lost_np])
    bits, lost = torch.from_numpy(bits), torch.from_numpy(lost_np)
    kept = bits & ~lost
    sample_out = torch.from_numpy(sample_out)
    assert int(lost.sum()) == 10 and int(counters[3]) == 2 and int(counters[0]) == nv
    assert torch.equal(mask[:N].bool(), bits)
    rgb = rgb[:N * 3].view(N, 3)
    assert bool(torch.isnan(sigma[:N][lost]).all()) and bool(torch.isnan(rgb[lost]).all())
    assert same(sigma[:N][kept], sample_out[rows, 3]) and same(rgb[kept], sample_out[rows, :3])
    assert bool((sigma[:N][~bits] == -80.0).all()) and bool((rgb[~bits] == 0.0).all())
    # everything fits: no flag
    counters2 = dv(np.zeros(8, np.int32))
    big = dv(rs.standard_normal((nv, 4)).astype(np.float32))
    o_rgb, o_sig, o_mask = dv(np.zeros(N * 3, np.float32)), dv(np.zeros(N, np.float32)), dv(np.zeros(N, np.uint8))
    _lib.call('sherf_field_scatter', P(counters2), P(d_words), P(d_base), P(big), N, nv, P(o_rgb), P(o_sig), P(o_mask), _lib.stream())
    _sync()
    assert int(G.plain(counters2)[3]) == 0


# ---- 8. generator ------------------------------------------------------------------------------------------------------------------------
class _FakeBackbone(torch.nn.Module):
    """Stands in for the StyleGAN2 backbone (outside the hot path): `mapping` is a fixed function of its inputs, `synthesis` scales the fixture's planes by ws."""

    def __init__(self, planes):
        super().__init__()
        self.planes = planes

    def mapping(self, z, c, truncation_psi=1, truncation_cutoff=None, update_emas=False):
        return (z.reshape(1, 1, -1)[:, :, :4] * 0.25 + 1.0).repeat(1, 3, 1)

    def synthesis(self, ws, update_emas=False, **kw):
        return self.planes * ws[0, 0, 0]


class _FakeEncoder(torch.nn.Module):
    def __init__(self, code, feat):
        super().__init__()
        self.code, self.feat = code, feat

    def forward(self, img, extract_feature=False):
        return self.feat if extract_feature else self.code


def _generator():
    from sherf_amd.triplane import TriPlaneGenerator
    fx = G.fixture('tiny')
    rend, dec = G.hip_modules()
    enc = _FakeEncoder(G.dev_tensor(torch.linspace(-1, 1, 8).reshape(1, 8)), G.to_cuda(fx['obs_feat']))
    gen = TriPlaneGenerator(8, 25, 4, True, True, True, True, True, img_resolution=32, img_channels=3, rendering_kwargs=dict(fx['options'], mlp_precision='f16x3'),
                            backbone=_FakeBackbone(G.to_cuda(fx['planes']).view(1, 96, 32, 32)), encoder_2d=enc, encoder_2d_feature=enc, smpl=G.smpl())
    gen.renderer, gen.decoder = rend, dec
    gen.graph_producers = False
    fixtures.load_seeded_state(gen.conv1d_projection, 'generator.conv1d_projection.')
    return G.dev_module(gen), G.to_cuda(fx['input_data'])


def grid_reference(input_data, bounds, resolution):
    """fp64: which grid centres lie within 5 cm of a posed vertex, and which are too close to the threshold to call (the oracle's own margin on d^2: 1e-6)."""
    from sherf_amd.field import grid_centres
    c = G.plain(grid_centres(G.plain(bounds), resolution)).double().reshape(-1, 3)
    v = G.plain(input_data['vertices']).double().reshape(-1, 3)
    d2 = torch.cdist(c, v).min(1)[0] ** 2
    return d2 < 0.05 ** 2, (d2 - 0.05 ** 2).abs() < 1e-6


GRID_BOUNDS = ((-0.45, -0.95, -0.30), (0.50, 0.85, 0.33))          # (an offset for which no centre of the 8^3 grid lies on the threshold: asserted below)


def check_generator():
    from sherf_amd import field
    gen, d = _generator()
    pts, dirs, _, _ = _ray_samples()
    v = torch.from_numpy(G.fixture('tiny')['input_data']['vertices'][0])
    points = torch.cat([v[::40] + 0.01, pts[:500]])                        # near the body and around it
    dirs = dirs[:points.shape[0]]
    P, D = G.dev_tensor(points[None].contiguous()), G.dev_tensor(dirs[None].contiguous())
    z, c0 = G.dev_tensor(torch.linspace(0, 1, 8).reshape(1, 8)), G.dev_tensor(torch.zeros(1, 25))
    with torch.no_grad():
        ws = gen.mapping(z, c0, input_img=d['obs_img_all'][:, 0])
        a = gen.sample_mixed(P, D, ws, input_data=d)
        planes, img, feat, sp, mask, sp_input, _ = gen._observation(ws, d, False, False, False, None, False, False, {})     # what synthesis hands its renderer
        b = gen.renderer.query_points(planes, img, feat, sp, mask, sp_input, gen.decoder, P, D, d, gen.rendering_kwargs)
        s = gen.sample(P, D, z, c0, input_data=d)
    _sync()
    assert set(a) == {'rgb', 'sigma', 'mask'} and 20 < int(a['mask'].sum()) < points.shape[0]
    for k in ('rgb', 'sigma', 'mask'):
        assert same(G.plain(a[k]), G.plain(b[k])) and same(G.plain(s[k]), G.plain(a[k])), k
    with pytest.raises(TypeError):
        gen.sample_mixed(P, D, ws)
    # density_grid
    bounds = torch.tensor(GRID_BOUNDS)
    inside, marginal = grid_reference(d, bounds, 8)
    assert int(marginal.sum()) == 0 and marginal.float().mean() <= 0.01 and int(inside.sum()) > 3
    sigma, rgb, m, bnd = field.density_grid(gen, ws, None, d, 8, bounds=G.dev_tensor(bounds))
    _sync()
    assert sigma.shape == (8, 8, 8) and rgb.shape == (8, 8, 8, 3) and m.shape == (8, 8, 8) and m.dtype == torch.bool and bnd.shape == (2, 3)
    assert int(m.sum()) == int(inside.sum()) and torch.equal(G.plain(m).reshape(-1), inside)
    assert bool((G.plain(sigma)[~G.plain(m)] == -80.0).all())
    # through z and with the default bounds: the posed vertices' box grown by the shell
    sigma2, _, m2, bnd2 = field.density_grid(gen, z, c0, d, (4, 6, 5))
    vv = G.plain(d['vertices']).reshape(-1, 3)
    assert sigma2.shape == (4, 6, 5) and torch.allclose(G.plain(bnd2), torch.stack([vv.min(0)[0] - 0.05, vv.max(0)[0] + 0.05]))


# ---- the tests ---------------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize('case', list(CASES))
def test_query_matches_the_reference_goldens(case):
    check_reference_golden(case)


@gpu
@pytest.mark.parametrize('prec', ['f16x3', 'bf16'])
def test_query_has_the_frames_bits(prec):
    check_same_bits_as_frame(prec)


@gpu
def test_query_through_the_dense_marcher_gives_the_golden_image():
    check_through_the_marcher()


@gpu
def test_per_point_indexing():
    check_per_point_indexing()


@gpu
def test_edge_shapes_chunks_and_token_resize():
    check_edge_shapes()


@gpu
def test_frames_around_a_query_are_undisturbed():
    check_neighbours_undisturbed()


@gpu
def test_abi_rejects_bad_arguments():
    check_abi_rejects_bad_arguments()


@gpu
def test_scatter_alone_overflow_and_guard_words():
    check_scatter_alone()


@gpu
def test_generator_sample_and_density_grid():
    check_generator()
