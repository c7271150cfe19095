"""csrc/gather.hip on table borders, empty voxels, ragged counts and long runs: the seven forward launch forms and the three backward scatters on a
SYNTHETIC scene whose samples are placed by construction (no rendered frame), against a float64 torch evaluation of the same taps written here.
The `check_*` bodies run on the HOST build of the unchanged kernel sources (tests/hipcpu) below and on the MI355X in tests/test_gpu_gather_edges.py.

Every comparison is made per output tensor AND per sample group (the backward: per set of table rows a group's stencils touch), each relative to its
own largest reference entry, at the project's standing bound for these kernels (1e-4: test_gathered_tokens, test_gather_backward_kernel).  Beside
each figure the same reference restated in fp32 torch is printed: what fp32 alone costs.  A group whose fp32 restatement exceeded 5e-5 would be
ill-posed at this bound; the builder's magnitudes keep all of them below it and the tests assert that too.

Row 0 of every voxel level holds 1e4: the forms that read row 0 for an absent corner must weigh it with an exact 0.  Samples whose stencil reaches
row 0's own voxel (key 2 = voxel (0, 0, 2) at every level), or comes within 1e-3 of a cell of it, form the group `row0`, so that its magnitude does
not loosen any other group's comparison."""
import contextlib
import ctypes
import itertools
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from sherf_amd import _lib
from tests import gpu_common as G
from tests.bwd_emulator import make_level
from tests.test_hipcpu_frame import cpu_product          # noqa: F401  (the host builds behind sherf_amd._lib, CPU tensors)

P, HF, WF, H, W = 8, 6, 10, 12, 20
DIMS = ((12, 16, 10), (6, 8, 5), (3, 4, 3))               # (D, H, W) of the three tapped levels: all coarser than the 0.005 grid below
VOX_SH = (24, 32, 20)                                    # (z, y, x) cells of 0.005
BOUND = 1e-4                                             # the standing bound of these kernels
WELL_POSED = 5e-5                                        # the fp32 restatement of a group must stay below this
SENT = -7.5
GUARD = 384                                              # floats between the backward outputs (four voxel rows)
ROW0_VOXEL = (0, 0, 2)                                   # (z, y, x) of key 2: the smallest occupied key of every level


# ---- 1. the synthetic scene -----------------------------------------------------------------------------------------------------------
def _f32(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))


def build_scene(seed=0, n_int=300, n_run=64, n_distinct=200, dims=DIMS, vox_sh=VOX_SH, slabs=None):
    """Random folded tables, three voxel levels and geom [n,8] in named groups (see the module's header and `groups`).  `slabs`: [(z_lo, z_hi)] in
    level-0 cells -- the occupied voxels and the samples of the interior groups are confined to them (large grids)."""
    rs = np.random.RandomState(seed)
    sc = SimpleNamespace(dims=tuple(dims), vox_sh=tuple(vox_sh))
    sc.planes_f, sc.feat_f = _f32(rs.standard_normal((3, P, P, 32))), _f32(rs.standard_normal((HF, WF, 64)))
    sc.img4, sc.tok_bias = _f32(rs.uniform(0, 1, (H, W, 4))), _f32(rs.standard_normal(96))
    ext = np.array(vox_sh[::-1], np.float64) * 0.005                         # (x, y, z) extent of the voxel volume
    sc.vox_min = _f32(-ext * np.array([0.5, 0.45, 0.55]))
    vmin = sc.vox_min.double().numpy()
    sc.bounds = _f32(np.concatenate([vmin - 0.12 * ext, vmin + 1.2 * ext]))      # tri-plane bounds: around the volume
    lo, hi = sc.bounds.double().numpy()[:3], sc.bounds.double().numpy()[3:]
    D0, H0, W0 = dims[0]
    in_slab = lambda z0: np.ones_like(z0, bool) if slabs is None else np.any([(z0 >= a) & (z0 < b) for a, b in slabs], axis=0)
    # voxel levels: about a third occupied; one empty and one full 2x2x2 neighbourhood; keys at bit 31 / bit 0 of a record word; the last key
    sc.levels = []
    for D, Hh, Ww in dims:
        K = D * Hh * Ww
        m = rs.rand(K) < 1 / 3
        z0 = (np.arange(K) // (Hh * Ww)) * (D0 - 1) / max(D - 1, 1)
        if slabs is not None:
            m &= np.any([(z0 >= a - 4) & (z0 < b + 4) for a, b in slabs], axis=0)
        key = lambda z, y, x: (z * Hh + y) * Ww + x
        for dz, dy, dx in itertools.product((0, 1), repeat=3):
            m[key(dz, dy, dx)] = False
            m[key(D - 2 + dz, Hh - 2 + dy, Ww - 2 + dx)] = True
        for k in (2, 31, 32, 63, 64, K - 1):
            if k < K:
                m[k] = True
        keys = torch.from_numpy(np.nonzero(m)[0])
        emu, ker = make_level(keys, (D, Hh, Ww))
        rows = _f32(rs.standard_normal((ker['cap'], 96)))
        rows[0] = 1e4                                                        # (an absent corner read at row 0 must weigh exactly 0)
        rows[keys.numel():] = float('nan')                                   # (the padding rows are never read)
        sc.levels.append(SimpleNamespace(dims=(D, Hh, Ww), keys=keys, n_rows=keys.numel(), cap=ker['cap'], wp=ker['wp'], rows=rows))

    def world(p, L=0):                                                       # level-L positions (pz, py, px) -> (x, y, z)
        D, Hh, Ww = dims[L]
        return vmin + p[:, ::-1] / (np.array([Ww, Hh, D], np.float64) - 1) * ext

    def zsel(n):
        if slabs is None:
            return rs.uniform(0, D0 - 1, n)
        s = np.array(slabs, np.float64)[rs.randint(0, len(slabs), n)]
        return rs.uniform(s[:, 0], np.minimum(s[:, 1], D0 - 1))

    interior = lambda n: np.stack([zsel(n), rs.uniform(0, H0 - 1, n), rs.uniform(0, W0 - 1, n)], 1)
    uv_in = lambda n: np.stack([rs.uniform(0, W * 0.999, n), rs.uniform(0, H * 0.999, n)], 1)
    g = {}
    g['interior'] = (world(interior(n_int)), uv_in(n_int))
    for name, base in (('empty_cell', lambda d: (0, 0, 0)), ('full_cell', lambda d: (d[0] - 2, d[1] - 2, d[2] - 2))):
        xs = [world(np.array(base(d), np.float64) + rs.uniform(0.05, 0.95, (6, 3)), L) for L, d in enumerate(dims)]
        g[name] = (np.concatenate(xs), uv_in(18))
    xs = [world(np.array(ROW0_VOXEL, np.float64) + rs.uniform(-0.9, 0.9, (4, 3)), L) for L in range(3)]
    g['row0'] = (np.concatenate(xs), uv_in(12))
    # (b) on each face of the tri-plane bounds, and outside it by a quarter of a texel / by 1.2 texels
    on, out = [], []
    for a in range(3):
        t = (hi[a] - lo[a]) / P
        for face, sgn in ((lo[a], -1.0), (hi[a], 1.0)):
            for off, dst in ((0.0, on), (0.25, out), (1.2, out)):
                x = world(interior(2))
                x[:, a] = face + sgn * off * t
                dst.append(x)
    g['plane_face'] = (np.concatenate(on), uv_in(12))
    g['plane_out'] = (np.concatenate(out), uv_in(24))
    # (c) far outside everything
    g['far'] = (rs.choice([-50.0, 50.0], (33, 3)), rs.choice([-500.0, 500.0], (33, 2)))
    # (d) outside the observed image on each side: half a feature-map texel (one column / row still tapped), and past the clamp
    uv = uv_in(16)
    for i, (ax, full, nf) in enumerate(((0, W, WF), (1, H, HF))):
        for k, p in enumerate((-0.5, -3.0, nf - 0.5, nf + 3.0)):
            uv[8 * i + 2 * k:8 * i + 2 * k + 2, ax] = full * p / (nf - 1)
    g['uv_out'] = (world(interior(16)), uv)
    # (e) outside the voxel volume on each side (half a level-0 cell; past the clamp), and exactly at vox_min
    p = interior(24)
    for a, d in enumerate(dims[0]):
        for k, v in enumerate((-0.5, -2.5, d - 0.5, d + 1.5)):
            p[8 * a + 2 * k:8 * a + 2 * k + 2, a] = v
    g['vox_out'] = (world(p), uv_in(24))
    g['vox_min'] = (np.repeat(vmin[None], 3, 0), uv_in(3))
    # (f) one finest cell, one feature-map texel: a run that is flushed once
    c0 = np.array([D0 - 4, H0 - 5, W0 - 4], np.float64)
    uvr = np.stack([W * (3 + rs.uniform(0.1, 0.9, n_run)) / (WF - 1), H * (2 + rs.uniform(0.1, 0.9, n_run)) / (HF - 1)], 1)
    g['run'] = (world(c0 + rs.uniform(0.02, 0.98, (n_run, 3))), uvr)
    # (g) every sample in its own finest cell, in descending cell order: a flush per sample
    zs = np.arange(D0 - 1)
    zs = zs[in_slab(zs) & in_slab(zs + 1)] if slabs is not None else zs
    cells = np.stack(np.meshgrid(zs, np.arange(H0 - 1), np.arange(W0 - 1), indexing='ij'), -1).reshape(-1, 3)
    cells = cells[np.sort(rs.choice(len(cells), min(n_distinct, len(cells)), replace=False))[::-1]]
    g['distinct'] = (world(cells + rs.uniform(0.1, 0.9, cells.shape)), uv_in(len(cells)))
    names = list(g)
    xyz, uv = np.concatenate([g[k][0] for k in names]), np.concatenate([g[k][1] for k in names])
    label = np.concatenate([np.full(len(g[k][0]), i) for i, k in enumerate(names)])
    n = len(xyz)
    v = rs.standard_normal((n, 3))
    geom = _f32(np.concatenate([xyz, v / np.linalg.norm(v, axis=1, keepdims=True), uv], 1))
    perm = rs.permutation(n)                                                 # the direct forms see the groups interleaved
    sc.geom, label = geom[perm].contiguous(), torch.from_numpy(label[perm])
    # whoever comes near row 0's voxel at any level belongs to `row0`
    pos = _positions(sc, sc.geom, torch.float64)
    near = torch.zeros(n, dtype=torch.bool)
    for L in range(3):
        px, py, pz = pos['vox'][L]
        near |= ((pz - ROW0_VOXEL[0]).abs() < 1.001) & ((py - ROW0_VOXEL[1]).abs() < 1.001) & ((px - ROW0_VOXEL[2]).abs() < 1.001)
    label[near] = names.index('row0')
    sc.groups = {k: torch.nonzero(label == i)[:, 0] for i, k in enumerate(names)}
    sc.n = n
    sc.d_tok = _f32(rs.standard_normal((n, 96)))
    return sc


# ---- 2. the reference: plain torch at `dtype` ---------------------------------------------------------------------------------------------
def _positions(sc, geom, dtype):
    """Continuous texel / voxel coordinates of every tap family (renderer.py:234-243 align_corners=False; :330-336 and :544-556 align_corners=True)."""
    g = geom.to(dtype)
    x, b, vm = g[:, :3], sc.bounds.to(dtype), sc.vox_min.to(dtype)
    nrm = 2 * (x - b[:3]) / (b[3:] - b[:3]) - 1
    pl = [((nrm[:, a] + 1) * P - 1) * 0.5 for a in range(3)]
    gx, gy = 2 * g[:, 6] / W - 1, 2 * g[:, 7] / H - 1
    gv = [((x[:, a] - vm[a]) / 0.005) / sc.vox_sh[2 - a] * 2 - 1 for a in range(3)]             # x, y, z
    return dict(planes=[(pl[0], pl[1]), (pl[0], pl[2]), (pl[2], pl[1])],
                feat=((gx + 1) * 0.5 * (WF - 1), (gy + 1) * 0.5 * (HF - 1)), img=((gx + 1) * 0.5 * (W - 1), (gy + 1) * 0.5 * (H - 1)),
                vox=[tuple((gv[a] + 1) * 0.5 * (d[2 - a] - 1) for a in range(3)) for d in sc.dims])


def _stencil(ps, dims, eps=0.0):
    """Linear interpolation with zero padding.  ps / dims: fastest axis first.  -> flat index [n,K] (-1 outside the table), weight [n,K].
    eps > 0: every texel a position within eps of this one could tap (three per axis), weights 1."""
    n = ps[0].shape[0]
    idx, w = torch.zeros(n, 1, dtype=torch.long), torch.ones(n, 1, dtype=ps[0].dtype)
    ok, stride = torch.ones(n, 1, dtype=torch.bool), 1
    for p, d in zip(ps, dims):
        l = torch.floor(p - eps)
        c = l.long()[:, None] + torch.arange(3 if eps else 2)
        oka = (c >= 0) & (c < d)
        if eps:
            oka &= c <= (torch.floor(p + eps).long()[:, None] + 1)
            wa = torch.ones_like(c, dtype=p.dtype)
        else:
            wa = torch.stack([1 - (p - l), p - l], 1)
        idx = (idx[:, None, :] + (c * stride)[:, :, None]).reshape(n, -1)
        w = (w[:, None, :] * wa[:, :, None]).reshape(n, -1)
        ok = (ok[:, None, :] & oka[:, :, None]).reshape(n, -1)
        stride *= d
    return torch.where(ok, idx, torch.full_like(idx, -1)), torch.where(ok, w, torch.zeros_like(w))


def _rows_of(lev, key):
    """voxel keys [n,K] (-1: outside) -> row indices, -1 where the voxel is absent."""
    pos = torch.searchsorted(lev.keys, key.clamp(min=0)).clamp(max=lev.n_rows - 1)
    return torch.where((key >= 0) & (lev.keys[pos] == key), pos, torch.full_like(pos, -1))


def taps(sc, geom, dtype, eps=0.0):
    """[(table, row index [n,K] or -1, weight [n,K], the token channels the table's columns add to)]"""
    pos, out = _positions(sc, geom, dtype), []
    for p in range(3):
        i, w = _stencil(pos['planes'][p], (P, P), eps)
        out.append(('planes', torch.where(i >= 0, i + p * P * P, i), w, slice(32 * p, 32 * p + 32)))
    out.append(('feat', *_stencil(pos['feat'], (WF, HF), eps), slice(0, 64)))
    for L, lev in enumerate(sc.levels):
        D, Hh, Ww = lev.dims
        k, w = _stencil(pos['vox'][L], (Ww, Hh, D), eps)
        r = _rows_of(lev, k)
        out.append((f'rows{L}', r, torch.where(r >= 0, w, torch.zeros_like(w)), slice(0, 96)))
    return out


def tables(sc, half, dtype):
    """The folded tables as [rows, channels]; `half`: rounded to fp16 first, as the fp16 forms read them."""
    r = (lambda t: t.half()) if half else (lambda t: t)
    t = dict(planes=r(sc.planes_f).view(3 * P * P, 32), feat=r(sc.feat_f).view(HF * WF, 64))
    t.update({f'rows{L}': r(lev.rows) for L, lev in enumerate(sc.levels)})
    return {k: v.to(dtype) for k, v in t.items()}


def ref_forward(sc, geom, dtype, half=False):
    """-> tokens [n,96] (slot s = channels 32 s ..), tapped rgb [n,3]"""
    tab = tables(sc, half, dtype)
    tok = sc.tok_bias.to(dtype).expand(geom.shape[0], 96).clone()
    for name, i, w, sl in taps(sc, geom, dtype):
        tok[:, sl] += (w[..., None] * tab[name][i.clamp(min=0)]).sum(1)                  # (an absent corner: row 0 with weight 0)
    i, w = _stencil(_positions(sc, geom, dtype)['img'], (W, H))
    rgb = (w[..., None] * sc.img4.to(dtype).view(H * W, 4)[i.clamp(min=0)]).sum(1)[:, :3]
    return tok, rgb


def table_shapes(sc):
    s = dict(planes=(3 * P * P, 32), feat=(HF * WF, 64))
    s.update({f'rows{L}': (lev.cap, 96) for L, lev in enumerate(sc.levels)})
    return s


def ref_backward(sc, geom, d_tok, dtype):
    """The scatter of d_tok [n,96] with the forward's weights -> {table: gradient}, 'bias': [96]"""
    d = d_tok.to(dtype)
    out = {k: torch.zeros(s, dtype=dtype) for k, s in table_shapes(sc).items()}
    for name, i, w, sl in taps(sc, geom, dtype):
        C = out[name].shape[1]
        out[name].index_add_(0, i.clamp(min=0).reshape(-1), (w[..., None] * d[:, None, sl]).reshape(-1, C))
    out['bias'] = d.sum(0)
    return out


def touched(sc, geom, eps=0.0):
    """{table: bool [rows]}: the rows some sample's stencil reaches (eps: or would reach from a position within eps)."""
    out = {k: torch.zeros(s[0], dtype=torch.bool) for k, s in table_shapes(sc).items()}
    for name, i, w, sl in taps(sc, geom, torch.float64, eps):
        out[name][i[i >= 0]] = True
    return out


# ---- 3. the kernels through the C ABI -------------------------------------------------------------------------------------------------------
@contextlib.contextmanager
def experiment(word):
    old = os.environ.get('SHERF_EXPERIMENT')
    os.environ['SHERF_EXPERIMENT'] = str(word)
    try:
        yield
    finally:
        if old is None:
            del os.environ['SHERF_EXPERIMENT']
        else:
            os.environ['SHERF_EXPERIMENT'] = old


@contextlib.contextmanager
def debug_bits(bits):
    _lib.lib().sherf_set_debug(int(bits))
    try:
        yield
    finally:
        _lib.lib().sherf_set_debug(0)


def _sync():
    if not G.CPU_SHIM:
        torch.cuda.synchronize()


_MAPPINGS = []


def guarded_copy(t, side):
    """A copy of the int32 tensor t (host memory) in an anonymous mapping between two inaccessible pages; its first ('start') or last ('end') byte
    touches one of them, so that a read outside the array on that side ends the process instead of returning whatever lies there."""
    import mmap
    page, nbytes = mmap.PAGESIZE, t.numel() * 4
    body = -(-nbytes // page) * page
    mm = mmap.mmap(-1, body + 2 * page)
    base = ctypes.addressof(ctypes.c_char.from_buffer(mm))
    libc = ctypes.CDLL(None, use_errno=True)
    libc.mprotect.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
    assert libc.mprotect(base, page, 0) == 0 and libc.mprotect(base + page + body, page, 0) == 0, ctypes.get_errno()
    out = torch.frombuffer(mm, dtype=torch.int32, count=t.numel(), offset=page + (body - nbytes if side == 'end' else 0))
    out.copy_(t.reshape(-1))
    _MAPPINGS.append(mm)
    return out


class Dev:
    """A scene's tables on the device (fp32 and fp16) and the entry points' argument lists."""

    def __init__(self, sc, guard=None):
        d = G.dev_tensor
        self.sc = sc
        self.planes, self.feat = {False: d(sc.planes_f), True: d(sc.planes_f.half())}, {False: d(sc.feat_f), True: d(sc.feat_f.half())}
        self.img4, self.bias, self.bounds, self.vox_min = d(sc.img4), d(sc.tok_bias), d(sc.bounds), d(sc.vox_min)
        self.vox_sh = (ctypes.c_int32 * 3)(*sc.vox_sh)
        self.wp = [d(lev.wp) if guard is None else guarded_copy(lev.wp, guard) for lev in sc.levels]       # (guard: host build only)
        self.rows = {False: [d(lev.rows) for lev in sc.levels], True: [d(lev.rows.half()) for lev in sc.levels]}
        self.levels = {h: self._struct(self.rows[h]) for h in (False, True)}
        self.geom = d(sc.geom)

    def _struct(self, rows):
        lv = (_lib.VoxLevel * 3)()
        for L, lev in enumerate(self.sc.levels):
            lv[L].wp, lv[L].rows = _lib.addr(self.wp[L]), _lib.addr(rows[L])
            lv[L].D, lv[L].H, lv[L].W = lev.dims
        return lv

    @staticmethod
    def counters(count):
        return G.dev_tensor(torch.tensor([count, 0, 0, 0, 0, 0, 0, 0], dtype=torch.int32))

    def buffers(self, tiles):
        where = None if G.CPU_SHIM else 'cuda'
        return (G.dev_tensor(torch.full((tiles * 3072,), SENT, device=where)), G.dev_tensor(torch.full((tiles * 384,), SENT, device=where)))

    def forward(self, count, capacity, mode, bufs, geom=None):
        """sherf_gather_tokens into `bufs` = (tokens, extras); `mode | 16` reads the fp16 tables."""
        half, p = bool(mode & 16), _lib.ptr
        cnt = self.counters(count)
        _lib.call('sherf_gather_tokens', p(cnt), p(self.geom if geom is None else geom), p(self.planes[half]), P, p(self.feat[half]), HF, WF, p(self.img4), H, W,
                  self.levels[half], p(self.bias), p(self.bounds), p(self.vox_min), self.vox_sh, mode, capacity, p(bufs[0]), p(bufs[1]), _lib.stream())
        _sync()
        return bufs

    def backward(self, count, capacity, d_tiled, form, geom=None):
        """form: 'runs' (the step's), 'binned' (SHERF_EXPERIMENT=256), 'direct'.  -> ({table: gradient, 'bias'}, scratch or None, bins)"""
        p = _lib.ptr
        # the outputs, pre-filled with zeros as the step does, carved out of one buffer with GUARD zeros before, between and behind them: a row index of -1
        # or of `cap` lands in a guard and is reported, instead of in somebody else's memory
        shapes = dict(table_shapes(self.sc), bias=(96,))
        sizes = [int(np.prod(s)) for s in shapes.values()]
        flat = G.dev_tensor(torch.zeros(sum(sizes) + GUARD * (len(sizes) + 1), device=None if G.CPU_SHIM else 'cuda'))
        out, guards, o = {}, [], 0
        for (k, s), size in zip(shapes.items(), sizes):
            guards.append(flat[o:o + GUARD])
            out[k] = flat[o + GUARD:o + GUARD + size].view(s)
            o += GUARD + size
        guards.append(flat[o:])
        self.guards = guards
        cnt = self.counters(count)
        args = (p(cnt), p(self.geom if geom is None else geom), p(d_tiled), P, HF, WF, H, W, self.levels[False], p(self.bounds), p(self.vox_min), self.vox_sh,
                capacity, p(out['planes']), p(out['feat']), p(out['rows0']), p(out['rows1']), p(out['rows2']), p(out['bias']))
        if form == 'direct':
            _lib.call('sherf_gather_tokens_bwd', *args, _lib.stream())
            _sync()
            self.assert_guards(form)
            return out, None, 0
        words = ctypes.c_int64(0)
        _lib.call('sherf_gather_bwd_scratch_words', self.levels[False], capacity, ctypes.byref(words))
        slack = 2 * max(count - capacity, 0) + 64               # (behind the words the entry point asks for; stays untouched)
        scratch = G.dev_tensor(torch.full((words.value + slack,), -7, dtype=torch.int32, device=None if G.CPU_SHIM else 'cuda'))       # (not zeroed by the caller)
        with experiment(0 if form == 'runs' else 256):
            _lib.call('sherf_gather_tokens_bwd_binned', *args, p(scratch), words.value, _lib.stream())
            _sync()
        self.assert_guards(form)
        assert bool((scratch[words.value:] == -7).all()), (form, 'the scratch was written behind its end')
        D, Hh, Ww = self.sc.dims[0 if form == 'runs' else 2]
        return out, scratch, (D + 4) * (Hh + 4) * (Ww + 4)


    def assert_guards(self, form):
        assert all(bool((g == 0).all()) for g in self.guards) and self.guards[-1].numel() == GUARD, (form, 'a scatter landed outside its table')


def tile_tokens(d_tok, tiles, fill=0.0):
    """[n,96] -> [tile][3][8][32] float4 (sherf_bwd_tile_tokens); the columns behind sample n hold `fill` (no kernel reads them)"""
    pad = torch.full((tiles * 32, 96), fill)
    pad[:d_tok.shape[0]] = d_tok
    return pad.view(tiles, 32, 3, 8, 4).permute(0, 2, 3, 1, 4).reshape(-1).contiguous()


def _bits(t):
    return t.contiguous().view(torch.int32)


def same_bits(a, b):
    return all(torch.equal(_bits(x), _bits(y)) for x, y in zip(a, b))


# ---- 4. assertions ------------------------------------------------------------------------------------------------------------------
def _err(a, b):
    """largest error of a against b, relative to b's largest entry"""
    return float((a.double() - b.double()).abs().max() / b.double().abs().max().clamp(min=1e-30))


def _references(sc, half):
    key = f'ref_fwd_{half}'
    if not hasattr(sc, key):
        setattr(sc, key, (ref_forward(sc, sc.geom, torch.float64, half), ref_forward(sc, sc.geom, torch.float32, half)))
    return getattr(sc, key)


def assert_forward(sc, label, bufs, n, tiles, half, exact=True):
    """Accuracy per tensor and group; the exact properties of the layout (see the module's header)."""
    tokens, extras = (G.plain(b) for b in bufs)
    tiles_n = (n + 31) // 32
    tok = tokens[:tiles_n * 3072].view(tiles_n, 3, 8, 32, 4).permute(0, 3, 1, 2, 4).reshape(tiles_n * 32, 96)
    ex = extras[:tiles_n * 384].view(tiles_n, 12, 32).permute(0, 2, 1).reshape(tiles_n * 32, 12)
    # beyond tile ceil(n / 32) nothing is written; the last tile's padding columns and the extras' padding rows are exactly 0
    assert bool((tokens[tiles_n * 3072:] == SENT).all()) and bool((extras[tiles_n * 384:] == SENT).all()), label
    assert tokens.numel() == tiles * 3072 and bool((tok[n:] == 0).all()) and bool((ex[n:] == 0).all()) and bool((ex[:n, 9:] == 0).all()), label
    assert torch.equal(_bits(ex[:n, :6]), _bits(sc.geom[:n, :6])), label                          # x_c, v_c: copies
    (t64, c64), (t32, c32) = _references(sc, half)
    bad = []
    for name, g in sc.groups.items():
        g = g[g < n]
        if not g.numel():
            continue
        for tensor, ours, r64, r32 in (('tokens', tok, t64, t32), ('rgb', ex[:, 6:9], c64, c32)):
            if tensor == 'rgb' and float(r64[g].abs().max()) == 0:
                assert bool((ours[g] == 0).all()), (label, name)
                continue
            e, e32 = _err(ours[g], r64[g]), _err(r32[g], r64[g])
            print(f'{label:34s} {tensor:7s} {name:11s} n={g.numel():5d}  ours {e:.2e}  fp32 torch {e32:.2e}')
            if e > BOUND or e32 > WELL_POSED:
                bad.append((label, tensor, name, e, e32))
    if exact and 'far' in sc.groups:                                                              # empty stencils: the bias, bit for bit
        g = sc.groups['far'][sc.groups['far'] < n]
        assert torch.equal(_bits(tok[g]), _bits(sc.tok_bias.expand(g.numel(), 96))), label
    assert not bad, bad


def check_forward(sc, dev, label, n=None, over=0):
    """Every forward form on the first n samples (counters[0] = n + over, capacity = n): the forms agree bit for bit, the parts assemble one launch,
    the two-pass split agrees within the bound; accuracy and layout against the references."""
    n = sc.n if n is None else n
    tiles = (n + over + 31) // 32 + 2                          # (room for what a kernel without the capacity clamp would write)
    run = lambda mode, bufs=None: dev.forward(n + over, n, mode, bufs or dev.buffers(tiles))
    for half in (False, True):
        h = 16 if half else 0
        base = run(h)                                          # fp32: the branching four-channel kernel; fp16: the sixteen-channel kernel
        assert_forward(sc, f'{label} {"fp16" if half else "fp32"}', base, n, tiles, half)
        if half:
            with experiment(1024):
                assert same_bits(run(h), base), (label, 'eight channels, rows requested ahead')
            with experiment(1536):
                assert same_bits(run(h), base), (label, 'eight channels')
            with debug_bits(1 << 29):
                assert same_bits(run(h), base), (label, 'records staged in LDS')
            # the four-channel kernel on fp16 tables (debug bit 11; `mode | 4`: branchless): the same taps in another order of lanes -- within the bound
            with debug_bits(2048):
                assert_forward(sc, f'{label} fp16 four channels', run(h), n, tiles, half)
            assert_forward(sc, f'{label} fp16 branchless', run(h | 4), n, tiles, half)
        else:
            assert same_bits(run(4), base), (label, 'branchless')
            assert same_bits(run(12), base), (label, 'squeezed')
        for nparts in (2, 3):
            bufs = dev.buffers(tiles)
            for part in range(nparts):
                run(h | (part << 8) | (nparts << 16), bufs)
            assert same_bits(bufs, base), (label, half, nparts)
        two = run(h | 2, run(h | 1))                           # planes + pixel taps, then the voxel taps added onto the stored tokens
        assert torch.equal(_bits(G.plain(two[1])), _bits(G.plain(base[1]))), (label, half)
        assert_forward(sc, f'{label} {"fp16" if half else "fp32"} two passes', two, n, tiles, half, exact=False)


def assert_backward(sc, label, out, n, d_tok, reps=1, tail=0):
    """Per table and group: the rows the group's stencils touch, against float64, relative to the largest reference entry among them.  Rows no stencil
    reaches (with 1e-3 of a cell to spare), and every row at or above n_rows, are exactly 0.  reps, tail: the first n samples were given `reps` times
    over, then the first `tail` of them once more."""
    geom = sc.geom[:n]
    r64, r32 = ref_backward(sc, geom, d_tok[:n], torch.float64), ref_backward(sc, geom, d_tok[:n], torch.float32)
    if (reps, tail) != (1, 0):
        t64, t32 = ref_backward(sc, geom[:tail], d_tok[:tail], torch.float64), ref_backward(sc, geom[:tail], d_tok[:tail], torch.float32)
        r64, r32 = {k: reps * v + t64[k] for k, v in r64.items()}, {k: reps * v + t32[k] for k, v in r32.items()}
    ours = {k: G.plain(v) for k, v in out.items()}
    reach = touched(sc, geom, eps=1e-3)
    for k, m in reach.items():
        assert bool((ours[k][~m] == 0).all()), (label, k, 'an element no stencil reaches was written')
    for L, lev in enumerate(sc.levels):
        assert bool((ours[f'rows{L}'][lev.n_rows:] == 0).all()), (label, L)
    bad = []
    e, e32 = _err(ours['bias'], r64['bias']), _err(r32['bias'], r64['bias'])
    print(f'{label:34s} {"bias":7s} {"all":11s} n={n:5d}  ours {e:.2e}  fp32 torch {e32:.2e}')
    if e > BOUND or e32 > WELL_POSED:
        bad.append((label, 'bias', e, e32))
    for name, g in sc.groups.items():
        g = g[g < n]
        if not g.numel():
            continue
        for k, m in touched(sc, geom[g]).items():
            if not bool(m.any()):
                continue
            if float(r64[k][m].abs().max()) == 0:
                assert bool((ours[k][m] == 0).all()), (label, k, name)
                continue
            e, e32 = _err(ours[k][m], r64[k][m]), _err(r32[k][m], r64[k][m])
            print(f'{label:34s} {k:7s} {name:11s} n={g.numel():5d}  ours {e:.2e}  fp32 torch {e32:.2e}')
            if e > BOUND or e32 > WELL_POSED:
                bad.append((label, k, name, e, e32))
    assert not bad, bad


def assert_scratch(label, scratch, bins, nv, capacity, form):
    """Every sample counted once, the order a permutation, the run form's ascending in the finest cell."""
    s = G.plain(scratch)
    counts = s[4:4 + bins]
    assert int(counts.sum()) == nv and int(s[0]) == int((counts > 0).sum()), (label, form)
    b = s[4 + 4 * bins:4 + 4 * bins + capacity][:nv]
    order = s[4 + 4 * bins + capacity:4 + 4 * bins + 2 * capacity][:nv].long()
    assert torch.equal(torch.sort(order)[0], torch.arange(nv)), (label, form)
    if form == 'runs':
        assert bool((b[order][1:] >= b[order][:-1]).all()), (label, form)
    return b[order]


def check_backward(sc, dev, label, n=None, over=0, forms=('runs', 'binned', 'direct')):
    n = sc.n if n is None else n
    d_tiled = G.dev_tensor(tile_tokens(sc.d_tok[:n], (n + over + 31) // 32, fill=3.0))
    for form in forms:
        out, scratch, bins = dev.backward(n + over, n, d_tiled, form)
        if scratch is not None:
            assert_scratch(label, scratch, bins, n, n, form)
        assert_backward(sc, f'{label} {form}', out, n, sc.d_tok)


# ---- 5. the cases -------------------------------------------------------------------------------------------------------------------
_SCENES, _DEVS = {}, {}
N_FIXED = 160                                            # samples of the groups whose size the builder fixes


def scene(name):
    """-> (scene, its tables on the device): one per name, the device copy per build (host / device) as well."""
    if name not in _SCENES:
        _SCENES[name] = {'small': lambda: build_scene(seed=1, n_int=40, n_run=24, n_distinct=40),
              'run': lambda: build_scene(seed=2, n_int=300, n_run=5000, n_distinct=400),
              'base4096': lambda: build_scene(seed=3, n_int=600, n_run=2500, n_distinct=4096 - 600 - 2500 - N_FIXED),
              'scan': lambda: build_scene(seed=4, n_int=900, n_run=100, n_distinct=2000 - 900 - 100 - N_FIXED, dims=((100, 100, 100), (50, 50, 50), (25, 25, 25)),
                                          vox_sh=(200, 200, 200), slabs=[(0, 4), (95, 99)])}[name]()
    return _SCENES[name]


def scene_on_device(name):
    key = (name, G.CPU_SHIM)
    if key not in _DEVS:
        _DEVS[key] = Dev(scene(name))
    return scene(name), _DEVS[key]


RAGGED = (1, 31, 33, 64, 65, 127, 129, 200)


def check_groups_are_what_they_say():
    """The builder's own claims, from the float64 stencils: `far` taps nothing, `empty_cell` / `full_cell` hold samples with no / all eight corners of
    a level present, only `row0` reaches row 0, every record word's bit 0 and bit 31 and the last word are exercised."""
    sc = scene('small')
    assert all(g.numel() for g in sc.groups.values()), {k: g.numel() for k, g in sc.groups.items()}
    t = {name: (i, w) for name, i, w, sl in taps(sc, sc.geom, torch.float64) if name.startswith('rows')}
    far = sc.groups['far']
    for name, i, w, sl in taps(sc, sc.geom, torch.float64):
        assert bool((i[far] < 0).all()), name
    present = torch.stack([(t[f'rows{L}'][0] >= 0).sum(1) for L in range(3)], 1)
    assert bool((present[sc.groups['empty_cell']] == 0).any(1).all()) and bool((present[sc.groups['full_cell']] == 8).any(1).all())
    assert 0 < int((present == 0).sum()) and 0 < int(((present > 0) & (present < 8)).sum())
    others = torch.cat([g for k, g in sc.groups.items() if k != 'row0'])
    assert all(bool((t[f'rows{L}'][0][others] != 0).all()) for L in range(3)) and any(bool((t[f'rows{L}'][0][sc.groups['row0']] == 0).any()) for L in range(3))
    for lev in sc.levels:
        K = lev.dims[0] * lev.dims[1] * lev.dims[2]
        assert {2, 31, 32, K - 1} <= set(lev.keys.tolist()) and 0.2 < lev.n_rows / K < 0.6, lev.dims
    pos = _positions(sc, sc.geom, torch.float64)['vox'][0]
    cell = lambda g: torch.stack([torch.floor(p[g]) for p in pos], 1)
    assert len(torch.unique(cell(sc.groups['run']), dim=0)) == 1
    assert len(torch.unique(cell(sc.groups['distinct']), dim=0)) == sc.groups['distinct'].numel()


def check_ragged_forward(n):
    sc, dev = scene_on_device('small')
    assert sc.n >= 256
    check_forward(sc, dev, f'n={n}', n=n)


def check_ragged_backward(n):
    sc, dev = scene_on_device('small')
    check_backward(sc, dev, f'n={n}', n=n)


def check_overflowing_count():
    """counters[0] = n + 100 > capacity = n: every kernel clamps; nothing beyond tile ceil(n / 32) is written, no sample beyond n is scattered."""
    sc, dev = scene_on_device('small')
    check_forward(sc, dev, 'n=77+100', n=77, over=100)
    check_backward(sc, dev, 'n=77+100', n=77, over=100)


def check_records_are_read_inside_their_array():
    """Host build only: every form on the small scene with each level's (bits, prefix) records between two inaccessible pages, once flush with the
    page before them, once with the page behind them.  The stencils of the outside groups ask for keys below 0 and beyond the last word."""
    sc = scene('small')
    for side in ('start', 'end'):
        dev = Dev(sc, guard=side)
        check_forward(sc, dev, f'records guarded at their {side}')
        check_backward(sc, dev, f'records guarded at their {side}')


def check_long_run_forward():
    sc, dev = scene_on_device('run')
    check_forward(sc, dev, f'run n={sc.n}')


def check_long_run_backward():
    """5000 samples in one finest cell (about 80 chunks of one run: flushed once, at the end, by every wave that holds a piece of it) among samples that
    each have a cell of their own (a flush per sample).  The host build reports two compute units, so its eight workgroups walk three chunks per wave
    (per = 3) here; the device needs tests/test_gpu_gather_edges.py::test_multi_chunk_walk for per > 1."""
    sc, dev = scene_on_device('run')
    assert sc.groups['run'].numel() == 5000
    check_backward(sc, dev, f'run n={sc.n}')


def check_second_scan_trip():
    """A finest level of (100, 100, 100): 104^3 = 1 124 864 bins = 1099 scan blocks, so bin_scan_top_kernel makes a second trip with a carry; half
    of the samples fall in bins above 1024 x 1024."""
    sc, dev = scene_on_device('scan')
    n = sc.n
    assert n == 2000
    d_tiled = G.dev_tensor(tile_tokens(sc.d_tok, (n + 31) // 32))
    out, scratch, bins = dev.backward(n, n, d_tiled, 'runs')
    assert bins == 104 ** 3 and (bins + 1023) // 1024 == 1099
    b = assert_scratch('scan', scratch, bins, n, n, 'runs')
    hi = int((b >= 1024 * 1024).sum())
    assert 0.4 * n < hi < 0.6 * n, hi
    assert_backward(sc, 'scan runs', out, n, sc.d_tok)


# ---- the host build -----------------------------------------------------------------------------------------------------------------------
def test_scene_groups_are_what_they_say():
    check_groups_are_what_they_say()


@pytest.mark.parametrize('n', RAGGED)
def test_ragged_counts_forward(cpu_product, n):
    check_ragged_forward(n)


@pytest.mark.parametrize('n', RAGGED)
def test_ragged_counts_backward(cpu_product, n):
    check_ragged_backward(n)


def test_count_above_capacity(cpu_product):
    check_overflowing_count()


def test_long_run_forward(cpu_product):
    check_long_run_forward()


def test_long_run_backward(cpu_product):
    check_long_run_backward()


def test_second_scan_trip(cpu_product):
    check_second_scan_trip()


def test_records_are_read_inside_their_array():
    """tests/gather_guard_child.py runs check_records_are_read_inside_their_array in a process of its own: a read outside the records ends that process,
    not the suite."""
    import subprocess
    import sys
    r = subprocess.run([sys.executable, '-m', 'tests.gather_guard_child'], cwd=G.ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=900)
    assert r.returncode == 0 and b'records stayed inside' in r.stdout, (r.returncode, r.stdout.decode()[-2000:])
