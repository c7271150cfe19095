"""csrc/sample.hip and the two searches of csrc/common.h on edge geometry: the cell lists, the near mask and near lists, the shell mask with its nearest
vertex and compaction, and the warp's T-vertex search, called through the C ABI on SYNTHETIC scenes placed by construction (no rendered frame), against
brute force in the kernels' own fp32 arithmetic:

  * depths near + fl(fl(k / (S - 1)) * fl(far - near)), positions o + fl(t d) with separate roundings, (x - Th) @ R in to_smpl_frame's order,
    d^2 = ((dx dx) + (dy dy)) + (dz dz) without fma; a sample is valid iff min d^2 < fp32(0.05 * 0.05), its vertex the lowest id among the minima.

Every comparison is EXACT (bits): counters, ray_cnt, ray_base, cs_idx, cs_vid, cs_xs, cs_tvid, cell_start, cell_pts.  Every output buffer is filled with
a sentinel first; it must survive behind what a call may write.  Every case asserts from the grid header, the launch arithmetic restated here or the
brute force that it reached the branch it is about (`Grid.path`, `launch_path`, `nn_path`, the tie counts of `flat`, the bands of the grazing rays).

The `check_*` bodies run on the HOST build of the unchanged kernel sources below and on the MI355X in tests/test_gpu_sampler_edges.py."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from sherf_amd import _lib
from tests import gpu_common as G
from tests.test_hipcpu_frame import cpu_product          # noqa: F401  (the host builds behind sherf_amd._lib, CPU tensors)
from tests.test_hipcpu_gather_edges import _sync, debug_bits, experiment
from tests.test_hipcpu_nn import _d2, _points

F = np.float32
MAX_CELLS, NSUB, MASK_WORDS = 64 * 64 * 64, 524288, 32768
CELL_SIZE = 0.05
THRESH2 = F(0.05 * 0.05)
LDS_CELLS, LDS_POINTS = 24576, 8192                      # build_cells_body: cell counters / points of its LDS path
SENT, FSENT = -1234567, -7.5
GUARD = 64                                               # sentinel words / rows around and behind the outputs
R0, S0 = 97, 65                                          # the standard shape


# ---- 1. the kernels' arithmetic in numpy (fp32, one rounding per operation) -------------------------------------------------------------------
def to_smpl(x, Rm, Th):
    """(x - Th) @ R as to_smpl_frame evaluates it: ((a0 R0c + a1 R1c) + a2 R2c)"""
    a = (x.astype(F) - Th.astype(F)).astype(F)
    return np.stack([((a[:, 0] * Rm[0, c] + a[:, 1] * Rm[1, c]).astype(F) + a[:, 2] * Rm[2, c]).astype(F) for c in range(3)], 1)


def depths(near, far, S):
    step = (np.arange(S, dtype=F) / F(S - 1)).astype(F)
    return (near[:, None] + (step[None, :] * (far - near).astype(F)[:, None]).astype(F)).astype(F)


def f2ord(f):
    i = int(np.array(f, F).view(np.int32))
    return i if i >= 0 else i ^ 0x7FFFFFFF


def brute(pts, xs):
    """-> (min d^2 [N], lowest id among the minima, number of minima).  Large problems are cut down by what cannot change the answer: samples are taken in
    order of x, a chunk of them against the points of its slab widened by 5.1 cm -- a point outside it is farther than 5.1 cm from every sample of the chunk, so
    validity, the vertex of a valid sample and every d^2 below 0.051^2 are those of the full brute force (min d^2 = inf: no point in the slab)."""
    N, n = len(xs), len(pts)
    best, vid, ntie = np.full(N, np.inf, F), np.full(N, -1, np.int64), np.zeros(N, np.int64)
    slabs = N * n > 20_000_000
    order = np.argsort(xs[:, 0], kind='stable') if slabs else np.arange(N)
    by_x = np.argsort(pts[:, 0], kind='stable')
    px = pts[by_x, 0].astype(np.float64)
    chunk = 256 if slabs else max(1, 4_000_000 // n)
    for a in range(0, N, chunk):
        i = order[a:a + chunk]
        if slabs:
            lo, hi = np.searchsorted(px, [float(xs[i, 0].min()) - 0.051, float(xs[i, 0].max()) + 0.051])
            cand = np.sort(by_x[lo:hi])                              # (ascending ids: argmin's first = the lowest id)
            if not len(cand):
                continue
        else:
            cand = np.arange(n)
        d2 = _d2(xs[i], pts[cand])
        best[i], vid[i] = d2.min(1), cand[d2.argmin(1)]
        ntie[i] = (d2 == best[i][:, None]).sum(1)
    return best, vid, ntie


# ---- 2. the scenes: points in the SMPL frame, posed into the world by a seeded rotation and translation ------------------------------------------
def _rotation(rs):
    q, _ = np.linalg.qr(rs.normal(size=(3, 3)))
    if np.linalg.det(q) < 0:
        q[:, 0] *= -1
    return q


def _box(rs, n, ext, hole=0.15):
    """n points: uniform in a box of extent `ext` around 0 but for a hole around its centre; two opposite corners; the isolated vertex at the centre"""
    ext = np.array(ext, np.float64)
    p = rs.uniform(-0.5, 0.5, (2 * n, 3)) * ext
    p = p[np.linalg.norm(p, axis=1) > hole][:n - 3]
    return np.concatenate([p, [-ext / 2], [ext / 2], [[0.0, 0.0, 0.0]]])


LATTICE, PITCH, N_DUP = 40, 2.0 ** -6, 30


def _flat(rs):
    """A 40 x 40 lattice in z = 0 with pitch 2^-6, ids shuffled; 30 exact duplicates with higher ids; an isolated vertex in the plane beside it."""
    ij = np.stack(np.meshgrid(np.arange(LATTICE), np.arange(LATTICE), indexing='ij'), -1).reshape(-1, 2)
    ij = ij[rs.permutation(len(ij))]
    lat = np.concatenate([(ij - LATTICE // 2) * PITCH, np.zeros((len(ij), 1))], 1)
    dup = lat[rs.choice(len(lat), N_DUP, replace=False)]
    return np.concatenate([lat, dup, [[(LATTICE // 2 + 13) * PITCH, 0.0, 0.0]]]), ij


_SCENES = {}


def scene(name):
    if name in _SCENES:
        return _SCENES[name]
    seed = sorted(['body', 'wide', 'wider', 'long', 'many', 'most', 'few1', 'few2', 'few3', 'flat', 'flat_posed']).index(name)
    rs = np.random.RandomState(100 + seed)
    sc = SimpleNamespace(name=name, lattice=None)
    shell = {'body': 900, 'many': 9000, 'most': 65535}
    if name in shell:                                    # the shell of test_hipcpu_nn with its cluster; the isolated vertex inside it
        p = np.concatenate([_points(rs, shell[name] - 1).astype(np.float64), [[0.0, 0.0, 0.0]]])
    elif name == 'wide':
        p = _box(rs, 3000, (1.6, 1.6, 1.6))
    elif name == 'wider':
        p = _box(rs, 3000, (2.2, 2.2, 2.2))
    elif name == 'long':
        p = _box(rs, 2000, (4.0, 0.4, 0.4))
    elif name in ('flat', 'flat_posed'):
        p, sc.lattice = _flat(rs)
    elif name == 'few1':
        p = np.array([[0.1, 0.2, 0.3]])
    elif name == 'few2':
        p = np.array([[0.1, 0.2, 0.3], [0.1, 0.21, 0.3]])
    elif name == 'few3':
        p = np.array([[0.1, 0.2, 0.3]]) + np.arange(3)[:, None] * np.array([[0.02, 0.02, 0.0]])
    sc.n = len(p)
    sc.iso = sc.n - 1 if sc.n > 3 else 0                 # the vertex the grazing rays pass
    others = np.delete(p, sc.iso, 0)
    away = p[sc.iso] - others.mean(0) if len(others) and name.startswith(('few', 'flat')) else rs.normal(size=3)
    sc.graze_u = away / np.linalg.norm(away)
    if name == 'flat':                                   # the ties need exact coordinates: Rg = I, Th = 0
        Rg, Th = np.eye(3), np.zeros(3)
    else:
        Rg, Th = _rotation(rs), rs.uniform(-0.3, 0.3, 3)
    sc.Rg, sc.Th = Rg.astype(F), Th.astype(F)
    sc.verts_b = p.astype(F)                                                        # set 1: untransformed
    sc.verts_a = (sc.verts_b.astype(np.float64) @ sc.Rg.astype(np.float64).T + sc.Th).astype(F)   # set 0: posed; the kernel takes it back
    sc.pts = to_smpl(sc.verts_a, sc.Rg, sc.Th)                                       # what the cell list of set 0 must hold
    if name == 'flat':
        assert np.array_equal(sc.pts, sc.verts_b)
    _SCENES[name] = sc
    return sc


# ---- 3. the cell lists through the C ABI ------------------------------------------------------------------------------------------------------------
def _t(a):
    return G.dev_tensor(torch.from_numpy(np.ascontiguousarray(a)))


def _full(shape, value, dtype):
    return G.dev_tensor(torch.full(shape if isinstance(shape, tuple) else (shape,), value, dtype=dtype))


def _header(h):
    h = G.plain(h).contiguous()
    g = SimpleNamespace(o=h[:3].numpy().copy(), cell=F(float(h[3])), inv=F(float(h[4])))
    g.dims = [int(v) for v in h[5:8].view(torch.int32)]
    g.sub = int(h[8:9].view(torch.int32))
    g.ncell = g.dims[0] * g.dims[1] * g.dims[2]
    return g


def cell_of(g, p, clamp=True):
    """The cell index of points p [N,3] with the kernel's floorf: (int)floorf((p - o) * inv)"""
    c = np.floor(((p.astype(F) - g.o).astype(F) * g.inv).astype(F)).astype(np.int64)
    return np.clip(c, 0, np.array(g.dims) - 1) if clamp else c


class Grid:
    """Both cell lists of a scene (sherf_build_cells2; `single`: set 0 alone through sherf_build_cells) and the near lists of set 0."""

    def __init__(self, sc, single=False):
        p, n = _lib.ptr, sc.n
        self.sc, self.single = sc, single
        self.va, self.vb, self.Rg, self.Th = _t(sc.verts_a), _t(sc.verts_b), _t(sc.Rg), _t(sc.Th)
        self.hdr = _full((2, 12), FSENT, torch.float32)
        self.cell_start = _full((2, MAX_CELLS + 1), SENT, torch.int32)
        self.cell_pts = _full((2 * n + GUARD, 4), FSENT, torch.float32)
        self.scratch = _full(10 * n + GUARD, SENT, torch.int32)
        self.mask_buf, self.mask2_buf = (_full(MASK_WORDS + 2 * GUARD, SENT, torch.int32) for _ in range(2))
        self.near_mask, self.mask2 = (b[GUARD:GUARD + MASK_WORDS] for b in (self.mask_buf, self.mask2_buf))
        if single:
            _lib.call('sherf_build_cells', p(self.va), n, p(self.Rg), p(self.Th), CELL_SIZE, p(self.hdr[0]), p(self.cell_start[0]), p(self.cell_pts), p(self.scratch),
                      p(self.near_mask), _lib.stream())
        else:
            _lib.call('sherf_build_cells2', p(self.va), p(self.Rg), p(self.Th), p(self.vb), n, CELL_SIZE, p(self.hdr), p(self.cell_start), p(self.cell_pts), p(self.scratch),
                      p(self.near_mask), _lib.stream())
        self.list_cap = 125 * n + 3 * NSUB
        self.hdr_buf = _full(2 * NSUB + 2 + 2 * GUARD, SENT, torch.int32)
        self.near_hdr = self.hdr_buf[GUARD:GUARD + 2 * NSUB + 2]
        self.near_list = _full(self.list_cap + GUARD, 0x5A5A, torch.int16)
        _lib.call('sherf_build_near_lists', p(self.hdr[0]), p(self.cell_pts), n, CELL_SIZE, p(self.near_hdr), p(self.near_list), self.list_cap, p(self.mask2), _lib.stream())
        _sync()
        self.g = [_header(self.hdr[0])] + ([] if single else [_header(self.hdr[1])])

    def path(self, s=0):
        g = self.g[s]
        return 'lds' if g.ncell + 1 <= LDS_CELLS and self.sc.n <= LDS_POINTS else 'global'


_GRIDS = {}


def grid(name):
    key = (name, G.CPU_SHIM)
    if key not in _GRIDS:
        _GRIDS[key] = Grid(scene(name), single=name.startswith('few'))
    return _GRIDS[key]


#          build path, sub, what else the header must say
EXPECT = {'body': ('lds', 2), 'wide': ('global', 2), 'wider': ('global', 1), 'long': ('lds', 2), 'many': ('global', 2), 'most': ('global', 2), 'flat': ('lds', 2),
          'flat_posed': ('lds', 2), 'few1': ('lds', 2), 'few2': ('lds', 2), 'few3': ('lds', 2)}


def assert_branch(name):
    """The branch of build_cells_body the scene is there for, from the header it wrote."""
    gr = grid(name)
    g, n = gr.g[0], gr.sc.n
    assert (gr.path(0), g.sub) == EXPECT[name], (name, gr.path(0), g.sub, g.dims)
    assert g.sub == (2 if 8 * g.ncell <= 2 ** 19 else 1)
    if name == 'wide':
        assert LDS_CELLS <= g.ncell and 8 * g.ncell <= 2 ** 19 and n <= LDS_POINTS, g.dims
    if name == 'wider':
        assert 8 * g.ncell > 2 ** 19 and g.sub == 1, g.dims
    if name == 'long':
        assert g.cell > F(CELL_SIZE) and max(g.dims) <= 64 and max(g.dims) >= 60, (g.cell, g.dims)
    else:
        assert g.cell == F(CELL_SIZE), g.cell
    if name in ('many', 'most'):
        assert n > LDS_POINTS and g.ncell + 1 <= LDS_CELLS and n == {'many': 9000, 'most': 65535}[name]
    if name.startswith('flat'):
        assert min(g.dims) == 3


def check_cells(name):
    gr = grid(name)
    sc, n = gr.sc, gr.sc.n
    assert_branch(name)
    cp_all, cs_all = G.plain(gr.cell_pts), G.plain(gr.cell_start)
    sets = [(sc.pts, 0)] if gr.single else [(sc.pts, 0), (sc.verts_b, 1)]
    for pts, s in sets:
        g = gr.g[s]
        cp = cp_all[s * n:(s + 1) * n]
        ids = cp[:, 3].contiguous().view(torch.int32).numpy().astype(np.int64)
        assert np.array_equal(np.sort(ids), np.arange(n)), (name, s, 'ids are not a permutation')
        assert np.array_equal(cp[:, :3].numpy().view(np.int32), pts[ids].view(np.int32)), (name, s, 'positions')
        # header: cell >= cell_size, dims <= 64, every point one cell inside on the low side and inside on the high side
        assert g.cell >= F(CELL_SIZE) and max(g.dims) <= 64 and min(g.dims) >= 3, (name, s, g.dims)
        raw = cell_of(g, pts, clamp=False)
        assert (raw >= 1).all() and (raw <= np.array(g.dims) - 1).all(), (name, s, raw.min(0), raw.max(0), g.dims)
        c = cell_of(g, pts)
        flat = (c[:, 2] * g.dims[1] + c[:, 1]) * g.dims[0] + c[:, 0]
        counts = np.bincount(flat, minlength=g.ncell)
        start = cs_all[s, :g.ncell + 1].numpy()
        assert np.array_equal(start, np.concatenate([[0], np.cumsum(counts)])) and start[-1] == n, (name, s, 'cell_start')
        assert np.array_equal(flat[ids], np.repeat(np.arange(g.ncell), counts)), (name, s, 'a point sits in the wrong cell')
        assert bool((cs_all[s, g.ncell + 1:] == SENT).all()), (name, s, 'cell_start written behind its last entry')
    assert bool((cp_all[len(sets) * n:] == FSENT).all()) and bool((G.plain(gr.scratch)[10 * n:] == SENT).all())
    if gr.single:
        assert bool((G.plain(gr.hdr)[1] == FSENT).all())
    check_near_lists(gr)


def check_near_lists(gr):
    """must <= list <= may per sub-cell, lists packed without overlap on multiples of four, mask bit <=> list not empty, the mask == sherf_build_cells2's own."""
    g, n, name = gr.g[0], gr.sc.n, gr.sc.name
    sn = [d * g.sub for d in g.dims]
    nsub = sn[0] * sn[1] * sn[2]
    cs = float(g.cell) / g.sub
    assert nsub <= NSUB
    for buf, words in ((gr.mask_buf, MASK_WORDS), (gr.mask2_buf, MASK_WORDS), (gr.hdr_buf, 2 * NSUB + 2)):
        b = G.plain(buf)
        assert bool((b[:GUARD] == SENT).all()) and bool((b[GUARD + words:] == SENT).all()), (name, 'a guard word was written')
    assert bool((G.plain(gr.near_list)[gr.list_cap:] == 0x5A5A).all())
    nh = G.plain(gr.near_hdr)
    hq = nh[:2 * NSUB].view(NSUB, 2).numpy()
    start, count = hq[:nsub, 0].astype(np.int64), hq[:nsub, 1].astype(np.int64)
    assert not hq[nsub:].any() and (start % 4 == 0).all() and (count >= 0).all()
    mask, mask2 = G.plain(gr.near_mask).numpy(), G.plain(gr.mask2).numpy()
    bits = np.unpackbits(mask.view(np.uint8), bitorder='little')[:nsub].astype(bool)
    assert np.array_equal(bits, count > 0), (name, 'mask bit <=> list not empty')
    assert np.array_equal(mask2[:(nsub + 31) // 32], mask[:(nsub + 31) // 32]) and not np.unpackbits(mask.view(np.uint8), bitorder='little')[nsub:].any()
    padded = (count + 3) // 4 * 4
    full = np.flatnonzero(count > 0)
    order = full[np.argsort(start[full], kind='stable')]
    assert (start[order][1:] == (start[order] + padded[order])[:-1]).all() and (not len(order) or start[order][0] == 0), (name, 'lists overlap or leave gaps')
    assert int(nh[2 * NSUB]) == int(padded.sum()) and int(padded.sum()) <= gr.list_cap
    rs = np.random.RandomState(7)
    empty = np.flatnonzero(count == 0)
    sel = full if len(full) <= 20000 else np.concatenate([rs.choice(full, 2000, replace=False), rs.choice(empty, min(500, len(empty)), replace=False)])
    pts = G.plain(gr.cell_pts)[:n, :3].numpy().astype(np.float64)                 # (list entries index cell_pts)
    lst = G.plain(gr.near_list).numpy().view(np.uint16)
    by_x = np.argsort(pts[:, 0], kind='stable')                                    # (only the points within 6 cm of a sub-cell's box on every axis can be in its list)
    px, total = pts[by_x, 0], 0
    for q in sel.tolist():
        b0 = g.o.astype(np.float64) + np.array([q % sn[0], (q // sn[0]) % sn[1], q // (sn[0] * sn[1])]) * cs
        lo, hi = np.searchsorted(px, [b0[0] - 0.06, b0[0] + cs + 0.06])
        cand = by_x[lo:hi]
        cand = cand[(np.abs(pts[cand, 1:] - (b0[1:] + cs / 2)) < cs / 2 + 0.06).all(1)]
        e = np.maximum(np.maximum(b0 - pts[cand], pts[cand] - (b0 + cs)), 0.0)
        dist = np.sqrt((e ** 2).sum(1))
        mine = lst[start[q]:start[q] + count[q]].astype(np.int64)
        assert len(set(mine.tolist())) == len(mine), (name, q, 'a vertex twice in one list')
        must, may = set(cand[dist < CELL_SIZE].tolist()), set(cand[dist < CELL_SIZE + 2e-3 * cs].tolist())
        assert must <= set(mine.tolist()) <= may, (name, q)
        total += len(mine)
    assert total >= min(n, 100)


# ---- 4. rays, placed in the SMPL frame and posed like the vertices -------------------------------------------------------------------------------
N_HALO, N_GRAZE, N_MISS, N_INSIDE = 18, 6, 4, 4
GRAZE_E = (-2e-6, -1e-6, -3e-7, 3e-7, 1e-6, 2e-6)
KINDS = ('through', 'halo', 'graze', 'miss', 'inside')


def _unit(v):
    return v / np.linalg.norm(v)


def build_rays(sc, R, S, only_miss=False):
    """-> world-frame ray_o, ray_d, near, far (fp32), kind [R] (index into KINDS), halo_axis [R] (axis, -1 / +1: side; 0 elsewhere)"""
    rs = np.random.RandomState(1000 + 7 * R + S)
    pts = sc.pts.astype(np.float64)
    lo, hi = pts.min(0), pts.max(0)
    k0 = (S - 1) // 2
    o, d, nr, fr, kind, side = [], [], [], [], [], []

    def add(oo, dd, n_, f_, kd, sd=(0, 0)):
        o.append(oo); d.append(dd); nr.append(n_); fr.append(f_); kind.append(KINDS.index(kd)); side.append(sd)

    def anchored(c, dd, kd, sd=(0, 0), n_=0.3, f_=0.9):   # sample k0 of the ray sits at c
        t0 = float(depths(np.array([n_], F), np.array([f_], F), S)[0, k0])
        add(c - t0 * dd, dd, n_, f_, kd, sd)

    total = max(R, R0)
    if not only_miss:
        for a in range(3):                                 # halo: beside each face of the bounding box, through the point that defines the face
            for sgn, ext in ((-1, lo), (1, hi)):
                v = pts[np.argmin(pts[:, a]) if sgn < 0 else np.argmax(pts[:, a])]
                for delta in (0.01, 0.03, 0.049):
                    c = v.copy(); c[a] = ext[a] + sgn * delta
                    anchored(c, np.eye(3)[(a + 1) % 3], 'halo', (a, sgn))
        for e in GRAZE_E:                                  # grazing: past the isolated vertex at 0.05 + e
            dd = rs.normal(size=3)
            dd = _unit(dd - dd.dot(sc.graze_u) * sc.graze_u)
            anchored(pts[sc.iso] + (0.05 + e) * sc.graze_u, dd, 'graze')
        diag = float(np.linalg.norm(hi - lo))
        for i in range(N_INSIDE):                          # start inside the grid and leave it
            add(pts[rs.randint(sc.n)] + rs.uniform(-0.01, 0.01, 3), _unit(rs.normal(size=3)), 0.0, diag + 1.0, 'inside')
    for i in range(N_MISS if not only_miss else total):    # miss the grid entirely (one of them with negative depths)
        add(hi + np.array([10.0, 0, 0]) + rs.uniform(-1, 1, 3), _unit(np.array([1.0, 0, 0]) + rs.uniform(-0.2, 0.2, 3)), -0.5 if i == 1 else 0.5, 0.5 if i == 1 else 1.5, 'miss')
    n_through = total - len(o)
    if sc.lattice is not None and sc.name == 'flat' and n_through:
        # the tie rays: parallel to z through the centres (40) and edge midpoints (the rest) of lattice squares; the first 15 at squares with a duplicated vertex
        ij = sc.lattice
        dup_xy = np.round(sc.verts_b[len(ij):len(ij) + N_DUP, :2].astype(np.float64) / PITCH).astype(int)
        sq = np.concatenate([np.clip(dup_xy[:15], -LATTICE // 2, LATTICE // 2 - 2), rs.randint(-LATTICE // 2, LATTICE // 2 - 1, (n_through - 15, 2))])
        for i, (a, b) in enumerate(sq):
            off = (0.5, 0.5) if i < 40 else ((0.5, 0.0) if i % 2 else (0.0, 0.5))
            add(np.array([(a + off[0]) * PITCH, (b + off[1]) * PITCH, -0.5]), np.array([0.0, 0.0, 1.0]), 0.4, 0.6, 'through')
    else:
        for i in range(n_through):                         # through the points
            dd = _unit(rs.normal(size=3))
            anchored(pts[rs.randint(sc.n)] + rs.uniform(-0.015, 0.015, 3), dd, 'through', n_=0.55, f_=1.45)
    o, d, kind, side = np.array(o), np.array(d), np.array(kind), np.array(side)
    perm = rs.permutation(len(o))
    if not only_miss:                                      # a ray through the points comes first: every prefix holds valid samples
        first = np.flatnonzero(kind[perm] == 0)[0]
        perm[[0, first]] = perm[[first, 0]]
    perm = perm[:R]
    Rm = sc.Rg.astype(np.float64)
    exact = sc.name == 'flat'
    ow = o[perm] if exact else o[perm] @ Rm.T + sc.Th.astype(np.float64)
    dw = d[perm] if exact else d[perm] @ Rm.T
    return SimpleNamespace(o=ow.astype(F), d=dw.astype(F), near=np.array(nr, F)[perm], far=np.array(fr, F)[perm], kind=kind[perm], side=side[perm], R=R, S=S)


_REFS = {}


def reference(name, R=R0, S=S0, only_miss=False):
    """Rays + brute force of (scene, R, S), once; the conditions on the inputs are asserted here, from the brute force alone, before any kernel runs."""
    key = (name, R, S, only_miss)
    if key in _REFS:
        return _REFS[key]
    sc = scene(name)
    ry = build_rays(sc, R, S, only_miss)
    t = depths(ry.near, ry.far, S)
    x = (ry.o[:, None, :] + (t[..., None] * ry.d[:, None, :]).astype(F)).astype(F).reshape(-1, 3)
    xs = to_smpl(x, sc.Rg, sc.Th)
    best, vid, ntie = brute(sc.pts, xs)
    ok = best < THRESH2
    valid = np.flatnonzero(ok)
    cnt = np.bincount(valid // S, minlength=R)
    ref = SimpleNamespace(rays=ry, xs=xs, best=best, vid=vid, ntie=ntie, valid=valid, nv=valid.size, cnt=cnt, base=np.concatenate([[0], np.cumsum(cnt)[:-1]]),
                          tmin=f2ord(min(t[:, 0].min(), t[:, S - 1].min())), tmax=f2ord(max(t[:, 0].max(), t[:, S - 1].max())))
    per_ray = ok.reshape(R, S)
    if only_miss:
        assert ref.nv == 0
    else:
        assert ref.nv > 0 and per_ray[0].any()
        assert not per_ray[ry.kind == KINDS.index('miss')].any()
        assert per_ray[ry.kind == KINDS.index('halo')].any(1).all(), (name, R, S, 'a halo ray without a valid sample')
    if R >= R0 and not only_miss:
        kinds = np.bincount(ry.kind, minlength=5)
        assert (kinds[1:] == (N_HALO, N_GRAZE, N_MISS, N_INSIDE)).all() and kinds[0] > 0, kinds
        inside = per_ray[ry.kind == KINDS.index('inside')]
        assert not inside[:, -1].any()                     # (left the shell; the last samples lie beyond the points' box)
        band = np.abs(np.sqrt(best.astype(np.float64)) - 0.05) < 1e-5
        graze = np.repeat(ry.kind == KINDS.index('graze'), S)
        assert (band & graze & ok).any() and (band & graze & ~ok).any(), (name, R, S, 'the grazing rays do not straddle the threshold')
    _REFS[key] = ref
    return ref


# ---- 5. sherf_sample_mask_nn ---------------------------------------------------------------------------------------------------------------------------
#         form      SHERF_EXPERIMENT  debug word  near lists
FORMS = {'lists':  (0,                0,          True),
         'walk':   (0,                0,          False),
         'dbg14':  (0,                1 << 14,    True),
         'wave':   (0,                1 << 9,     True),
         'x2048':  (2048,             0,          True),
         'x8192':  (8192,             0,          True),
         'x16384': (16384,            0,          True),
         'x24576': (24576,            0,          True),
         'x49152': (49152,            0,          True)}
BIG_FORMS = ('lists', 'walk', 'wave')
SHAPE_FORMS = ('lists', 'wave', 'x2048', 'x8192')


def launch_path(form, R, S, capacity):
    """sherf_sample_mask_nn_impl's dispatch restated: -> (search kernel, compaction kernel)"""
    xp, dbg, lists = FORMS[form]
    nch = (S + 63) // 64
    if (dbg & 512) or capacity < R * S:
        search = 'sample_nn'
    elif not lists or (dbg & 16384):
        search = 'cand_search'
    else:
        search = {0: 'cand_search_lists', 16384: 'cand_search_lists2<5>', 49152: 'cand_search_lists2<6>'}[xp & 49152]
    compact = 'compact_quad' if (xp & 8192) and nch != 3 else ('compact_rays' if xp & 2048 else 'compact')
    return search, compact


def run_sampler(gr, ry, form, capacity=None):
    xp, dbg, lists = FORMS[form]
    p, R, S = _lib.ptr, ry.R, ry.S
    cap = R * S if capacity is None else capacity
    nch = (S + 63) // 64
    ws = R + R // 1024 + 2
    o = SimpleNamespace(cap=cap, two_pass=launch_path(form, R, S, cap)[0] != 'sample_nn')
    o.counters = _full(4 + GUARD, SENT, torch.int32)
    o.ray_base, o.ray_cnt = _full(R + GUARD, SENT, torch.int32), _full(R + GUARD, SENT, torch.int32)
    o.cs_idx, o.cs_vid = _full(cap + GUARD, SENT, torch.int32), _full(cap + GUARD, SENT, torch.int32)
    o.cs_xs = _full((cap + GUARD, 4), FSENT, torch.float32)
    o.dense_vid, o.ray_mask, o.scan_ws = _full(R * S + GUARD, SENT, torch.int32), _full(R * nch + GUARD, SENT, torch.int64), _full(ws + GUARD, SENT, torch.int32)
    rays = [_t(a) for a in (ry.o, ry.d, ry.near, ry.far)]
    with experiment(xp), debug_bits(dbg):
        _lib.call('sherf_sample_mask_nn', *(p(a) for a in rays), R, S, p(gr.Rg), p(gr.Th), p(gr.hdr[0]), p(gr.cell_start[0]), p(gr.cell_pts), p(gr.near_mask), cap,
                  p(o.counters), p(o.ray_base), p(o.ray_cnt), p(o.cs_idx), p(o.cs_vid), p(o.cs_xs), p(o.dense_vid), p(o.ray_mask), p(o.scan_ws),
                  p(gr.near_hdr) if lists else None, p(gr.near_list) if lists else None, _lib.stream())
        _sync()
    for k in ('counters', 'ray_base', 'ray_cnt', 'cs_idx', 'cs_vid', 'cs_xs', 'dense_vid', 'ray_mask', 'scan_ws'):
        setattr(o, k, G.plain(getattr(o, k)))
    return o


def assert_sampler(label, o, ref, R, S):
    nv, cap = ref.nv, o.cap
    m = min(nv, cap)
    assert int(o.counters[0]) == nv, (label, int(o.counters[0]), nv)
    assert (int(o.counters[1]), int(o.counters[2])) == (ref.tmin, ref.tmax) and int(o.counters[3]) == 0, label
    assert np.array_equal(o.ray_cnt[:R].numpy(), ref.cnt) and np.array_equal(o.ray_base[:R].numpy(), ref.base), label
    assert np.array_equal(o.cs_idx[:m].numpy(), ref.valid[:m]), label
    assert np.array_equal(o.cs_vid[:m].numpy(), ref.vid[ref.valid[:m]]), label
    assert np.array_equal(o.cs_xs[:m, :3].numpy().view(np.int32), ref.xs[ref.valid[:m]].view(np.int32)) and bool((o.cs_xs[:m, 3] == 0).all()), label
    # the sentinel behind what the call may write (cs_xs doubles as the two-pass form's candidate list, `capacity` records: only its guard survives there)
    assert bool((o.counters[4:] == SENT).all()) and bool((o.ray_base[R:] == SENT).all()) and bool((o.ray_cnt[R:] == SENT).all()), label
    assert bool((o.cs_idx[m:] == SENT).all()) and bool((o.cs_vid[m:] == SENT).all()), (label, 'records written at or beyond min(nv, capacity)')
    assert bool((o.cs_xs[cap if o.two_pass else m:] == FSENT).all()), label
    assert bool((o.scan_ws[R + R // 1024 + 2:] == SENT).all()) and bool((o.dense_vid[R * S:] == SENT).all()), label
    assert bool((o.ray_mask[R * ((S + 63) // 64):] == SENT).all()), label


def check_sampler(name, R=R0, S=S0, forms=('lists',)):
    ref = reference(name, R, S)
    gr = grid(name)
    if name in EXPECT:
        assert_branch(name)
    for form in forms:
        assert_sampler(f'{name} R={R} S={S} {form} {launch_path(form, R, S, R * S)}', run_sampler(gr, ref.rays, form), ref, R, S)
    return ref


S_CASES = (2, 63, 64, 65, 128, 129, 192, 193, 256)
R_CASES = (1, 3, 5, 17, 255, 1023, 1025, 2500)
FORM_S = (65, 129, 193, 256)


def check_shape_S(S):
    assert (S + 63) // 64 == {2: 1, 63: 1, 64: 1, 65: 2, 128: 2, 129: 3, 192: 3, 193: 4, 256: 4}[S]
    check_sampler('body', R0, S, SHAPE_FORMS)


def check_shape_R(R):
    """R ragged against the 4 (sample_nn, compact), 16 (compact_quad), 16 / nch x 4 (cand_mark), 256 (compact_rays) and 1024 (scans) rays per workgroup."""
    ref = check_sampler('body', R, S0, SHAPE_FORMS)
    if R == 2500:
        cum = np.concatenate([[0], np.cumsum(ref.cnt)])
        assert all(ref.cnt[a:a + 1024].sum() > 0 for a in (0, 1024, 2048)) and 0 < cum[1024] < cum[2048] < cum[R - 1] <= ref.nv
        assert (ref.base[1024], ref.base[2048], ref.base[-1]) == (cum[1024], cum[2048], cum[R - 1])


def check_forms(name, S):
    """All nine search and compaction forms, each asserted from the dispatch restated in launch_path."""
    nch = (S + 63) // 64
    paths = {form: launch_path(form, R0, S, R0 * S) for form in FORMS}
    assert paths['lists'] == ('cand_search_lists', 'compact') and paths['walk'] == paths['dbg14'] == ('cand_search', 'compact') and paths['wave'] == ('sample_nn', 'compact')
    assert paths['x2048'] == ('cand_search_lists', 'compact_rays') and paths['x8192'][1] == ('compact' if nch == 3 else 'compact_quad')
    assert paths['x16384'][0] == 'cand_search_lists2<5>' and paths['x24576'] == ('cand_search_lists2<5>', 'compact_quad' if nch != 3 else 'compact')
    assert paths['x49152'][0] == 'cand_search_lists2<6>'
    check_sampler(name, R0, S, tuple(FORMS))


def check_ties():
    """`flat`: what the brute force says about the ties, then every form (check_forms('flat', 65)) must give the lowest id."""
    ref, sc, gr = reference('flat'), scene('flat'), grid('flat')
    g = gr.g[0]
    d2 = _d2(ref.xs[ref.valid], sc.pts)
    tied = d2 == ref.best[ref.valid][:, None]
    multi = tied.sum(1) > 1
    assert multi.sum() >= 500, multi.sum()
    c = cell_of(g, sc.pts)
    flat = (c[:, 2] * g.dims[1] + c[:, 1]) * g.dims[0] + c[:, 0]
    lo_c, hi_c = np.where(tied, flat[None], 2 ** 40).min(1), np.where(tied, flat[None], -1).max(1)
    assert (multi & (lo_c != hi_c)).sum() >= 100, (multi & (lo_c != hi_c)).sum()
    ids = G.plain(gr.cell_pts)[:sc.n, 3].contiguous().view(torch.int32).numpy()
    pos = np.empty(sc.n, np.int64); pos[ids] = np.arange(sc.n)                      # where a vertex sits in cell_pts
    first = np.where(tied, pos[None], 2 ** 40).argmin(1)                            # the tied vertex the cell order meets first
    assert (multi & (first != ref.vid[ref.valid])).sum() >= 100
    # the duplicates (ids >= LATTICE^2) tie with their originals in some valid samples and never win
    dup = np.arange(LATTICE ** 2, LATTICE ** 2 + N_DUP)
    assert tied[:, dup].any() and not np.isin(ref.vid[ref.valid], dup).any()
    assert ref.ntie[ref.valid].max() >= 4


def check_capacity():
    """capacity = nv - 7 (the one-wave kernel, records truncated, counters[0] the total) and capacity = R S - 1 > nv (the same kernel, everything held)."""
    ref, gr = reference('body'), grid('body')
    full = run_sampler(gr, ref.rays, 'lists')
    assert_sampler('uncapped', full, ref, R0, S0)
    for cap in (ref.nv - 7, R0 * S0 - 1):
        assert (cap < ref.nv) == (cap == ref.nv - 7) and launch_path('lists', R0, S0, cap)[0] == 'sample_nn'
        for form in ('lists', 'x2048', 'x8192'):
            o = run_sampler(gr, ref.rays, form, capacity=cap)
            assert not o.two_pass
            assert_sampler(f'capacity {cap} {form}', o, ref, R0, S0)
            assert torch.equal(o.ray_base[:R0], full.ray_base[:R0]) and torch.equal(o.ray_cnt[:R0], full.ray_cnt[:R0])
            m = min(cap, ref.nv)
            assert torch.equal(o.cs_idx[:m], full.cs_idx[:m]) and torch.equal(o.cs_vid[:m], full.cs_vid[:m]) and torch.equal(o.cs_xs[:m].view(torch.int32), full.cs_xs[:m].view(torch.int32))


def check_nothing_valid():
    ref, gr = reference('body', only_miss=True), grid('body')
    for form in ('lists', 'walk', 'wave', 'x2048', 'x8192'):
        o = run_sampler(gr, ref.rays, form)
        assert_sampler(f'nothing valid {form}', o, ref, R0, S0)
        assert int(o.counters[0]) == 0 and not o.ray_cnt[:R0].any() and not o.ray_base[:R0].any()
        assert bool((o.cs_idx == SENT).all()) and bool((o.cs_vid == SENT).all()) and bool((o.cs_xs == FSENT).all()), form


def check_halo_cells(name):
    """The valid samples of the low-side halo rays sit in the grid's first layer of cells along their axis, those of the high side at or above the last point's."""
    ref, sc, g = reference(name), scene(name), grid(name).g[0]
    top = cell_of(g, sc.pts).max(0)
    for r in np.flatnonzero(ref.rays.kind == KINDS.index('halo')):
        a, sgn = ref.rays.side[r]
        v = ref.valid[ref.valid // S0 == r]
        c = cell_of(g, ref.xs[v], clamp=False)[:, a]
        assert len(v) and ((c == 0).all() if sgn < 0 else ((c >= top[a]) & (c < g.dims[a])).all()), (name, r, a, sgn, c)


def check_refusals():
    """A grid of cells below the sampler's 5 cm shell gave a fraction of the valid samples without a word; its builders refuse one with SHERF_EINVAL (-1), and a list
    without a near mask (the T-vertex search's, any cell_size > 0) is still built."""
    gr, p, L = grid('body'), _lib.ptr, _lib.lib()
    n, fine = gr.sc.n, 0.02
    hdr, cell_start, cell_pts = _full((2, 12), FSENT, torch.float32), _full((2, MAX_CELLS + 1), SENT, torch.int32), _full((2 * n, 4), FSENT, torch.float32)
    scratch, mask = _full(10 * n, SENT, torch.int32), _full(MASK_WORDS, SENT, torch.int32)
    cells2 = lambda cs: L.sherf_build_cells2(p(gr.va), p(gr.Rg), p(gr.Th), p(gr.vb), n, cs, p(hdr), p(cell_start), p(cell_pts), p(scratch), p(mask), _lib.stream())
    cells = lambda cs, m: L.sherf_build_cells(p(gr.vb), n, None, None, cs, p(hdr[1]), p(cell_start[1]), p(cell_pts[n:]), p(scratch), m, _lib.stream())
    lists = lambda r: L.sherf_build_near_lists(p(gr.hdr[0]), p(gr.cell_pts), n, r, p(gr.near_hdr), p(gr.near_list), gr.list_cap, p(gr.mask2), _lib.stream())
    assert cells2(fine) == -1 and cells2(0.0499) == -1 and cells(fine, p(mask)) == -1 and lists(fine) == -1 and cells(0.0, None) == -1
    _sync()
    for t, sent in ((hdr, FSENT), (cell_start, SENT), (cell_pts, FSENT), (scratch, SENT), (mask, SENT)):
        assert bool((G.plain(t) == sent).all()), 'a refused call wrote something'
    assert cells(fine, None) == 0
    _sync()
    g = _header(hdr[1])
    assert g.cell == F(fine) and bool((G.plain(hdr)[0] == FSENT).all())
    # the T-vertex search on that finer grid: the same answers as on the 5 cm grid
    Q = build_queries('body')
    fine_grid = SimpleNamespace(sc=gr.sc, Rg=gr.Rg, vb=gr.vb, hdr=hdr, cell_start=cell_start, cell_pts=cell_pts)
    assert_warp('fine T grid', Q, *run_warp(fine_grid, Q))


# ---- 6. sherf_warp_geom: the nearest T-vertex on grid 1 ----------------------------------------------------------------------------------------------
def nn_path(g, q, rad2):
    """nn_search_batched's choice restated: True where the ball reaches more than 3 x 3 rows of cells (the plain loops of nn_search)."""
    r = (np.sqrt(rad2.astype(F)) * F(1.00001) + F(1e-6)).astype(F)
    rr = (r + F(1e-4) * g.cell).astype(F)
    span = []
    for a in (1, 2):
        c0 = np.floor((((q[:, a] - rr).astype(F) - g.o[a]).astype(F) * g.inv).astype(F)).astype(np.int64)
        c1 = np.floor((((q[:, a] + rr).astype(F) - g.o[a]).astype(F) * g.inv).astype(F)).astype(np.int64)
        span.append(np.minimum(c1, g.dims[a] - 1) - np.maximum(c0, 0))
    return (span[0] > 2) | (span[1] > 2)


_QUERIES = {}


def build_queries(name, nq=2000):
    """-> q [nq,3], same [nq] (the same-index vertex that bounds the ball), ref [nq] (brute force), group [nq]"""
    if (name, nq) in _QUERIES:
        return _QUERIES[(name, nq)]
    sc, g = scene(name), grid(name).g[1]
    rs = np.random.RandomState(len(name) + nq)
    v = sc.verts_b.astype(np.float64)
    lo, hi = v.min(0), v.max(0)
    n_out, n_tie = 300 * nq // 2000, (300 * nq // 2000 if name == 'flat' else 0)
    n_far = 600 * nq // 2000
    n_near = nq - n_out - n_tie - n_far
    q, same, group = [], [], []
    i = rs.randint(0, sc.n, n_near)
    q.append(v[i] + rs.normal(scale=0.01, size=(n_near, 3))); same.append(i); group += ['near'] * n_near
    q.append(v[rs.randint(0, sc.n, n_far)] + rs.normal(scale=0.01, size=(n_far, 3))); same.append(rs.randint(0, sc.n, n_far)); group += ['far'] * n_far
    glo, ghi = g.o.astype(np.float64), g.o.astype(np.float64) + np.array(g.dims) * float(g.cell)
    out = rs.uniform(lo, hi + 1e-9, (n_out, 3))
    for k in range(n_out):                                # outside grid 1 by 0.3 .. 2 cells, on each of the six sides in turn
        a, u = (k % 6) // 2, rs.uniform(0.3, 2.0) * float(g.cell)
        out[k, a] = glo[a] - u if k % 2 == 0 else ghi[a] + u
    q.append(out); same.append(np.full(n_out, -1)); group += ['outside'] * n_out
    if n_tie:                                             # lattice centres: four equidistant vertices, the same-index one among them but not the lowest id
        ab = rs.randint(-LATTICE // 2, LATTICE // 2 - 1, (n_tie, 2))
        q.append(np.concatenate([(ab + 0.5) * PITCH, np.full((n_tie, 1), 0.003)], 1)); same.append(np.full(n_tie, -2)); group += ['tie'] * n_tie
    q, same, group = np.concatenate(q).astype(F), np.concatenate(same), np.array(group)
    ref, d_same = np.empty(nq, np.int64), np.empty(nq, F)
    for a in range(0, nq, 1000):
        d2 = _d2(q[a:a + 1000], sc.verts_b)
        ref[a:a + 1000] = d2.argmin(1)
        sm = same[a:a + 1000]
        nearest = sm == -1                                # outside: every other one the nearest vertex (a small ball), the others a random one
        sm[nearest] = np.where(np.arange(nearest.sum()) % 2 == 0, ref[a:a + 1000][nearest], rs.randint(0, sc.n, nearest.sum()))
        tie = np.flatnonzero(sm == -2)
        if len(tie):
            t = d2[tie] == d2[tie].min(1)[:, None]
            assert (t.sum(1) >= 4).all()
            sm[tie] = np.where(t, np.arange(sc.n)[None], -1).max(1)      # the highest id of the tied
            assert (sm[tie] != ref[a:a + 1000][tie]).all()
        same[a:a + 1000] = sm
        d_same[a:a + 1000] = d2[np.arange(len(sm)), sm]
    plain = nn_path(g, q, d_same)
    assert (np.sqrt(d_same) > 3 * float(g.cell)).mean() > 0.1 and plain.mean() > 0.1 and (~plain).sum() > 100, (name, plain.mean())
    c = cell_of(g, q, clamp=False)
    outside = ((c < 0) | (c >= np.array(g.dims))).any(1)
    assert outside[group == 'outside'].all() and (group == 'outside').sum() >= 6
    _QUERIES[(name, nq)] = SimpleNamespace(q=q, same=same.astype(np.int32), ref=ref, group=group, nq=nq)
    return _QUERIES[(name, nq)]


def run_warp(gr, Q, nv=None, xp=0):
    """sherf_warp_geom with identity T2C / C2S on nv queries (Q repeated periodically) -> geom [nv + GUARD, 8], cs_tvid [nv + GUARD] on the device"""
    p, n = _lib.ptr, gr.sc.n
    nv = Q.nq if nv is None else nv
    rep = lambda t: t if nv == Q.nq else torch.cat([t.repeat((nv // Q.nq,) + (1,) * (t.ndim - 1)), t[:nv % Q.nq]]).contiguous()
    xs = torch.zeros(Q.nq, 4); xs[:, :3] = torch.from_numpy(Q.q)
    ident = torch.zeros(n, 12); ident[:, 0] = ident[:, 4] = ident[:, 8] = 1.0
    ident, rd = _t(ident.numpy()), _t(np.tile(np.array([[0.0, 0.0, 1.0]], F), (nv, 1)))
    counters = _t(np.array([nv, 0, 0, 0], np.int32))
    idx, vid, xs = _t(2 * np.arange(nv, dtype=np.int32)), rep(_t(Q.same)), rep(_t(xs.numpy()))
    geom, tvid = _full((nv + GUARD, 8), FSENT, torch.float32), _full(nv + GUARD, SENT, torch.int32)
    with experiment(xp):
        _lib.call('sherf_warp_geom', p(counters), p(idx), p(vid), p(xs), p(rd), 2, p(gr.Rg), p(ident), p(ident), p(gr.vb), p(gr.hdr[1]), p(gr.cell_start[1]),
                  p(gr.cell_pts[n:]), nv, p(geom), p(tvid), _lib.stream())
        _sync()
    return geom, tvid


def assert_warp(label, Q, geom, tvid, first=0):
    """geom / tvid of queries first .. against the brute force"""
    geom, tvid = G.plain(geom), G.plain(tvid)
    m = tvid.numel() - GUARD
    assert bool((tvid[m:] == SENT).all()) and bool((geom[m:] == FSENT).all()), (label, 'written behind the last sample')
    k = (first + np.arange(m)) % Q.nq
    bad = np.flatnonzero(tvid[:m].numpy() != Q.ref[k])
    assert not len(bad), (label, len(bad), [(int(b), Q.group[k[b]], int(tvid[b]), int(Q.ref[k[b]])) for b in bad[:5]])
    assert np.array_equal(geom[:m, :3].numpy().view(np.int32), Q.q[k].view(np.int32)), label


def check_warp(name):
    gr, Q = grid(name), build_queries(name)
    assert_warp(name, Q, *run_warp(gr, Q))


def n_cus():
    return 2 if G.CPU_SHIM else torch.cuda.get_device_properties(0).multi_processor_count      # (the host build's hipDeviceGetAttribute says 2)


def check_warp_persistent_trips():
    """SHERF_EXPERIMENT = 1 << 16: one persistent workgroup per CU; nv = 256 CUs + 37 makes every workgroup's loop take a second trip (the last one ragged)."""
    gr, Q = grid('body'), build_queries('body')
    cus = n_cus()
    nv = 256 * cus + 37
    grid_wgs = min(1 * cus, -(-nv // 256))               # sherf_warp_geom's launch arithmetic
    assert grid_wgs == cus and -(-nv // (256 * grid_wgs)) >= 2
    assert_warp('persistent', Q, *run_warp(gr, Q, nv=nv, xp=1 << 16))


# ---- the host build -------------------------------------------------------------------------------------------------------------------------------------------
CELL_SCENES = ('body', 'wide', 'wider', 'long', 'many', 'few1', 'few2', 'few3', 'flat', 'flat_posed')
RAY_SCENES = ('wide', 'wider', 'long', 'many', 'few1', 'few2', 'few3', 'flat')


@pytest.mark.parametrize('name', CELL_SCENES)
def test_cell_lists(cpu_product, name):
    check_cells(name)


@pytest.mark.parametrize('name', RAY_SCENES)
def test_scene(cpu_product, name):
    check_sampler(name, forms=BIG_FORMS)
    check_halo_cells(name)


def test_most(cpu_product):
    check_cells('most')
    check_sampler('most', forms=BIG_FORMS)
    check_halo_cells('most')


@pytest.mark.parametrize('S', S_CASES)
def test_samples_per_ray(cpu_product, S):
    check_shape_S(S)


@pytest.mark.parametrize('R', R_CASES)
def test_ray_counts(cpu_product, R):
    check_shape_R(R)


@pytest.mark.parametrize('S', FORM_S)
def test_forms(cpu_product, S):
    check_forms('body', S)
    if S == S0:
        check_halo_cells('body')


def test_ties(cpu_product):
    check_ties()
    check_forms('flat', S0)


def test_capacity(cpu_product):
    check_capacity()


def test_nothing_valid(cpu_product):
    check_nothing_valid()


@pytest.mark.parametrize('name', ('body', 'wide', 'long', 'flat'))
def test_warp(cpu_product, name):
    check_warp(name)


def test_warp_persistent_trips(cpu_product):
    check_warp_persistent_trips()


def test_refusals(cpu_product):
    check_refusals()
