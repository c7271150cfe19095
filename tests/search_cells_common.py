"""Shared by tests/test_hipcpu_search_cells.py (the host build of csrc/sample.hip) and tests/test_gpu_search_cells.py (the library on the device): the edge
geometries of the candidate search by sub-cell (cand_search_cells_kernel), run through sherf_sample_mask_nn_ws twice -- the search by sub-cell and, under
sherf_set_debug bit 28, the search by candidate it replaces -- and against brute force in the kernels' own arithmetic (tests/test_hipcpu_nn.py: fp32, no fma,
d^2 < 0.05^2 strictly, ties to the lower vertex id).

Every case is a function of S -> dict(verts [n,3], o, d [R,3], near, far [R], check=callable(info) asserting that the geometry really is the edge it is named for).
`info` holds what the check may look at: the brute-force d^2 table, the candidates' sub-cells and the near lists' lengths, all derived from the grid header the
library itself wrote."""
import ctypes

import numpy as np
import torch

MAX_CELLS = 64 * 64 * 64
NSUB = 524288
THR = np.float32(0.05 * 0.05)
SEARCH_BY_CANDIDATE = 1 << 28
GUARD, SENT = 64, -1234567
S_VALUES = (64, 80, 128)          # one mask word, two with a ragged second chunk, two full

FUNCS = ('sherf_build_cells2', 'sherf_build_near_lists', 'sherf_sample_mask_nn_ws')


def bind(lib, protos):
    for name in FUNCS:
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = protos[name][0], [a[0] for a in protos[name][1]]
    return lib


def cell_ws_ints(R, S):
    return 4 * NSUB + 6 + 2 * (R * S // 64)           # SHERF_CELL_WS_INTS (include/sherf_hip.h)


def _P(t):
    return ctypes.c_void_p(t.data_ptr())


def d2_table(q, p):
    """[nq,3] x [np,3] -> [nq,np] squared distances exactly as dist2_exact evaluates them (fp32, no fma)."""
    d = (q[:, None, :].astype(np.float32) - p[None, :, :].astype(np.float32)).astype(np.float32)
    sq = (d * d).astype(np.float32)
    return ((sq[..., 0] + sq[..., 1]).astype(np.float32) + sq[..., 2]).astype(np.float32)


def positions(o, d, near, far, S):
    """Sample positions as the sampler evaluates them (math_utils.py:101-118; separate roundings), [R*S, 3]."""
    k = np.arange(S, dtype=np.float32)
    step = (k / np.float32(S - 1)).astype(np.float32)
    t = (near[:, None] + (step[None, :] * (far - near).astype(np.float32)[:, None]).astype(np.float32)).astype(np.float32)
    return (o[:, None, :] + (t[..., None] * d[:, None, :]).astype(np.float32)).astype(np.float32).reshape(-1, 3)


def sub_cells(x, hdr):
    """Sub-cell index per position in cand_mark_kernel's arithmetic (-1 outside the grid), and the number of sub-cells."""
    g = hdr.numpy()
    o, inv = g[:3].astype(np.float32), np.float32(g[4])
    nx, ny, nz, sub = [int(v) for v in hdr[5:9].view(torch.int32)]
    fs = np.float32(inv * np.float32(sub))
    s = np.floor(((x - o[None, :]).astype(np.float32) * fs).astype(np.float32)).astype(np.int64)
    dims = np.array([nx, ny, nz]) * sub
    inside = ((s >= 0) & (s < dims[None, :])).all(1)
    q = (s[:, 2] * dims[1] + s[:, 1]) * dims[0] + s[:, 0]
    return np.where(inside, q, -1), int(dims.prod())


# ---- the cases ------------------------------------------------------------------------------------------------------------------------------------
def _axis_rays(px, py, z0, z1):
    """Rays along +z from z = 0 through (px[i], py[i]) whose samples span [z0, z1]: x and y of every sample are exactly px, py and z exactly t."""
    R = len(px)
    o = np.stack([px, py, np.zeros(R)], 1).astype(np.float32)
    d = np.tile(np.array([0, 0, 1], np.float32), (R, 1))
    return o, d, np.full(R, z0, np.float32), np.full(R, z1, np.float32)


def case_none(S):
    rs = np.random.RandomState(1)
    verts = rs.uniform(-0.15, 0.15, size=(200, 3)).astype(np.float32)
    o, d, near, far = _axis_rays(rs.uniform(2.0, 2.5, 64), rs.uniform(2.0, 2.5, 64), 0.5, 1.5)

    def check(i):
        assert i['ncand'] == 0 and i['nv'] == 0
    return dict(verts=verts, o=o, d=d, near=near, far=far, check=check)


def case_bundle(S):
    """199 parallel rays inside one 1 cm square through a sheet of vertices: several hundred candidates in one sub-cell -- chunks of 64 + 64 + ... + a remainder."""
    rs = np.random.RandomState(2)
    gx, gy = np.meshgrid(np.arange(10) * 0.01, np.arange(10) * 0.01)
    verts = np.stack([gx.ravel(), gy.ravel(), np.full(100, 1.0)], 1).astype(np.float32)
    verts = np.concatenate([verts, rs.uniform(0.3, 0.5, size=(60, 3)).astype(np.float32) + np.array([0, 0, 0.7], np.float32)])
    o, d, near, far = _axis_rays(0.04 + rs.uniform(0, 0.01, 199), 0.04 + rs.uniform(0, 0.01, 199), 0.8, 1.2)

    def check(i):
        c = i['cand_per_q']
        assert c.max() >= 130 and ((c > 128) & (c % 64 != 0)).any(), c.max()
    return dict(verts=verts, o=o, d=d, near=near, far=far, check=check)


def case_clusters(S):
    """Near lists of more than 128, of 65..128 and of at most four vertices (the padding minimum), each with candidates."""
    rs = np.random.RandomState(3)
    a = rs.uniform(-0.005, 0.005, size=(150, 3)) + np.array([0.0, 0.0, 1.0])
    b = rs.uniform(-0.005, 0.005, size=(70, 3)) + np.array([0.5, 0.0, 1.0])
    c = np.array([[1.0, 0.0, 1.0]])
    verts = np.concatenate([a, b, c]).astype(np.float32)
    cx = np.repeat([0.0, 0.5, 1.0], 32)
    o, d, near, far = _axis_rays(cx + rs.uniform(-0.02, 0.02, 96), rs.uniform(-0.02, 0.02, 96), 0.9, 1.1)

    def check(i):
        n = i['list_len_of_cand']
        assert (n > 128).any() and ((n > 64) & (n <= 128)).any() and ((n > 0) & (n <= 4)).any(), np.unique(n)
        assert i['nv'] > 100
    return dict(verts=verts, o=o, d=d, near=near, far=far, check=check)


def case_ties(S):
    """Duplicate vertices, and pairs of vertices exactly equidistant from every sample of a ray (either id order in space): ties go to the lower id."""
    rs = np.random.RandomState(4)
    dlt = np.float32(0.0078125)
    verts = np.array([[0.25, 0.0, 1.0]] * 3 +                                    # ids 0, 1, 2: one point three times
                     [[0.75 - dlt, 0.0, 1.0], [0.75 + dlt, 0.0, 1.0],            # ids 3, 4: left, right of the rays through x = 0.75
                      [1.25 + dlt, 0.0, 1.0], [1.25 - dlt, 0.0, 1.0],            # ids 5, 6: right, left of the rays through x = 1.25
                      [1.75, 0.0, 1.0], [1.75, 0.0, 1.0]], np.float32)            # ids 7, 8: a duplicate pair
    verts = np.concatenate([verts, (rs.uniform(-0.1, 0.1, size=(100, 3)) + np.array([0.25, 0.5, 1.0])).astype(np.float32)])
    px = np.repeat(np.array([0.25, 0.75, 1.25, 1.75], np.float32), 16)
    py = np.tile(np.arange(16, dtype=np.float32) * np.float32(0.001953125) - np.float32(0.015625), 4)
    o, d, near, far = _axis_rays(px, py, 0.9, 1.1)

    def check(i):
        d2 = i['d2']
        best = d2.min(1)
        tied = ((d2 == best[:, None]).sum(1) >= 2) & (best < THR)
        vids = set(i['ref_vid'][tied].tolist())
        assert tied.sum() > 100 and {0, 3, 5, 7} <= vids and not ({1, 2, 4, 6, 8} & vids), vids
    return dict(verts=verts, o=o, d=d, near=near, far=far, check=check)


def _threshold_sample(vz, target):
    """(ox, z): a sample (ox, 0, z) whose d^2 to the vertex (0, 0, vz) is exactly `target` in the kernels' arithmetic."""
    v = np.array([[0.0, 0.0, vz]], np.float32)
    z = np.float32(vz) + np.float32(0.0499)
    zs = [z]
    for _ in range(2000):
        z = np.nextafter(z, np.float32(10.0)); zs.append(z)
    zs = np.array(zs, np.float32)
    for j in range(2000):
        ox = np.float32(j) * np.float32(2.0 ** -17)
        q = np.stack([np.full(zs.size, ox, np.float32), np.zeros(zs.size, np.float32), zs], 1)
        hit = np.flatnonzero(d2_table(q, v)[:, 0] == target)
        if hit.size:
            return float(ox), float(zs[hit[0]])
    raise AssertionError('no sample with the target d^2 found')


def case_threshold(S):
    """Samples whose d^2 to their only vertex is kThresh2 exactly, one float below (valid) and one float above: the test is a strict <."""
    targets = (THR, np.nextafter(THR, np.float32(0)), np.nextafter(THR, np.float32(1)))
    vz = 0.015625                                                        # (small z: the samples' float spacing is far below the 5 cm ball's)
    verts = np.array([[0.0, 0.0, vz], [0.0, 1.0, vz], [0.0, 2.0, vz]], np.float32)
    px, py, near = [], [], []
    for j, tg in enumerate(targets):
        ox, z = _threshold_sample(vz, tg)
        for r in range(21):                                              # sample k = 0 of a ray sits at z = near exactly; the copies start a little later
            px.append(ox); py.append(float(j)); near.append(z + r * 1e-4)
    px.append(0.0); py.append(0.0); near.append(vz)                      # (64 rays)
    R = len(px)
    o = np.stack([px, py, np.zeros(R)], 1).astype(np.float32)
    d = np.tile(np.array([0, 0, 1], np.float32), (R, 1))
    near = np.array(near, np.float32)
    far = (near + np.float32(0.2)).astype(np.float32)

    def check(i):
        best = i['d2'].min(1).reshape(R, S)
        assert best[0, 0] == targets[0] and best[21, 0] == targets[1] and best[42, 0] == targets[2], (best[0, 0], best[21, 0], best[42, 0])
        valid = i['valid_mask'].reshape(R, S)
        assert not valid[0, 0] and valid[21, 0] and not valid[42, 0]
        assert i['is_cand'].reshape(R, S)[[0, 21, 42], 0].all()
    return dict(verts=verts, o=o, d=d, near=near, far=far, check=check)


def case_corners(S):
    """Candidates in sub-cell 0 and in the last sub-cell of the grid: beyond the bounding box's two extreme vertices, along the diagonal."""
    rs = np.random.RandomState(6)
    E = 0.05 * 6.96                                                      # the upper corner sits 0.96 of a cell into its cell: the last sub-cell is within 5 cm of it
    verts = np.concatenate([[[0.0, 0.0, 1.0]], [[E, E, 1.0 + E]], rs.uniform(0.05, E - 0.05, size=(100, 3)) + np.array([0, 0, 1.0])]).astype(np.float32)
    lo = np.array([0.0, 0.0, 1.0]) - 0.027
    hi = np.array([E, E, 1.0 + E]) + 0.028
    px = np.concatenate([lo[0] + rs.uniform(-0.001, 0.001, 32), hi[0] + rs.uniform(-0.0005, 0.0005, 32)])
    py = np.concatenate([lo[1] + rs.uniform(-0.001, 0.001, 32), hi[1] + rs.uniform(-0.0005, 0.0005, 32)])
    o, d, _, _ = _axis_rays(px, py, 0, 0)
    near = np.concatenate([np.full(32, lo[2] - 0.03), np.full(32, hi[2] - 0.03)]).astype(np.float32)
    far = (near + np.float32(0.06)).astype(np.float32)

    def check(i):
        c = i['cand_per_q']
        assert c[0] > 0 and c[i['nsub'] - 1] > 0, (c[0], c[i['nsub'] - 1])
        q = i['q'][i['valid_mask']]
        assert (q == 0).any() and (q == i['nsub'] - 1).any()
    return dict(verts=verts, o=o, d=d, near=near, far=far, check=check)


def case_slab(S):
    """Every sample of a workgroup's rays is a candidate: more than pass 1 stages per workgroup (2048), so waves append their share directly."""
    gx, gy = np.meshgrid(np.arange(20) * 0.01, np.arange(20) * 0.01)
    verts = np.stack([gx.ravel(), gy.ravel(), np.full(400, 1.0)], 1).astype(np.float32)
    rs = np.random.RandomState(7)
    o, d, near, far = _axis_rays(rs.uniform(0.05, 0.15, 64), rs.uniform(0.05, 0.15, 64), 0.97, 1.03)

    def check(i):
        rays_per_wg = 64 if S <= 64 else 32                              # cand_mark_kernel: 4 waves x 16 / ceil(S / 64) rays
        per_wg = i['is_cand'].reshape(64, S).sum(1).reshape(-1, rays_per_wg).sum(1)
        assert per_wg.max() > 2048, per_wg
    return dict(verts=verts, o=o, d=d, near=near, far=far, check=check)


CASES = dict(none=case_none, bundle=case_bundle, clusters=case_clusters, ties=case_ties, threshold=case_threshold, corners=case_corners, slab=case_slab)


# ---- the runner ------------------------------------------------------------------------------------------------------------------------------------
def run_case(lib, set_debug, dev, name, S, sync=lambda: None):
    c = CASES[name](S)
    verts_np, o, d, near, far = c['verts'], c['o'], c['d'], c['near'], c['far']
    n, R = verts_np.shape[0], o.shape[0]
    nch = (S + 63) // 64
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    Z = lambda *shape, dtype=torch.int32: torch.zeros(*shape, dtype=dtype, device=dev)
    verts, Rg, Th = T(verts_np), torch.eye(3).contiguous().to(dev), torch.zeros(3).to(dev)
    hdr, cell_start, cell_pts = Z(2, 12, dtype=torch.float32), Z(2, MAX_CELLS + 1), Z(2, n, 4, dtype=torch.float32)
    scratch, near_mask = Z(2 * 5 * n), Z(32768)
    near_hdr, near_list = Z(2 * NSUB + 2), Z(125 * n + 3 * NSUB, dtype=torch.int16)
    assert lib.sherf_build_cells2(_P(verts), _P(Rg), _P(Th), _P(verts), n, 0.05, _P(hdr), _P(cell_start), _P(cell_pts), _P(scratch), _P(near_mask), None) == 0
    assert lib.sherf_build_near_lists(_P(hdr), _P(cell_pts), n, 0.05, _P(near_hdr), _P(near_list), near_list.numel(), None, None) == 0
    ray_o, ray_d, t_near, t_far = T(o), T(d), T(near), T(far)
    cap = R * S
    wlen = cell_ws_ints(R, S)
    cell_ws = Z(wlen + GUARD)
    cell_ws[wlen:] = SENT
    outs = []
    for flag in (0, SEARCH_BY_CANDIDATE):
        set_debug(flag)
        b = dict(counters=Z(4), ray_base=Z(R), ray_cnt=Z(R), cs_idx=Z(cap), cs_vid=Z(cap), cs_xs=Z(cap, 4, dtype=torch.float32),
                 dense_vid=Z(R * S), ray_mask=Z(R * nch, dtype=torch.int64), scan_ws=Z(R + R // 1024 + 2))
        try:
            rc = lib.sherf_sample_mask_nn_ws(_P(ray_o), _P(ray_d), _P(t_near), _P(t_far), R, S, _P(Rg), _P(Th), _P(hdr[0]), _P(cell_start[0]), _P(cell_pts[0]),
                                             _P(near_mask), cap, _P(b['counters']), _P(b['ray_base']), _P(b['ray_cnt']), _P(b['cs_idx']), _P(b['cs_vid']),
                                             _P(b['cs_xs']), _P(b['dense_vid']), _P(b['ray_mask']), _P(b['scan_ws']), _P(near_hdr), _P(near_list),
                                             _P(cell_ws), wlen, None)
            sync()
        finally:
            set_debug(0)
        assert rc == 0
        outs.append({k: v.cpu() for k, v in b.items()})
        # the per-sub-cell counts are left zero for the next frame, nothing is written behind the workspace
        assert not bool(cell_ws[:NSUB].any()) and bool((cell_ws[wlen:] == SENT).all()), (name, S, flag)
    new, old = outs
    nv = int(new['counters'][0])
    # the search by sub-cell really ran (it counts its work items; the search by candidate leaves the word alone)
    n_items = int(cell_ws[2 * NSUB + 1])
    # ---- bit-identical to the search by candidate ----
    assert nv == int(old['counters'][0]), (name, S, nv, int(old['counters'][0]))
    for k in ('ray_mask', 'ray_cnt', 'ray_base'):
        assert torch.equal(new[k], old[k]), (name, S, k)
    for k in ('cs_idx', 'cs_vid', 'cs_xs'):
        assert torch.equal(new[k][:nv].view(torch.int32), old[k][:nv].view(torch.int32)), (name, S, k)
    assert int(new['scan_ws'][-1]) == int(old['scan_ws'][-1])
    # ---- equal to brute force ----
    x = positions(o, d, near, far, S)
    d2 = d2_table(x, verts_np)
    best = d2.min(1)
    vid = d2.argmin(1)                                                    # (first minimum == lowest id)
    valid_mask = best < THR
    valid = np.flatnonzero(valid_mask)
    assert nv == valid.size, (name, S, nv, valid.size)
    assert np.array_equal(new['cs_idx'][:nv].numpy(), valid) and np.array_equal(new['cs_vid'][:nv].numpy(), vid[valid]), (name, S)
    assert np.array_equal(new['cs_xs'][:nv, :3].numpy(), x[valid]), (name, S)
    cnt = np.bincount(valid // S, minlength=R)
    assert np.array_equal(new['ray_cnt'].numpy(), cnt)
    assert np.array_equal(new['ray_base'].numpy(), np.concatenate([[0], np.cumsum(cnt)[:-1]]))
    bits = np.unpackbits(new['ray_mask'].numpy().view(np.uint8), bitorder='little').reshape(R, nch * 64)[:, :S].astype(bool)
    assert np.array_equal(bits.ravel(), valid_mask), (name, S)
    # ---- the geometry is the edge it is named for ----
    q, nsub = sub_cells(x, hdr[0].cpu())
    mbits = np.unpackbits(near_mask.cpu().numpy().view(np.uint8), bitorder='little').astype(bool)
    is_cand = (q >= 0) & mbits[np.maximum(q, 0)]
    ncand = int(new['scan_ws'][-1])
    assert ncand == int(is_cand.sum()), (name, S, ncand, int(is_cand.sum()))
    cand_per_q = np.bincount(q[is_cand], minlength=nsub)
    assert n_items == int(((cand_per_q + 63) // 64).sum()), (name, S, n_items)
    hq = near_hdr[:2 * NSUB].view(NSUB, 2).cpu().numpy()
    c['check'](dict(d2=d2, ref_vid=vid, valid_mask=valid_mask, nv=nv, ncand=ncand, q=q, nsub=nsub, is_cand=is_cand, cand_per_q=cand_per_q,
                    list_len_of_cand=hq[q[is_cand], 1]))
