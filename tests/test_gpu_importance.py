"""Importance sampling (depth_resolution_importance > 0; csrc/importance.hip, csrc/composite.hip: sherf_composite_merged, csrc/frame.hip:
sherf_render_frame_importance) on the MI355X.  The `check_*` bodies are shared with tests/test_hipcpu_importance.py, which runs them on the host build of the
unchanged kernel sources.  Pinned to the reference through tests/golden/importance_*.npz (tools/make_golden_importance.py)."""
import ctypes
import functools
import os

import numpy as np
import pytest
import torch

from oracle import sherf_oracle as O
from sherf_amd import _lib
from tests import gpu_common as G
from tests import test_gpu_field as F

gpu = pytest.mark.gpu
N_FINE = 16


@functools.lru_cache(None)
def golden(name):
    return dict(np.load(os.path.join(G.GOLDEN, name + '.npz')))


def dv(a, dtype=None):
    t = torch.as_tensor(np.ascontiguousarray(a)) if not torch.is_tensor(a) else a.contiguous()
    if dtype is not None:
        t = t.to(dtype)
    return G.dev_tensor(t) if not G.CPU_SHIM else (t.as_subclass(G._HostTensor) if t.is_floating_point() else t)


P = lambda t: None if t is None else _lib.ptr(t)


def stream():
    return _lib.stream()


def compact(dens):
    """Dense [R,S] densities (-80 = rejected) -> the frame's compact lists: ray_base, ray_cnt, cs_idx, sample_out rows (rgb filled in by the caller)."""
    mask = dens != -80.0
    cnt = mask.sum(1).astype(np.int32)
    base = (np.cumsum(cnt) - cnt).astype(np.int32)
    idx = np.nonzero(mask.reshape(-1))[0].astype(np.int32)
    return mask, base, cnt, idx


# ---- 1. the resampling kernel alone ----------------------------------------------------------------------------------------------------------------
def importance_fp64(dens, z, rd, u, mode):
    """sample_importance + sample_pdf (renderer.py:483-542) on MipRayMarcher2's weights, every formula in float64 from the fp32 inputs -> sorted [R,N]."""
    dens, z, u = dens.astype(np.float64), z.astype(np.float64), u.astype(np.float64)
    dn = np.sqrt((rd.astype(np.float64) ** 2).sum(1, keepdims=True))
    R, S = dens.shape
    delta = np.concatenate([z[:, 1:] - z[:, :-1], np.full((R, 1), 1e10)], 1) * dn
    x = dens - 1
    s = np.maximum(dens, 0) if mode == 'relu' else np.where(x > 20, x, np.log1p(np.exp(np.minimum(x, 20))))
    alpha = 1 - np.exp(-s * delta)
    T = np.cumprod(np.concatenate([np.ones((R, 1)), 1 - alpha + 1e-10], 1), 1)[:, :-1]
    w = alpha * T
    pad = np.concatenate([np.full((R, 1), -np.inf), w, np.full((R, 1), -np.inf)], 1)
    mx = np.maximum(pad[:, :-1], pad[:, 1:])                        # max_pool1d(2, 1, padding=1): S + 1
    av = 0.5 * (mx[:, :-1] + mx[:, 1:]) + 0.01                      # avg_pool1d(2, 1): S
    wi = av[:, 1:-1] + 1e-5
    cdf = np.concatenate([np.zeros((R, 1)), np.cumsum(wi / wi.sum(1, keepdims=True), 1)], 1)
    bins = 0.5 * (z[:, :-1] + z[:, 1:])
    M = S - 2
    out = np.empty_like(u)
    for r in range(R):
        inds = np.searchsorted(cdf[r], u[r], side='right')
        below, above = np.maximum(inds - 1, 0), np.minimum(inds, M)
        c0, c1 = cdf[r][below], cdf[r][above]
        den = c1 - c0
        den[den < 1e-5] = 1
        out[r] = bins[r][below] + (u[r] - c0) / den * (bins[r][above] - bins[r][below])
    return np.sort(out, 1)


def run_importance_kernel(dens, near, far, rd, u, mode, tok_cap=None):
    R, S = dens.shape
    N = u.shape[1]
    mask, base, cnt, idx = compact(dens)
    so = np.zeros((max(len(idx), 1), 4), np.float32)
    so[:len(idx), 3] = dens[mask]
    out = dv(np.full((R, N), np.nan, np.float32))
    keep = [dv(base), dv(cnt), dv(idx if len(idx) else np.zeros(1, np.int32)), dv(so), dv(rd), dv(near.reshape(-1)), dv(far.reshape(-1)), dv(u)]
    _lib.call('sherf_importance_depths', *[P(t) for t in keep[:4]], None, P(keep[4]), P(keep[5]), P(keep[6]), R, S,
              _lib.composite_bits(False, mode), tok_cap or max(len(idx), 1), P(keep[7]), N, P(out), None, stream())
    F._sync()
    return G.plain(out).numpy()


def check_resampling(ci):
    g = golden('importance_units')
    S, N = [int(v) for v in g['imp_cases'][ci]]
    dens, near, far, rd, u = (g[f'imp{ci}_{k}'] for k in ('dens', 'near', 'far', 'rd', 'u'))
    z = O.depths(torch.from_numpy(near.reshape(-1)), torch.from_numpy(far.reshape(-1)), S).numpy()
    assert dens.shape == (300, S) and u.shape == (300, N) and float(u.min()) == 0.0 and float(u.max()) <= 1.0
    span = (z[:, -1] - z[:, 0]).astype(np.float64)
    for mode in ('relu', 'softplus'):
        if f'imp{ci}_fine_{mode}' not in g:
            continue
        ours = run_importance_kernel(dens, near, far, rd, u, mode)
        ref64 = importance_fp64(dens, z, rd, u, mode)
        e_ours = np.abs(ours.astype(np.float64) - ref64).max(1)
        e_ref = np.abs(g[f'imp{ci}_fine_{mode}'].astype(np.float64) - ref64).max(1)
        print(f'resampling S={S} N={N} {mode}: max distance from the fp64 formulas / span: ours {float((e_ours / span).max()):.2e}, '
              f'the reference\'s fp32 {float((e_ref / span).max()):.2e}')
        assert not np.isnan(ours).any()
        assert bool((np.diff(ours, axis=1) >= 0).all())
        assert bool((ours >= z[:, :1]).all() and (ours <= z[:, -1:]).all())
        # the project's rule for what the fp32 reference itself only approximates (tests/test_gpu_backward.py): twice its own distance + 1e-6 of the span
        assert bool((e_ours <= 2 * e_ref + 1e-6 * span).all()), (S, N, mode, float((e_ours - 2 * e_ref - 1e-6 * span).max()))


# ---- 2. the merged compositing alone ---------------------------------------------------------------------------------------------------------------
def fine_lists(dens_f):
    """[R,N] fine densities -> the point sampler's rows of 64 over R * N points: mask words, row bases, the compact order."""
    flat = (dens_f != -80.0).reshape(-1)
    rows = (flat.size + 63) // 64
    bits = np.zeros(rows * 64, bool)
    bits[:flat.size] = flat
    words = (bits.reshape(rows, 64).astype(np.uint64) << np.arange(64, dtype=np.uint64)).sum(1, dtype=np.uint64).view(np.int64)
    cnt = bits.reshape(rows, 64).sum(1)
    return flat, words, (np.cumsum(cnt) - cnt).astype(np.int32)


def run_merged(near, far, rd, dens_c, col_c, fine, dens_f, col_f, mode, wb, tok_cap=None, fine_tok_cap=None):
    R, S = dens_c.shape
    N = fine.shape[1]
    z = O.depths(torch.from_numpy(near.reshape(-1)), torch.from_numpy(far.reshape(-1)), S).numpy()
    mask, base, cnt, idx = compact(dens_c)
    so = np.zeros((len(idx) + 1, 4), np.float32)
    so[:len(idx), :3], so[:len(idx), 3] = col_c[mask], dens_c[mask]
    fmask, words, fbase = fine_lists(dens_f)
    fo = np.zeros((int(fmask.sum()) + 1, 4), np.float32)
    fo[:-1, :3], fo[:-1, 3] = col_f.reshape(-1, 3)[fmask], dens_f.reshape(-1)[fmask]
    counters = np.array([len(idx), z.min().view(np.int32), z.max().view(np.int32), 0], np.int32)          # (positive depths: the ordered int is the bit pattern)
    GUARD = 7
    out = [dv(np.full(n + GUARD, 777.0, np.float32)) for n in (3 * R, R, R)]
    keep = [dv(counters), dv(base), dv(cnt), dv(np.append(idx, 0).astype(np.int32)), dv(so), dv(fine), dv(words), dv(fbase), dv(fo), dv(rd), dv(near.reshape(-1)), dv(far.reshape(-1))]
    c, b, n, i, s, f, w, fb, fo_, d, nr, fr = keep
    _lib.call('sherf_composite_merged', P(c), P(b), P(n), P(i), P(s), tok_cap or len(idx) + 1, P(f), P(w), P(fb), P(fo_), fine_tok_cap or fo.shape[0],
              P(d), P(nr), P(fr), R, S, N, _lib.composite_bits(wb, mode), P(out[0]), P(out[1]), P(out[2]), stream())
    F._sync()
    o = [G.plain(t) for t in out]
    for t, n_ in zip(o, (3 * R, R, R)):
        assert bool((t[n_:] == 777.0).all()), 'a guard word behind an output was written'
    return dict(rgb=o[0][:3 * R].view(R, 3), depth=o[1][:R], acc=o[2][:R], flags=int(G.plain(c)[3]), z=z, base=base, cnt=cnt, fmask=fmask.reshape(R, N), fbase=fbase, words=words)


def dense_merge(z, fine, dens_c, col_c, dens_f, col_f, rd, mode, wb):
    """The same samples merged in the stated order (stable sort of [coarse, fine]) and scattered densely, through sherf_composite_dense."""
    t = np.concatenate([z, fine], 1)
    order = np.argsort(t, 1, kind='stable')
    take = lambda a: np.take_along_axis(a, order if a.ndim == 2 else order[:, :, None], 1)
    t, s, c = take(t), take(np.concatenate([dens_c, dens_f], 1)), take(np.concatenate([col_c, col_f], 1))
    R, K = t.shape
    rgb, dep, w = dv(np.zeros((R, 3), np.float32)), dv(np.zeros(R, np.float32)), dv(np.zeros((R, K), np.float32))
    keep = [dv(c), dv(s), dv(t), dv(rd), dv(np.array([t.min(), t.max()], np.float32))]
    _lib.call('sherf_composite_dense', *[P(k) for k in keep[:4]], R, K, _lib.composite_bits(wb, mode), P(keep[4]), P(rgb), P(dep), P(w), stream())
    F._sync()
    return G.plain(rgb), G.plain(dep), seq_sum(G.plain(w)), G.plain(w)


def seq_sum(w):
    """The kernels' running `wsum += w` over the dense weights in fp32, sample by sample: a rejected sample's weight is exactly 0, so this IS the compact /
    merged kernels' acc, bit for bit (torch's .sum pairs the terms in another order)."""
    acc = torch.zeros(w.shape[0], dtype=torch.float32)
    for k in range(w.shape[1]):
        acc = acc + w[:, k]
    return acc


def check_merged(ci):
    g = golden('importance_units_merged')
    R, S, N = [int(v) for v in g[f'mrg{ci}_shape']]
    near, far, rd, fine, dens_c, dens_f, col_c, col_f = (g[f'mrg{ci}_{k}'] for k in ('near', 'far', 'rd', 'fine', 'dens_c', 'dens_f', 'col_c', 'col_f'))
    assert ci != 1 or S + N == 512
    # (a fine sample BEFORE the first coarse one cannot occur: the bins are mid-points of the coarse depths, so every fine depth exceeds the ray's first)
    for mode in ('relu', 'softplus'):
        for wb in (False, True):
            o = run_merged(near, far, rd, dens_c, col_c, fine, dens_f, col_f, mode, wb)
            assert o['flags'] == 0
            d_rgb, d_dep, d_acc, _ = dense_merge(o['z'], fine, dens_c, col_c, dens_f, col_f, rd, mode, wb)
            assert F.same(o['rgb'], d_rgb) and F.same(o['depth'], d_dep) and F.same(o['acc'], d_acc), (ci, mode, wb)
            e = [float((o['rgb'] - torch.from_numpy(g[f'mrg{ci}_rgb_{mode}_{int(wb)}'])).abs().max()), float((o['acc'] - torch.from_numpy(g[f'mrg{ci}_acc_{mode}_{int(wb)}'])).abs().max()),
                 float((o['depth'] - torch.from_numpy(g[f'mrg{ci}_depth_{mode}_{int(wb)}'])).abs().max())]
            print(f'merged compositing case {ci} {mode} wb={int(wb)}: max abs error vs the reference rgb {e[0]:.2e} acc {e[1]:.2e} depth {e[2]:.2e}')
            # tests/test_hipcpu_composite_edges.py: check_dense_forward's absolute bounds against a reference golden
            assert e[0] < 2e-6 and e[1] < 1e-6 and e[2] < 1e-5, (ci, mode, wb, e)
    if ci != 0:
        return
    # ties (not in the golden: torch.sort promises no order): a coarse-fine tie and a fine-fine tie, against the dense kernel in the stated order
    z = O.depths(torch.from_numpy(near.reshape(-1)), torch.from_numpy(far.reshape(-1)), S).numpy()
    ft = fine.copy()
    dc, df = dens_c.copy(), dens_f.copy()
    for r in range(5, 60):
        ft[r] = np.sort(ft[r])
        ft[r, 1] = z[r, 2]; ft[r, 2] = z[r, 2]                       # fine == fine == coarse sample 2
        ft[r] = np.sort(ft[r])
        dc[r, 2] = 1.5; df[r] = np.where(df[r] == -80.0, 0.75, df[r])
    cf = np.where((df == -80.0)[:, :, None], 0, np.maximum(col_f, 0.25)).astype(np.float32)
    cc = np.where((dc == -80.0)[:, :, None], 0, np.maximum(col_c, 0.125)).astype(np.float32)
    for mode in ('relu', 'softplus'):
        o = run_merged(near, far, rd, dc, cc, ft, df, cf, mode, False)
        d_rgb, d_dep, d_acc, _ = dense_merge(o['z'], ft, dc, cc, df, cf, rd, mode, False)
        assert F.same(o['rgb'], d_rgb) and F.same(o['depth'], d_dep) and F.same(o['acc'], d_acc), ('ties', mode)
    # token capacities ten rows short, each list in turn: NaN on exactly the rays that reach beyond, flag bit 1
    full = run_merged(near, far, rd, dens_c, col_c, fine, dens_f, col_f, 'relu', False)
    nvc, nvf = int(full['cnt'].sum()), int(full['fmask'].sum())
    o = run_merged(near, far, rd, dens_c, col_c, fine, dens_f, col_f, 'relu', False, tok_cap=nvc - 10)
    beyond = torch.from_numpy((full['base'] + full['cnt']) > nvc - 10)
    assert o['flags'] == 2 and int(beyond.sum()) > 0 and torch.equal(torch.isnan(o['acc']), beyond) and F.same(o['rgb'][~beyond], full['rgb'][~beyond])
    o = run_merged(near, far, rd, dens_c, col_c, fine, dens_f, col_f, 'relu', False, fine_tok_cap=nvf - 10)
    rank = np.cumsum(full['fmask'].reshape(-1)).reshape(R, N)         # compact position + 1 of each valid fine sample
    beyond = torch.from_numpy(((rank > nvf - 10) & full['fmask']).any(1))
    assert o['flags'] == 2 and int(beyond.sum()) > 0 and torch.equal(torch.isnan(o['acc']), beyond) and F.same(o['depth'][~beyond], full['depth'][~beyond])


# ---- 3 / 4. the fine pass and the frame on `tiny_ri` -----------------------------------------------------------------------------------------------
def frame(precision='f16x3', decoder='nerf', branches=(True, True, True), options=None, n=N_FINE, u='golden'):
    rend, dec = F._modules(precision, decoder, branches)
    rend.train(True)
    x = F._inputs()
    d = x['d']
    opts = dict(G.fixture(F.CFG)['options'], mlp_precision=precision, depth_resolution_importance=n)
    if isinstance(u, str):
        opts['importance_u'] = dv(golden('importance_tiny_ri')['u'])
    elif u is not None:
        opts['importance_u'] = u
    opts.update(options or {})
    with torch.no_grad():
        rgb, depth, acc = rend(x['planes'], x['obs_img'], x['obs_feat'], x['sp'], None, x['sp_input'], dec, d['ray_o_all'][:, 0],
                               d['ray_d_all'][:, 0], d['near_all'][:, 0], d['far_all'][:, 0], d, opts)
    F._sync()
    last = rend.last
    imp = last.get('importance')
    return dict(rgb=G.plain(rgb[0]).clone(), depth=G.plain(depth[0, :, 0]).clone(), acc=G.plain(acc[0, :, 0]).clone(), last=last, rend=rend, dec=dec,
                depths_fine=None if imp is None else G.plain(imp['depths_fine']).clone(), imp=imp)


def same_frame(a, b):
    return F.same(a['rgb'], b['rgb']) and F.same(a['depth'], b['depth']) and F.same(a['acc'], b['acc'])


def fine_points(t):
    fx = G.fixture(F.CFG)['input_data']
    o, rd = torch.from_numpy(fx['ray_o_all'][0, 0]), torch.from_numpy(fx['ray_d_all'][0, 0])
    pts = o.unsqueeze(-2) + t.unsqueeze(-1) * rd.unsqueeze(-2)                       # renderer.py:381 in torch fp32
    return pts.reshape(-1, 3).contiguous(), rd.unsqueeze(-2).expand_as(pts).reshape(-1, 3).contiguous(), rd


def golden_fine_mask():
    g = golden('importance_tiny_ri')
    return torch.from_numpy(np.unpackbits(g['fine_mask_bits'])[:1024 * N_FINE].astype(bool))


def check_fine_pass_pinned():
    """The field query IS the fine pass's chain (the frame check below shows the frame's fine buffers hold its bits): on the golden's depths_fine."""
    g = golden('importance_tiny_ri')
    mask = golden_fine_mask()
    # the frame's OWN fine pass (sherf_render_frame_importance with the depths handed in: importance->u NULL) ...
    f = frame(u=None, options=dict(importance_depths=dv(g['depths_fine'])))
    fws, nf = f['imp']['ws'], f['imp']['n_fine']
    assert F.same(f['depths_fine'], torch.from_numpy(g['depths_fine'])) and nf == 1814
    words = G.plain(fws['ray_mask']).numpy().view(np.uint64)
    ours = torch.from_numpy(((words[:, None] >> np.arange(64, dtype=np.uint64)) & np.uint64(1)).astype(bool).reshape(-1)[:1024 * N_FINE])
    assert torch.equal(ours, mask)
    fo = G.plain(fws['sample_out'][:nf]).clone()
    sig_ref = torch.relu(torch.from_numpy(g['fine_sample_sigma']))
    e_sig = float((torch.relu(fo[:, 3]) - sig_ref).abs().max() / sig_ref.max())
    e_rgb = float((fo[:, :3] - torch.from_numpy(g['fine_sample_rgb'])).abs().max())
    print(f'the frame\'s fine pass on the golden depths: sigma+ rel-to-max err {e_sig:.2e}, rgb max abs err {e_rgb:.2e}')
    assert e_sig < F.PER_SAMPLE_TOL['f16x3'][0] and e_rgb < F.PER_SAMPLE_TOL['f16x3'][1]
    # ... and query_points on o + t d formed in torch fp32: the same bits
    pts, dirs, _ = fine_points(torch.from_numpy(g['depths_fine']))
    q = F.query(pts, dirs, 'f16x3')
    assert int(mask.sum()) == int(g['fine_n_valid']) == 1814 and torch.equal(q['mask'], mask)
    assert F.same(q['sigma'][mask], fo[:, 3].contiguous()) and F.same(q['rgb'][mask], fo[:, :3].contiguous())
    sig_ref = torch.relu(torch.from_numpy(g['fine_sample_sigma']))
    e_sig = float((torch.relu(q['sigma'][mask]) - sig_ref).abs().max() / sig_ref.max())
    e_rgb = float((q['rgb'][mask] - torch.from_numpy(g['fine_sample_rgb'])).abs().max())
    print(f'query_points on the golden depths: sigma+ rel-to-max err {e_sig:.2e}, rgb max abs err {e_rgb:.2e}')
    assert e_sig < F.PER_SAMPLE_TOL['f16x3'][0] and e_rgb < F.PER_SAMPLE_TOL['f16x3'][1]


def check_frame_staged(precision='f16x3', decoder='nerf', branches=(True, True, True), mode='relu'):
    """(a) the frame == coarse forward, kernel 1 on its `last`, query_points on the fine points, the dense merge through sherf_amd's MipRayMarcher2."""
    from sherf_amd.ray_marcher import MipRayMarcher2
    f = frame(precision, decoder, branches, options=dict(clamp_mode=mode))
    imp = f['imp']
    R, S, N = 1024, 16, N_FINE
    fws = imp['ws']
    nf = imp['n_fine']
    fine_out = G.plain(fws['sample_out'][:nf]).clone()
    fine_idx = G.plain(fws['cs_idx'][:nf]).long().clone()
    c = frame(precision, decoder, branches, n=0, u=None, options=dict(clamp_mode=mode))
    ws = c['last']['ws']
    nv = int(ws['counters'][0])
    assert nv == imp['n_coarse'] == 628
    x = F._inputs()['d']
    t = dv(np.full((R, N), np.nan, np.float32))
    u = dv(golden('importance_tiny_ri')['u'])
    _lib.call('sherf_importance_depths', P(ws['ray_base']), P(ws['ray_cnt']), P(ws['cs_idx']), P(ws['sample_out']), None, P(x['ray_d_all'][:, 0].contiguous()),
              P(x['near_all'][:, 0].contiguous()), P(x['far_all'][:, 0].contiguous()), R, S, _lib.composite_bits(False, mode), c['last']['cap'], P(u), N, P(t), None, stream())
    F._sync()
    t = G.plain(t)
    assert F.same(t, f['depths_fine'])
    pts, dirs, rd = fine_points(t)
    q = F.query(pts, dirs, precision, decoder, branches)
    assert int(q['mask'].sum()) == nf and torch.equal(torch.nonzero(q['mask'])[:, 0], fine_idx)
    assert F.same(q['sigma'][q['mask']], fine_out[:, 3].contiguous()) and F.same(q['rgb'][q['mask']], fine_out[:, :3].contiguous())
    # the coarse samples scattered densely, merged with the fine ones in the stated order
    cmask = F._golden_mask()
    cs = torch.full((R * S,), -80.0); cc = torch.zeros(R * S, 3)
    co = G.plain(ws['sample_out'][:nv])
    cs[cmask], cc[cmask] = co[:, 3], co[:, :3]
    _, _, z, _ = F._ray_samples()
    at = torch.cat([z, t], 1)
    order = torch.sort(at, dim=1, stable=True)[1]
    at = torch.gather(at, 1, order)
    a_s = torch.gather(torch.cat([cs.view(R, S), q['sigma'].view(R, N)], 1), 1, order)
    a_c = torch.gather(torch.cat([cc.view(R, S, 3), q['rgb'].view(R, N, 3)], 1), 1, order[:, :, None].expand(-1, -1, 3))
    rgb, depth, w = MipRayMarcher2()(dv(a_c.view(1, R, S + N, 3)), dv(a_s.view(1, R, S + N, 1)), dv(at.view(1, R, S + N, 1)), dv(rd.reshape(1, R, 3)),
                                     dict(clamp_mode=mode, white_back=False))
    F._sync()
    assert F.same(f['rgb'], G.plain(rgb[0])) and F.same(f['depth'], G.plain(depth[0, :, 0]))
    assert F.same(f['acc'], seq_sum(G.plain(w[0, :, :, 0])))
    return f


def check_frame_against_golden():
    """(b) rays whose 16 fine mask bits all equal the golden's meet tests/test_gpu_parity.py's bounds on hip_render; at most 3 of the 172 rays with a valid fine
    sample may be left out.  (c) a second call gives the same bits."""
    g = golden('importance_tiny_ri')
    f = frame()
    fws = f['imp']['ws']
    words = G.plain(fws['ray_mask']).numpy().view(np.uint64)
    ours = torch.from_numpy(((words[:, None] >> np.arange(64, dtype=np.uint64)) & np.uint64(1)).astype(bool).reshape(-1)[:1024 * N_FINE]).view(1024, N_FINE)
    gm = golden_fine_mask().view(1024, N_FINE)
    differ = (ours != gm).any(1)
    has = gm.any(1)
    print(f'frame vs the golden: {int(differ.sum())} rays with a differing fine mask bit are left out ({int((differ & has).sum())} of the {int(has.sum())} rays with a valid '
          f'fine sample); fine count {f["imp"]["n_fine"]} (golden {int(g["fine_n_valid"])})')
    assert int(has.sum()) == 172 and int((differ & has).sum()) <= 3 and int(differ.sum()) <= 3
    k = ~differ
    assert G.rel(f['rgb'][k], torch.from_numpy(g['rgb'])[k]) < 1e-3 and G.rel(f['acc'][k], torch.from_numpy(g['acc'][:, 0])[k]) < 1e-3
    assert torch.allclose(f['depth'][k], torch.from_numpy(g['depth'][:, 0])[k], rtol=1e-3, atol=1e-4)
    coarse = golden('renderer_tiny_ri')
    assert int(((f['rgb'] - torch.from_numpy(coarse['rgb'])).abs().max(1)[0] > 1e-3).sum()) > 100          # (not the coarse-only image)
    assert same_frame(frame(), f)


def check_seeds_neighbours_and_resize():
    """(d) the default draw follows torch's global generator; (e) coarse-only frames around an importance frame are undisturbed; (f) a token capacity below
    the fine count costs one re-size and changes no bit."""
    rend = F._modules()[0]
    c0 = frame(n=0, u=None, options=dict(reuse_observation=True))
    cap0 = c0['last']['cap']
    torch.manual_seed(5); a = frame(u=None)
    torch.manual_seed(5); b = frame(u=None)
    torch.manual_seed(6); c = frame(u=None)
    assert same_frame(a, b) and F.same(a['depths_fine'], b['depths_fine']) and not F.same(a['depths_fine'], c['depths_fine']) and not F.same(a['rgb'], c['rgb'])
    c1 = frame(n=0, u=None, options=dict(reuse_observation=True))
    assert same_frame(c0, c1) and c1['last']['cap'] == cap0 and 'importance' not in c1['last']
    c2 = frame(n=0, u=None, options=dict(reuse_observation=True))
    assert same_frame(c0, c2) and c2['last']['observation_reused']
    ref = frame()
    nf = ref['imp']['n_fine']
    before = (rend.__dict__.get('_flags') or {}).get('fine_token_rerenders', 0)
    small = frame(options=dict(token_capacity=1))                    # (rounded up to the granule: below the fine count only if the granule is)
    tiny_cap = small['imp']['cap']
    if tiny_cap >= nf:                                              # the granule exceeds this fixture's count: shrink it for the check
        g0 = type(rend).TOKEN_GRANULE
        try:
            type(rend).TOKEN_GRANULE = 256
            before = (rend.__dict__.get('_flags') or {}).get('fine_token_rerenders', 0)
            small = frame(options=dict(token_capacity=256))
        finally:
            type(rend).TOKEN_GRANULE = g0
    assert (rend.__dict__.get('_flags') or {}).get('fine_token_rerenders', 0) == before + 1
    assert bool(torch.isfinite(small['rgb']).all()) and same_frame(small, ref) and small['imp']['cap'] >= nf


# ---- 5. what raises ---------------------------------------------------------------------------------------------------------------------------------
def check_raises():
    rend = F._modules()[0]
    with pytest.raises(NotImplementedError, match='density_noise'):
        frame(options=dict(density_noise=0.5))
    with pytest.raises(NotImplementedError, match='depth_range'):
        frame(options=dict(depth_range=(1.0, 2.0)))
    with pytest.raises(ValueError, match='depth_resolution'):
        frame(options=dict(depth_resolution=2))
    with pytest.raises(ValueError, match='depth_resolution_importance'):
        frame(n=257, u=None)
    with pytest.raises(ValueError, match='importance_u'):
        frame(u=dv(np.zeros((1024, N_FINE + 1), np.float32)))
    bad = golden('importance_tiny_ri')['u'].copy()
    bad[3, 3] = 1.5
    with pytest.raises(ValueError, match=r'\[0, 1\]'):
        frame(u=dv(bad))
    rend.enable_autograd = True
    try:
        with torch.enable_grad(), pytest.raises(NotImplementedError, match='grad-recorded'):
            x = F._inputs(); d = x['d']
            rend(x['planes'], x['obs_img'], x['obs_feat'], x['sp'], None, x['sp_input'], F._modules()[1], d['ray_o_all'][:, 0], d['ray_d_all'][:, 0],
                 d['near_all'][:, 0], d['far_all'][:, 0], d, dict(G.fixture(F.CFG)['options'], depth_resolution_importance=N_FINE))
    finally:
        rend.enable_autograd = False
    # the ABI
    l = _lib.lib()
    one = ctypes.c_void_p(64)
    lv = (_lib.VoxLevel * 3)()
    assert l.sherf_importance_depths(None, one, one, one, None, one, one, one, 4, 16, 0, 8, one, 4, one, None, None) == -1
    assert l.sherf_importance_depths(one, one, one, one, None, one, one, one, 4, 2, 0, 8, one, 4, one, None, None) == -1           # S = 2
    assert l.sherf_importance_depths(one, one, one, one, None, one, one, one, 4, 16, 0, 8, one, 257, one, None, None) == -1        # N = 257
    assert l.sherf_importance_depths(one, one, one, one, None, one, one, one, 4, 16, 0, 8, one, 0, one, None, None) == -1          # n <= 0
    assert l.sherf_composite_merged(None, one, one, one, one, 8, one, one, one, one, 8, one, one, one, 4, 16, 4, 0, one, one, one, None) == -1
    assert l.sherf_composite_merged(one, one, one, one, one, 8, one, one, one, one, 8, one, one, one, 4, 16, 0, 0, one, one, one, None) == -1
    fr, im = _lib.Frame(), _lib.Importance()
    assert l.sherf_render_frame_importance(ctypes.byref(fr), None, lv, None, ctypes.c_void_p(8), None) == -1
    assert l.sherf_render_frame_importance(None, ctypes.byref(im), lv, None, ctypes.c_void_p(8), None) == -1
    for k, _ in _lib.Importance._fields_:
        if k not in ('n', 'pad_', 'capacity', 'tok_capacity'):
            setattr(im, k, 64)
    for k, t in _lib.Frame._fields_:
        if t is ctypes.c_void_p:
            setattr(fr, k, 64)
    fr.R, fr.S, fr.capacity, im.n, im.capacity = 8, 16, 128, 4, 31                                   # capacity < R * n
    assert l.sherf_render_frame_importance(ctypes.byref(fr), ctypes.byref(im), lv, None, ctypes.c_void_p(8), None) == -1
    assert b'bad argument' in l.sherf_last_error() and b'imp->capacity >= np' in l.sherf_last_error()      # (the check that tripped, by its text)
    im.n, im.capacity = 0, 64
    assert l.sherf_render_frame_importance(ctypes.byref(fr), ctypes.byref(im), lv, None, ctypes.c_void_p(8), None) == -1
    assert b'imp->n >= 1' in l.sherf_last_error()
    im.n, fr.S = 4, 2
    assert l.sherf_render_frame_importance(ctypes.byref(fr), ctypes.byref(im), lv, None, ctypes.c_void_p(8), None) == -1
    assert b'f->S >= 3' in l.sherf_last_error()
    assert l.sherf_importance_depths(one, one, one, one, None, one, one, one, 4, 2, 0, 8, one, 4, one, None, None) == -1 and b'S >= 3' in l.sherf_last_error()
    assert l.sherf_importance_depths(one, one, one, one, None, one, one, one, 4, 16, 0, 8, one, 257, one, None, None) == -1 and b'N <= kMaxN' in l.sherf_last_error()
    assert l.sherf_importance_points(None, one, one, 4, 4, one, None) == -1


# ---- 6. the generator passes rendering_kwargs through --------------------------------------------------------------------------------------------------
def check_generator():
    gen, d = F._generator()
    kw = dict(gen.rendering_kwargs)
    S = int(kw['depth_resolution'])
    z, c0 = G.dev_tensor(torch.linspace(0, 1, 8).reshape(1, 8)), G.dev_tensor(torch.zeros(1, 25))
    try:
        gen.rendering_kwargs = dict(kw, depth_resolution_importance=N_FINE)
        with torch.no_grad():
            torch.manual_seed(3)
            ws = gen.mapping(z, c0, input_img=d['obs_img_all'][:, 0])
            out = gen.synthesis(ws, d, c0, use_sr_module=False)
            F._sync()
            img = G.plain(out['image']).clone()
            imp = gen.renderer.last.get('importance')
            assert imp is not None and imp['N'] == N_FINE and gen.renderer.last['S'] == S
            ours = G.plain(gen.renderer.last['out']).clone()
            gen.rendering_kwargs = kw
            coarse = G.plain(gen.synthesis(ws, d, c0, use_sr_module=False)['image']).clone()
            F._sync()
    finally:
        gen.rendering_kwargs = kw
    R = ours.numel() // 5
    assert img.numel() == 3 * R and F.same(img.reshape(3, -1).t().contiguous().reshape(-1), ours[:3 * R].contiguous())    # the renderer's image, as synthesis lays it out
    assert not F.same(img, coarse)


# ---- the tests --------------------------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize('ci', range(6))
def test_resampling_kernel_against_the_reference(ci):
    check_resampling(ci)


@gpu
@pytest.mark.parametrize('ci', range(2))
def test_merged_compositing_alone(ci):
    check_merged(ci)


@gpu
def test_fine_pass_pinned_to_the_reference():
    check_fine_pass_pinned()


@gpu
@pytest.mark.parametrize('case', ['nerf-f16x3', 'nerf-bf16', 'osg', 'f101', 'nerf-f16x3/softplus'])
def test_frame_is_the_staged_composition(case):
    _, decoder, branches, prec = F.CASES[case.split('/')[0]]
    check_frame_staged(prec, decoder, branches, 'softplus' if case.endswith('softplus') else 'relu')


@gpu
def test_frame_against_the_golden_image():
    check_frame_against_golden()


@gpu
def test_seeds_neighbours_and_token_resize():
    check_seeds_neighbours_and_resize()


@gpu
def test_what_raises():
    check_raises()


@gpu
def test_generator_passes_the_option_through():
    check_generator()
