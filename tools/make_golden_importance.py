"""TEST INFRASTRUCTURE (CPU only, build container).  Goldens of the reference's importance sampling (renderer.py:373-398 with its two broken
calls repaired as include/sherf_hip.h states it: the coarse marcher call gets the ray directions, the fine samples go through the coarse pass's chain):

    python tools/make_golden_importance.py [frame] [units]        (default: both)

  tests/golden/importance_tiny_ri.npz   the two-pass frame on `tiny_ri` with N = 16 fine samples and u = torch.rand under seed 1:
        1. make_golden.run('tiny_ri')                         the coarse per-sample sigma / rgb and mask (== renderer_tiny_ri.npz)
        2. the reference's ray_marcher(colors, densities, depths, ray_directions, opts)  -> weights
        3. the reference's sample_importance, torch.rand replaced at run time by the recorded u
        4. make_golden.run again with ImportanceRenderer.sample_stratified replaced at run time by a function returning depths_fine and
           the fixture's depth_resolution set to N: its per-sample values and mask are the fine pass
        5. the reference's unify_samples and ray_marcher(all_colors, all_densities, all_depths, ray_directions, opts)
     Stored: u, depths_fine, the fine mask bits, the fine per-sample rgb / sigma, the merged weights, the final rgb / depth / acc, the smallest
     |d^2 - 0.05^2| over the fine samples.  depths_fine (and everything per fine sample) is stored with each ray's values in ASCENDING order: the
     reference leaves them in the order of u and sorts in unify_samples; per-sample values do not depend on the order they are evaluated in.
     Asserted before writing: no two depths of a ray are equal (torch.sort promises no order for ties), no fine |d^2 - 0.05^2| < 1e-6 (the oracle's
     own margin), the image differs from the coarse-only one on more than 100 rays.

  tests/golden/importance_units.npz          synthetic tables through the reference's sample_importance (`imp<i>_*`)
  tests/golden/importance_units_merged.npz   ... and through unify_samples + MipRayMarcher2 (`mrg<i>_*`), in the manner of units.npz /
                                             marcher_softplus.npz (two files: each stays under the 1 MiB a committed file may have)

oracle/make_golden.py is used as a library; nothing at test time imports this module; the files hold recorded data only.
"""
import os
import sys
import tempfile
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import fixtures, make_golden as MG          # noqa: E402

GOLDEN = os.path.join(ROOT, 'tests', 'golden')
CFG, N_FINE, SEED = 'tiny_ri', 16, 1
# (S, N) of the resampling cases: every S and N the tests ask for, the launch shape's edges (a lane holds 1..4 weights / draws) on both axes
IMP_CASES = ((3, 1), (4, 2), (16, 63), (64, 64), (65, 65), (256, 256))
IMP_RAYS = 300


def reference_importance(R, depths, weights, u):
    """The reference's sample_importance on depths [1,R,S,1] / weights [1,R,S,1] with torch.rand -> u [R,N]."""
    me = types.SimpleNamespace(sample_pdf=lambda *a, **k: R.ImportanceRenderer.sample_pdf(None, *a, **k))
    rand = torch.rand
    torch.rand = lambda *a, **k: u.clone()
    try:
        return R.ImportanceRenderer.sample_importance(me, depths, weights, u.shape[1])
    finally:
        torch.rand = rand


def dense(mask, rgb_c, sig_c, Rr, S):
    """renderer.py:364-371: the compact per-sample values scattered back, rgb 0 / sigma -80 outside the shell."""
    colors = torch.zeros(Rr * S, 3)
    dens = torch.full((Rr * S, 1), -80.0)
    colors[mask] = rgb_c
    dens[mask] = sig_c.reshape(-1, 1)
    return colors.view(1, Rr, S, 3), dens.view(1, Rr, S, 1)


def run_frame(R, T):
    from training.volumetric_rendering.ray_marcher import MipRayMarcher2
    fx = fixtures.renderer_inputs(CFG)
    opts = fx['options']
    d = fixtures.to_torch(fx['input_data'])
    ray_o, ray_d, near, far = d['ray_o_all'][:, 0], d['ray_d_all'][:, 0], d['near_all'][:, 0], d['far_all'][:, 0]
    Rr, S = ray_o.shape[1], int(opts['depth_resolution'])
    marcher = MipRayMarcher2()
    with tempfile.TemporaryDirectory() as tmp:
        MG.run(CFG, R, T, tmp)
        g = dict(np.load(os.path.join(tmp, f'renderer_{CFG}.npz')))
    mask_c = torch.from_numpy(np.unpackbits(g['mask_bits'])[:Rr * S].astype(bool))
    colors_c, dens_c = dense(mask_c, torch.from_numpy(g['sample_rgb']), torch.from_numpy(g['sample_sigma']), Rr, S)
    depths_c = R.ImportanceRenderer.sample_stratified(None, ray_o, near, far, S, False)
    with torch.no_grad():
        rgb0, _, w_c = marcher(colors_c, dens_c, depths_c, ray_d, opts)
        torch.manual_seed(SEED)
        u = torch.rand(Rr, N_FINE)
        fine = reference_importance(R, depths_c, w_c, u)                   # [1,R,N,1], in the order of u
    fine = torch.sort(fine, dim=-2)[0].contiguous()
    # the fine pass: the unmodified forward on the fine depths (knn distances of ALL samples recorded for the margin)
    d2_all = []
    orig_knn, orig_strat, orig_inputs = R.knn_points, R.ImportanceRenderer.sample_stratified, fixtures.renderer_inputs

    def knn_rec(a, b, K=1):
        out = orig_knn(a, b, K=K)
        d2_all.append(out[0].clone())
        return out

    def inputs_n(cfg_name, smpl=None):
        f = dict(orig_inputs(cfg_name, smpl))
        f['options'] = dict(f['options'], depth_resolution=N_FINE)
        return f
    R.knn_points, R.ImportanceRenderer.sample_stratified, fixtures.renderer_inputs = knn_rec, (lambda self, *a, **k: fine.clone()), inputs_n
    try:
        with tempfile.TemporaryDirectory() as tmp:
            MG.run(CFG, R, T, tmp)
            gf = dict(np.load(os.path.join(tmp, f'renderer_{CFG}.npz')))
    finally:
        R.knn_points, R.ImportanceRenderer.sample_stratified, fixtures.renderer_inputs = orig_knn, orig_strat, orig_inputs
    mask_f = torch.from_numpy(np.unpackbits(gf['mask_bits'])[:Rr * N_FINE].astype(bool))
    colors_f, dens_f = dense(mask_f, torch.from_numpy(gf['sample_rgb']), torch.from_numpy(gf['sample_sigma']), Rr, N_FINE)
    with torch.no_grad():
        all_t, all_c, all_s = R.ImportanceRenderer.unify_samples(None, depths_c, colors_c, dens_c, fine, colors_f, dens_f)
        rgb, depth, w = marcher(all_c, all_s, all_t, ray_d, opts)
    d2 = next(x for x in d2_all if x.numel() == Rr * N_FINE)           # (the sample query; the glue's canonicalisation searches too)
    margin = float((d2.view(-1) - 0.05 ** 2).abs().min())
    ties = int((all_t[0, :, 1:, 0] == all_t[0, :, :-1, 0]).sum())
    changed = int(((rgb[0] - rgb0[0]).abs().max(-1)[0] > 0).sum())
    rays_f = int(mask_f.view(Rr, N_FINE).any(1).sum())
    print(f'importance {CFG}: N={N_FINE} seed={SEED}: {int(mask_f.sum())} of {mask_f.numel()} fine samples valid on {rays_f} rays; equal depths {ties}; '
          f'min |d2 - 0.05^2| over the fine samples {margin:.3e}; image differs from the coarse-only one on {changed} rays by up to '
          f'{float((rgb - rgb0).abs().max()):.3f}')
    assert ties == 0, 'a ray holds two equal depths: choose another seed'
    assert margin >= 1e-6, 'a fine sample lies within the oracle\'s margin of the shell threshold: choose another seed'
    assert changed > 100
    path = os.path.join(GOLDEN, f'importance_{CFG}.npz')
    np.savez_compressed(path, u=u.numpy(), depths_fine=fine[0, :, :, 0].numpy(), fine_mask_bits=np.packbits(mask_f.numpy().astype(np.uint8)),
                        fine_n_valid=np.int64(mask_f.sum()), fine_sample_rgb=gf['sample_rgb'], fine_sample_sigma=gf['sample_sigma'],
                        weights=w[0, :, :, 0].numpy(), rgb=rgb[0].numpy(), depth=depth[0].numpy(), acc=w.sum(2)[0].numpy(),
                        fine_min_margin=np.float64(margin), n=np.int64(N_FINE), seed=np.int64(SEED))
    print('frame ->', path, f'({os.path.getsize(path) / 1e3:.0f} KB)')


def importance_inputs(rs, Rr, S, N):
    """Per-ray densities whose coarse weights are: ray 0 all zero (every sample rejected: the uniform pdf), rays 1-3 all mass on sample 0 / S-1 / one inner
    sample (an opaque sample alone), ray 4 a ramp, ray 5 every sample valid but transparent (sigma < 0), the rest random with ~60 % rejected.  Densities are
    multiples of 1/4 (the file stays small).  u: see `importance_u`."""
    dens = np.round(rs.normal(0, 6, (Rr, S)) * 4) / 4
    dens[rs.uniform(0, 1, (Rr, S)) < 0.6] = -80.0
    dens[:6] = -80.0
    dens[1, 0] = 1e4
    dens[2, S - 1] = 1e4
    dens[3, S // 2] = 1e4
    dens[4] = np.linspace(0.25, 0.25 * S, S)
    dens[5] = -1.0
    near = rs.uniform(1, 2, (Rr, 1)).astype(np.float32)
    far = near + rs.uniform(0.5, 2, (Rr, 1)).astype(np.float32)
    rd = rs.normal(0, 1, (Rr, 3)).astype(np.float32)
    return dens.astype(np.float32), near, far, rd


def run_units(R):
    from training.volumetric_rendering.ray_marcher import MipRayMarcher2
    rs = np.random.RandomState(41)
    marcher = MipRayMarcher2()
    out = {'imp_cases': np.asarray(IMP_CASES, dtype=np.int64)}
    for ci, (S, N) in enumerate(IMP_CASES):
        dens, near, far, rd = importance_inputs(rs, IMP_RAYS, S, N)
        depths = R.ImportanceRenderer.sample_stratified(None, torch.zeros(1, IMP_RAYS, 3), torch.from_numpy(near)[None], torch.from_numpy(far)[None], S, False)
        colors = torch.zeros(1, IMP_RAYS, S, 3)
        for mi, mode in enumerate(('relu', 'softplus') if S <= 65 else ('relu',)):       # (softplus up to S = 65: with S = 256 as well the file would pass 1 MiB)
            with torch.no_grad():
                _, _, w = marcher(colors, torch.from_numpy(dens).view(1, IMP_RAYS, S, 1), depths, torch.from_numpy(rd)[None], dict(clamp_mode=mode, white_back=False))
                if mi == 0:
                    # u: multiples of 2^-8 (the file stays small) with the edges on every ray: 0, 1 - 2^-24, 1.0, a duplicated value, and knots of the CDF
                    # of a first recorded run (the fp32 cdf the reference builds for this ray, read back by running sample_pdf's own lines on the weights)
                    u = (np.floor(rs.uniform(0, 1, (IMP_RAYS, N)) * 256) / 256).astype(np.float32)
                    ws = torch.nn.functional.max_pool1d(w.reshape(IMP_RAYS, -1).unsqueeze(1).float(), 2, 1, padding=1)
                    ws = torch.nn.functional.avg_pool1d(ws, 2, 1).squeeze(1) + 0.01
                    wi = ws[:, 1:-1] + 1e-5
                    cdf = torch.cumsum(wi / torch.sum(wi, -1, keepdim=True), -1).numpy()              # the knots behind the leading 0
                    edge = [np.zeros(IMP_RAYS, np.float32), np.full(IMP_RAYS, 1 - 2.0 ** -24, np.float32), np.ones(IMP_RAYS, np.float32), u[:, 0].copy(),
                            np.minimum(cdf[:, 0], 1).astype(np.float32), np.minimum(cdf[:, cdf.shape[1] // 2], 1).astype(np.float32),
                            np.minimum(cdf[:, -1], 1).astype(np.float32)]
                    for j, e in enumerate(edge):
                        if j < N:
                            u[:, N - 1 - j] = e                    # (N = 1: u = 0; N = 2: 0 and 1 - 2^-24; ...; the duplicate needs N >= 5)
                fine = reference_importance(R, depths, w, torch.from_numpy(u))
            out[f'imp{ci}_fine_{mode}'] = torch.sort(fine[0, :, :, 0], dim=-1)[0].numpy()
        out.update({f'imp{ci}_dens': dens, f'imp{ci}_near': near, f'imp{ci}_far': far, f'imp{ci}_rd': rd, f'imp{ci}_u': u})
    path = os.path.join(GOLDEN, 'importance_units.npz')
    np.savez_compressed(path, **out)
    print('units ->', path, f'({os.path.getsize(path) / 1e3:.0f} KB)')
    assert os.path.getsize(path) < 1 << 20
    # ---- unify_samples + MipRayMarcher2 (a file of its own: no committed file may pass 1 MiB) ----
    out = {}
    for ci, (Rr, S, N) in enumerate(((300, 6, 5), (12, 256, 256))):
        near = rs.uniform(1, 2, (Rr, 1)).astype(np.float32)
        far = near + rs.uniform(0.5, 2, (Rr, 1)).astype(np.float32)
        rd = rs.normal(0, 1, (Rr, 3)).astype(np.float32)
        depths = R.ImportanceRenderer.sample_stratified(None, torch.zeros(1, Rr, 3), torch.from_numpy(near)[None], torch.from_numpy(far)[None], S, False)
        z = depths[0, :, :, 0].numpy()
        # fine depths: strictly inside the coarse span, no ties (multiples of 2^-10 of the span off the coarse grid), ascending
        frac = np.stack([np.sort(rs.choice(np.arange(20, 1004), N, replace=False) + 0.37) / 1024 for _ in range(Rr)])      # (distinct values per ray)
        fine = (z[:, :1] + frac * (z[:, -1:] - z[:, :1])).astype(np.float32)
        dens_c = (np.round(rs.normal(0, 6, (Rr, S)) * 4) / 4).astype(np.float32)
        dens_f = (np.round(rs.normal(0, 6, (Rr, N)) * 4) / 4).astype(np.float32)
        dens_c[rs.uniform(0, 1, (Rr, S)) < 0.5] = -80.0
        dens_f[rs.uniform(0, 1, (Rr, N)) < 0.5] = -80.0
        if ci == 0:
            dens_c[0] = -80.0; dens_f[0] = -80.0                  # ray 0: no valid sample
            dens_f[1] = -80.0; dens_c[1] = 2.0                    # ray 1: only coarse valid samples
            dens_c[2] = -80.0; dens_f[2] = 2.0                    # ray 2: only fine valid samples
            fine[3, -1] = z[3, -1] + 0.125; dens_f[3, -1] = 3.0   # ray 3: a fine sample LAST in merged order (behind the last coarse one): the 1e10 delta
            dens_c[3, -1] = -80.0
            fine[4, -1] = z[4, -1] + 0.125; dens_f[4, -1] = -80.0; dens_c[4, -1] = 3.0   # ray 4: the last merged sample is a rejected fine one
        col_c = (np.floor(rs.uniform(0, 1, (Rr, S, 3)) * 256) / 256).astype(np.float32)
        col_f = (np.floor(rs.uniform(0, 1, (Rr, N, 3)) * 256) / 256).astype(np.float32)
        col_c[dens_c == -80.0] = 0; col_f[dens_f == -80.0] = 0
        tt = lambda a: torch.from_numpy(a)
        all_t, all_c, all_s = R.ImportanceRenderer.unify_samples(None, depths, tt(col_c)[None], tt(dens_c)[None, :, :, None], tt(fine)[None, :, :, None],
                                                                 tt(col_f)[None], tt(dens_f)[None, :, :, None])
        assert int((all_t[0, :, 1:, 0] == all_t[0, :, :-1, 0]).sum()) == 0
        out.update({f'mrg{ci}_near': near, f'mrg{ci}_far': far, f'mrg{ci}_rd': rd, f'mrg{ci}_fine': fine, f'mrg{ci}_dens_c': dens_c, f'mrg{ci}_dens_f': dens_f,
                    f'mrg{ci}_col_c': col_c, f'mrg{ci}_col_f': col_f, f'mrg{ci}_shape': np.asarray((Rr, S, N), dtype=np.int64)})
        for mode in ('relu', 'softplus'):
            for wb in (False, True):
                with torch.no_grad():
                    rgb, dep, w = marcher(all_c, all_s, all_t, tt(rd)[None], dict(clamp_mode=mode, white_back=wb))
                out.update({f'mrg{ci}_rgb_{mode}_{int(wb)}': rgb[0].numpy(), f'mrg{ci}_depth_{mode}_{int(wb)}': dep[0, :, 0].numpy(),
                            f'mrg{ci}_acc_{mode}_{int(wb)}': w.sum(2)[0, :, 0].numpy()})
    path = os.path.join(GOLDEN, 'importance_units_merged.npz')
    np.savez_compressed(path, **out)
    print('units ->', path, f'({os.path.getsize(path) / 1e3:.0f} KB)')
    assert os.path.getsize(path) < 1 << 20


if __name__ == '__main__':
    what = sys.argv[1:] or ['frame', 'units']
    R, T = MG.import_reference()
    if 'units' in what:
        run_units(R)
    if 'frame' in what:
        run_frame(R, T)
