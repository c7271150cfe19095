"""TEST INFRASTRUCTURE (CPU only, build container).  Goldens of the UNMODIFIED reference under clamp_mode='softplus':

    python tools/make_golden_softplus.py [marcher] [renderer] [grad]        (default: all three)

  tests/golden/marcher_softplus.npz             MipRayMarcher2 (ray_marcher.py:25-64): inputs, the three outputs under softplus, and the
                                                autograd gradients of a fixed loss w.r.t. colors / densities under relu AND softplus
  tests/golden/renderer_tiny_ri_softplus.npz    ImportanceRenderer on `tiny_ri` (image, per-sample rgb / sigma, weights)
  tests/golden/grad_tiny_nv_softplus.npz        oracle.make_golden.run_grad's fingerprints under softplus

oracle/make_golden.py is used as a library (import_reference, run, run_grad); its fixtures hard-code relu, so the option is overridden
at run time by wrapping `fixtures.renderer_inputs`.  Nothing at test time imports this module; the files hold recorded data only.
"""
import os
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import fixtures, make_golden as MG          # noqa: E402

GOLDEN = os.path.join(ROOT, 'tests', 'golden')
MODES = ('relu', 'softplus')


def softplus_fixtures():
    """fixtures.renderer_inputs with options['clamp_mode'] = 'softplus' (make_golden.run / run_grad look the function up per call)."""
    orig = fixtures.renderer_inputs

    def wrapped(cfg_name, smpl=None):
        fx = dict(orig(cfg_name, smpl))
        fx['options'] = dict(fx['options'], clamp_mode='softplus')
        return fx
    fixtures.renderer_inputs = wrapped
    return orig


def marcher_inputs(rs, Rr, S):
    """[1,Rr,S,*] inputs with the cases the softplus kernels must get right: ray 0 all rejected (sigma = -80: empty ray, NaN depth path),
    ray 1 above F.softplus's threshold (sigma - 1 > 20), ray 2 with equal depths (delta = 0 but for the last sample), ray 3 just around
    the threshold, rejected samples sprinkled over the rest, negative sigma throughout."""
    colors = rs.uniform(0, 1, (1, Rr, S, 3)).astype(np.float32)
    dens = rs.normal(0, 8, (1, Rr, S, 1)).astype(np.float32)
    dens[0, 4:][rs.uniform(0, 1, (Rr - 4, S, 1)) < 0.3] = -80.0
    dens[0, 0] = -80.0
    dens[0, 1, :, 0] = np.linspace(21.5, 40.0, S, dtype=np.float32)
    dens[0, 3, :, 0] = np.linspace(20.5, 21.5, S, dtype=np.float32)
    near = rs.uniform(1, 2, (1, Rr, 1, 1)).astype(np.float32)
    far = near + rs.uniform(0.5, 2, (1, Rr, 1, 1)).astype(np.float32)
    depths = (near + np.linspace(0, 1, S, dtype=np.float32).reshape(1, 1, S, 1) * (far - near)).astype(np.float32)
    depths[0, 2] = depths[0, 2, 0]
    # (thin slabs on a part of the rays: sigma * delta of order one, so that alpha is neither 0 nor 1 and every term of the backward counts)
    thin = np.arange(Rr) % 2 == 1
    thin[:4] = False
    depths[0, thin] = near[0, thin] + (depths[0, thin] - near[0, thin]) * 0.05
    rd = rs.normal(0, 1, (1, Rr, 3)).astype(np.float32)
    return colors, dens, depths, rd


def run_marcher(R):
    from training.volumetric_rendering.ray_marcher import MipRayMarcher2
    rs = np.random.RandomState(23)
    out = {}
    for tag, (Rr, S) in (('', (300, 5)), ('s2_', (300, 2))):
        colors, dens, depths, rd = marcher_inputs(rs, Rr, S)
        # the fixed loss: sum of each output times a seeded tensor
        g_rgb = rs.normal(0, 1, (1, Rr, 3)).astype(np.float32)
        g_dep = rs.normal(0, 1, (1, Rr, 1)).astype(np.float32)
        g_w = rs.normal(0, 1, (1, Rr, S, 1)).astype(np.float32)
        out.update({tag + 'colors': colors, tag + 'dens': dens, tag + 'depths': depths, tag + 'rd': rd,
                    tag + 'g_rgb': g_rgb, tag + 'g_depth': g_dep, tag + 'g_w': g_w})
        for wb in (False, True):
            for mode in MODES:
                c = torch.from_numpy(colors).requires_grad_(True)
                s = torch.from_numpy(dens).requires_grad_(True)
                rgb, dep, w = MipRayMarcher2()(c, s, torch.from_numpy(depths), torch.from_numpy(rd), dict(clamp_mode=mode, white_back=wb))
                if mode == 'softplus':
                    out.update({f'{tag}rgb_{int(wb)}': rgb.detach().numpy(), f'{tag}depth_{int(wb)}': dep.detach().numpy(),
                                f'{tag}w_{int(wb)}': w.detach().numpy()})
                # with and without the depth term: autograd's quotient turns the zero upstream of an EMPTY ray's depth (nan_to_num) into
                # 0 / 0 = NaN, so the full loss's gradient is NaN on that ray; the depth-free loss says what the other outputs contribute there
                for name, loss in (('', (rgb * torch.from_numpy(g_rgb)).sum() + (dep * torch.from_numpy(g_dep)).sum() + (w * torch.from_numpy(g_w)).sum()),
                                   ('nodepth_', (rgb * torch.from_numpy(g_rgb)).sum() + (w * torch.from_numpy(g_w)).sum())):
                    dc, ds = torch.autograd.grad(loss, (c, s), retain_graph=True)
                    out[f'{tag}{name}d_colors_{mode}_{int(wb)}'] = dc.numpy()
                    out[f'{tag}{name}d_dens_{mode}_{int(wb)}'] = ds.numpy()
                    print(f'marcher {tag or "s5_"}{name}{mode} wb={int(wb)}: non-finite gradient entries {int((~torch.isfinite(ds)).sum())} (sigma) '
                          f'{int((~torch.isfinite(dc)).sum())} (colors); max |d sigma| {float(ds[torch.isfinite(ds)].abs().max()):.3e}')
    path = os.path.join(GOLDEN, 'marcher_softplus.npz')
    np.savez_compressed(path, **out)
    print('marcher ->', path, f'({os.path.getsize(path) / 1e3:.0f} KB)')


KEEP = ('rgb', 'depth', 'acc', 'n_valid', 'sample_rgb', 'sample_sigma', 'weights')


def run_renderer(R, T):
    with tempfile.TemporaryDirectory() as tmp:
        MG.run('tiny_ri', R, T, tmp)
        g = np.load(os.path.join(tmp, 'renderer_tiny_ri.npz'))
        path = os.path.join(GOLDEN, 'renderer_tiny_ri_softplus.npz')
        np.savez_compressed(path, **{k: g[k] for k in KEEP})
    print('renderer ->', path, f'({os.path.getsize(path) / 1e3:.0f} KB)')


def run_grad(R, T):
    with tempfile.TemporaryDirectory() as tmp:
        MG.run_grad('tiny_nv', R, T, tmp)
        g = np.load(os.path.join(tmp, 'grad_tiny_nv.npz'))
        path = os.path.join(GOLDEN, 'grad_tiny_nv_softplus.npz')
        np.savez_compressed(path, **{k: g[k] for k in g.files})
    print('grad ->', path, f'({os.path.getsize(path) / 1e3:.0f} KB)')


if __name__ == '__main__':
    what = sys.argv[1:] or ['marcher', 'renderer', 'grad']
    R, T = MG.import_reference()
    softplus_fixtures()
    if 'marcher' in what:
        run_marcher(R)
    if 'renderer' in what:
        run_renderer(R, T)
    if 'grad' in what:
        run_grad(R, T)
