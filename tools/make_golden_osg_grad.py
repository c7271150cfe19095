"""TEST INFRASTRUCTURE (CPU only, build container).  Golden GRADIENTS of the UNMODIFIED reference on its OSGDecoder path (use_NeRF_decoder=False):

    python tools/make_golden_osg_grad.py [osg osg_notrans osg_softplus]        (default: all three)

  tests/golden/grad_tiny_ri_osg.npz             use_trans=True, relu
  tests/golden/grad_tiny_ri_osg_notrans.npz     use_trans=False, relu
  tests/golden/grad_tiny_ri_osg_softplus.npz    use_trans=True, clamp_mode='softplus'

Each file: forward + backward (training mode) of the reference's ImportanceRenderer(..., use_NeRF_decoder=False) + OSGDecoder on the `tiny_ri`
fixture under oracle.make_golden.loss_targets' stub loss, the decoder holding the parameters recorded in tests/golden/renderer_tiny_ri_osg.npz
(tools/make_golden_osg.py) -- `loss`, oracle.make_golden.grad_fingerprint of every parameter's gradient and of the three feature inputs'
(`input.planes`, `input.obs_feat`, `input.vertex_feat`), and the four decoder gradients IN FULL (`full.decoder.net.0.weight` ...: 2372 floats).
A file in which a recorded gradient is non-finite or has zero norm is not written.
oracle/make_golden.py is used as a library (import_reference, grad_fingerprint, loss_targets); nothing at test time imports this module; the files
hold recorded data only.
"""
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import fixtures, make_golden as MG          # noqa: E402

GOLDEN = os.path.join(ROOT, 'tests', 'golden')
CFG = 'tiny_ri'
#        tag             use_trans  clamp_mode
CASES = {'osg':          (True,     'relu'),
         'osg_notrans':  (False,    'relu'),
         'osg_softplus': (True,     'softplus')}
DEC_KEYS = ('net.0.weight', 'net.0.bias', 'net.2.weight', 'net.2.bias')


def run(tag, R, T):
    use_trans, clamp_mode = CASES[tag]
    fx = fixtures.renderer_inputs(CFG)
    torch.manual_seed(0)
    rend = R.ImportanceRenderer(True, True, True, use_trans=use_trans, use_NeRF_decoder=False)
    fixtures.load_seeded_state(rend, 'renderer.', fixtures.variant_of(CFG))
    dec = T.OSGDecoder(32, {'decoder_lr_mul': 1, 'decoder_output_dim': 3})
    rec = np.load(os.path.join(GOLDEN, f'renderer_{CFG}_osg.npz'))
    dec.load_state_dict({k: torch.from_numpy(rec['decoder.' + k]) for k in DEC_KEYS})
    rend.train(); dec.train()
    d = fixtures.to_torch(fx['input_data'])
    planes = torch.from_numpy(fx['planes']).requires_grad_(True)
    obs_feat = torch.from_numpy(fx['obs_feat']).requires_grad_(True)
    vfeat = torch.from_numpy(fx['vertex_feat']).requires_grad_(True)
    obs_img = d['obs_img_all'][:, 0]
    with torch.no_grad():
        smpl_obs_pts = torch.matmul(d['obs_vertices'] - d['obs_params']['Th'], d['obs_params']['R'])
        obs_can = rend.coarse_deform_target2c(d['obs_params'], d['obs_vertices'], d['t_params'], smpl_obs_pts)
    sp_input, _ = T.TriPlaneGenerator.prepare_sp_input(types.SimpleNamespace(), d['t_vertices'].clone(), obs_can)
    import spconv.pytorch as spconv
    sp = spconv.core.SparseConvTensor(vfeat, sp_input['coord'], sp_input['out_sh'], sp_input['batch_size'])
    opts = dict(fx['options'], clamp_mode=clamp_mode)
    rgb, depth, acc = rend(planes, obs_img, obs_feat, sp, None, sp_input, dec, d['ray_o_all'][:, 0], d['ray_d_all'][:, 0],
                           d['near_all'][:, 0], d['far_all'][:, 0], d, opts)
    t_rgb, t_acc = MG.loss_targets(rgb.shape, acc.shape)
    loss = ((rgb - t_rgb) ** 2).mean() + ((acc - t_acc) ** 2).mean()
    loss.backward()
    full = {'input.planes': planes.grad, 'input.obs_feat': obs_feat.grad, 'input.vertex_feat': vfeat.grad}
    n_none = 0
    for prefix, mod in (('renderer.', rend), ('decoder.', dec)):
        for name, p_ in mod.named_parameters():
            if p_.grad is None:
                n_none += 1
                continue
            full[prefix + name] = p_.grad
    out = {'loss': np.float64(loss.item())}
    bad = []
    print(f'{tag}: loss {loss.item():.6f}, {len(full)} gradients ({n_none} parameters without grad)')
    for name, g in full.items():
        norm = float(g.double().norm())
        finite = bool(torch.isfinite(g).all())
        print(f'   {name:60s} |g| {norm:.6e}{"" if finite else "   NON-FINITE"}')
        if not finite or not norm > 0.0:
            bad.append(name)
        out[name] = MG.grad_fingerprint(g)
    for k in DEC_KEYS:
        out['full.decoder.' + k] = full['decoder.' + k].detach().numpy().astype(np.float32)
    if bad or not np.isfinite(out['loss']):
        raise SystemExit(f'{tag}: non-finite or zero gradients, not written: {bad}')
    path = os.path.join(GOLDEN, f'grad_{CFG}_{tag}.npz')
    np.savez_compressed(path, **out)
    print(f'  -> {path} ({os.path.getsize(path) / 1e3:.0f} KB)')


if __name__ == '__main__':
    what = sys.argv[1:] or list(CASES)
    R, T = MG.import_reference()
    for tag in what:
        run(tag, R, T)
