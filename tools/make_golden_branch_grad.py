"""TEST INFRASTRUCTURE (CPU only, build container).  Golden GRADIENTS of the UNMODIFIED reference with a feature branch switched off
(use_1d_feature / use_2d_feature / use_3d_feature, renderer.py:261-269, 405-425):

    python tools/make_golden_branch_grad.py [f110 f101 f011 f100 notrans_f101 osg_notrans_f101 osg_f100]        (default: all seven)

  tests/golden/grad_tiny_ri_f110.npz ... _f100.npz       NeRFDecoder, use_trans=True
  tests/golden/grad_tiny_ri_notrans_f101.npz             NeRFDecoder, use_trans=False
  tests/golden/grad_tiny_ri_osg_notrans_f101.npz         OSGDecoder, use_trans=False     (decoder parameters: renderer_tiny_ri_osg_notrans_f101.npz)
  tests/golden/grad_tiny_ri_osg_f100.npz                 OSGDecoder, use_trans=True      (decoder parameters: renderer_tiny_ri_osg_f100.npz)

Each file: forward + backward (training mode) of the reference's ImportanceRenderer built with the tag's switches on the `tiny_ri` fixture under
oracle.make_golden.loss_targets' stub loss, the modules constructed as oracle.make_golden.run(..., branches=) / tools/make_golden_osg.py construct
them -- `loss`; oracle.make_golden.grad_fingerprint of every gradient that EXISTS (parameters and the three feature inputs `input.planes`,
`input.obs_feat`, `input.vertex_feat`); `none_names`: the names whose .grad is None after the step; `encoder_3d_buffers_changed`: whether any
encoder_3d buffer (BatchNorm running statistics, num_batches_tracked) differs after the step (the reference runs encoder_3d only under
`if self.use_3d_feature`, renderer.py:345-352).
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
#        tag                 use_trans  branches              decoder
CASES = {'f110':             (True,     (True, True, False),  'nerf'),
         'f101':             (True,     (True, False, True),  'nerf'),
         'f011':             (True,     (False, True, True),  'nerf'),
         'f100':             (True,     (True, False, False), 'nerf'),
         'notrans_f101':     (False,    (True, False, True),  'nerf'),
         'osg_notrans_f101': (False,    (True, False, True),  'osg'),
         'osg_f100':         (True,     (True, False, False), 'osg')}
DEC_KEYS = ('net.0.weight', 'net.0.bias', 'net.2.weight', 'net.2.bias')


def run(tag, R, T):
    use_trans, branches, kind = CASES[tag]
    fx = fixtures.renderer_inputs(CFG)
    torch.manual_seed(0)
    rend = R.ImportanceRenderer(*branches, use_trans=use_trans, use_NeRF_decoder=kind == 'nerf')
    if kind == 'nerf':
        dec = T.NeRFDecoder(32)
        fixtures.load_seeded_state(rend, 'renderer.', fixtures.variant_of(CFG))
        fixtures.load_seeded_state(dec, 'decoder.', fixtures.variant_of(CFG))
    else:
        fixtures.load_seeded_state(rend, 'renderer.', fixtures.variant_of(CFG))
        dec = T.OSGDecoder(32, {'decoder_lr_mul': 1, 'decoder_output_dim': 3})
        rec = np.load(os.path.join(GOLDEN, f'renderer_{CFG}_{tag}.npz'))
        dec.load_state_dict({k: torch.from_numpy(rec['decoder.' + k]) for k in DEC_KEYS})
    rend.train(); dec.train()
    d = fixtures.to_torch(fx['input_data'])
    leaves = {'input.planes': torch.from_numpy(fx['planes']).requires_grad_(True),
              'input.obs_feat': torch.from_numpy(fx['obs_feat']).requires_grad_(True),
              'input.vertex_feat': torch.from_numpy(fx['vertex_feat']).requires_grad_(True)}
    obs_img = d['obs_img_all'][:, 0]
    with torch.no_grad():
        smpl_obs_pts = torch.matmul(d['obs_vertices'] - d['obs_params']['Th'], d['obs_params']['R'])
        obs_can = rend.coarse_deform_target2c(d['obs_params'], d['obs_vertices'], d['t_params'], smpl_obs_pts)
    sp_input, _ = T.TriPlaneGenerator.prepare_sp_input(types.SimpleNamespace(), d['t_vertices'].clone(), obs_can)
    import spconv.pytorch as spconv
    sp = spconv.core.SparseConvTensor(leaves['input.vertex_feat'], sp_input['coord'], sp_input['out_sh'], sp_input['batch_size'])
    before = {k: v.clone() for k, v in rend.encoder_3d.named_buffers()}
    rgb, depth, acc = rend(leaves['input.planes'], obs_img, leaves['input.obs_feat'], sp, None, sp_input, dec, d['ray_o_all'][:, 0],
                           d['ray_d_all'][:, 0], d['near_all'][:, 0], d['far_all'][:, 0], d, dict(fx['options']))
    t_rgb, t_acc = MG.loss_targets(rgb.shape, acc.shape)
    loss = ((rgb - t_rgb) ** 2).mean() + ((acc - t_acc) ** 2).mean()
    loss.backward()
    changed = any(not torch.equal(v, before[k]) for k, v in rend.encoder_3d.named_buffers())
    full, none_names = {}, []
    for name, t in leaves.items():
        if t.grad is None:
            none_names.append(name)
        else:
            full[name] = t.grad
    for prefix, mod in (('renderer.', rend), ('decoder.', dec)):
        for name, p_ in mod.named_parameters():
            if p_.grad is None:
                none_names.append(prefix + name)
            else:
                full[prefix + name] = p_.grad
    out = {'loss': np.float64(loss.item()), 'none_names': np.array(sorted(none_names)), 'encoder_3d_buffers_changed': np.bool_(changed)}
    bad = []
    print(f'{tag}: loss {loss.item():.6f}, {len(full)} gradients, {len(none_names)} names without one, encoder_3d buffers {"moved" if changed else "unchanged"}')
    for name, g in full.items():
        norm = float(g.double().norm())
        finite = bool(torch.isfinite(g).all())
        print(f'   {name:60s} |g| {norm:.6e}{"" if finite else "   NON-FINITE"}')
        if not finite or not norm > 0.0:
            bad.append(name)
        out[name] = MG.grad_fingerprint(g)
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
