"""TEST INFRASTRUCTURE (CPU only, build container).  Goldens of the UNMODIFIED reference on its OSGDecoder path (use_NeRF_decoder=False):

    python tools/make_golden_osg.py [osg osg_notrans osg_softplus osg_notrans_f101 osg_f100]        (default: all five)

  tests/golden/renderer_tiny_ri_osg.npz                use_trans=True, relu
  tests/golden/renderer_tiny_ri_osg_notrans.npz        use_trans=False, relu
  tests/golden/renderer_tiny_ri_osg_softplus.npz       use_trans=True, clamp_mode='softplus'
  tests/golden/renderer_tiny_ri_osg_notrans_f101.npz   use_trans=False, 2-D branch off (W_b is the zero block)
  tests/golden/renderer_tiny_ri_osg_f100.npz           use_trans=True, tri-planes only (no reprojection module)

Each file: the reference's ImportanceRenderer(..., use_NeRF_decoder=False) + OSGDecoder(32, {'decoder_lr_mul': 1, 'decoder_output_dim': 3}) on the
`tiny_ri` fixture -- image (rgb, depth, acc), n_valid, per-sample rgb / sigma, the marcher's weights -- and the decoder's four parameters
(`decoder.net.0.weight` ...), drawn by the reference's own constructor under torch.manual_seed(DECODER_SEED) with the LAST layer multiplied by
`last_layer_scale` (recorded): FullyConnectedLayer's unit-variance initialisation gives |sigma| ~ 1 and an almost empty image on this fixture (and,
the softplus activations being positive, a sigma of one sign per draw: the seed is one whose densities come out positive).
oracle/make_golden.py is used as a library (import_reference); nothing at test time imports this module; the files hold recorded data only.
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
DECODER_SEED = 1
LAST_LAYER_SCALE = 10.0
#        tag                 use_trans  branches             clamp_mode
CASES = {'osg':              (True,     (True, True, True),  'relu'),
         'osg_notrans':      (False,    (True, True, True),  'relu'),
         'osg_softplus':     (True,     (True, True, True),  'softplus'),
         'osg_notrans_f101': (False,    (True, False, True), 'relu'),
         'osg_f100':         (True,     (True, False, False), 'relu')}


def run(tag, R, T):
    use_trans, branches, clamp_mode = CASES[tag]
    fx = fixtures.renderer_inputs(CFG)
    torch.manual_seed(0)
    rend = R.ImportanceRenderer(*branches, use_trans=use_trans, use_NeRF_decoder=False)
    fixtures.load_seeded_state(rend, 'renderer.', fixtures.variant_of(CFG))
    torch.manual_seed(DECODER_SEED)
    dec = T.OSGDecoder(32, {'decoder_lr_mul': 1, 'decoder_output_dim': 3})
    with torch.no_grad():
        dec.net[2].weight.mul_(LAST_LAYER_SCALE)
        dec.net[2].bias.mul_(LAST_LAYER_SCALE)
    rend.train(); dec.train()
    d = fixtures.to_torch(fx['input_data'])
    planes, obs_feat, vfeat = (torch.from_numpy(fx[k]) for k in ('planes', 'obs_feat', 'vertex_feat'))
    obs_img = d['obs_img_all'][:, 0]
    # the glue in front of the renderer with the reference's own functions (triplane.py:129-137), as oracle.make_golden.run does
    smpl_obs_pts = torch.matmul(d['obs_vertices'] - d['obs_params']['Th'], d['obs_params']['R'])
    obs_can = rend.coarse_deform_target2c(d['obs_params'], d['obs_vertices'], d['t_params'], smpl_obs_pts)
    sp_input, _ = T.TriPlaneGenerator.prepare_sp_input(types.SimpleNamespace(), d['t_vertices'].clone(), obs_can)
    import spconv.pytorch as spconv
    sp = spconv.core.SparseConvTensor(vfeat, sp_input['coord'], sp_input['out_sh'], sp_input['batch_size'])
    cap = {}
    knn_calls, orig_knn = [], R.knn_points

    def knn_rec(a, b, K=1):
        out = orig_knn(a, b, K=K)
        knn_calls.append(out[0].clone())
        return out
    R.knn_points = knn_rec
    run_model = rend.run_model

    def run_rec(*a, **k):
        out = run_model(*a, **k)
        cap['rgb'], cap['sigma'] = out['rgb'].clone(), out['sigma'].clone()
        return out
    rend.run_model = run_rec
    rm = rend.ray_marcher.run_forward

    def rm_rec(*a):
        out = rm(*a)
        cap['weights'] = out[2].clone()
        return out
    rend.ray_marcher.run_forward = rm_rec
    opts = dict(fx['options'], clamp_mode=clamp_mode)
    try:
        with torch.no_grad():
            rgb, depth, acc = rend(planes, obs_img, obs_feat, sp, None, sp_input, dec, d['ray_o_all'][:, 0], d['ray_d_all'][:, 0],
                                   d['near_all'][:, 0], d['far_all'][:, 0], d, opts)
    finally:
        R.knn_points = orig_knn
    n_valid = int((knn_calls[0].view(-1) < 0.05 ** 2).sum())
    out = dict(rgb=rgb[0].numpy(), depth=depth[0].numpy(), acc=acc[0].numpy(), n_valid=np.int64(n_valid),
               sample_rgb=cap['rgb'][0].numpy(), sample_sigma=cap['sigma'][0, :, 0].numpy(), weights=cap['weights'][0, :, :, 0].numpy(),
               last_layer_scale=np.float64(LAST_LAYER_SCALE), decoder_seed=np.int64(DECODER_SEED))
    out.update({'decoder.' + k: v.detach().numpy() for k, v in dec.state_dict().items()})
    # is this frame a usable yardstick?  the sampler does not depend on the decoder: the count must be the NeRF golden's; the image must not be
    # empty or saturated
    nerf = np.load(os.path.join(GOLDEN, f'renderer_{CFG}.npz'))
    a = out['acc']
    ok = n_valid == int(nerf['n_valid']) and out['sample_rgb'].shape[0] == n_valid and 0.0 < float(a.max()) and float(a.min()) < 1.0 \
        and 0.02 < float(a.mean()) < 0.98 and float(((a > 0.05) & (a < 0.95)).mean()) > 0.02
    path = os.path.join(GOLDEN, f'renderer_{CFG}_{tag}.npz')
    print(f'{tag}: n_valid {n_valid} (NeRF golden {int(nerf["n_valid"])}); acc min {a.min():.3f} mean {a.mean():.3f} max {a.max():.3f}, '
          f'{float(((a > 0.05) & (a < 0.95)).mean()):.1%} of the rays in (0.05, 0.95); sigma [{out["sample_sigma"].min():.2f}, {out["sample_sigma"].max():.2f}] '
          f'{float((out["sample_sigma"] > 0).mean()):.1%} positive; rgb [{out["rgb"].min():.3f}, {out["rgb"].max():.3f}]; last layer x {LAST_LAYER_SCALE:g} '
          f'-> {"usable yardstick" if ok else "DEGENERATE: not written"}')
    if not ok:
        raise SystemExit(f'{tag}: degenerate golden frame')
    np.savez_compressed(path, **out)
    print(f'  -> {path} ({os.path.getsize(path) / 1e3:.0f} KB)')


if __name__ == '__main__':
    what = sys.argv[1:] or list(CASES)
    R, T = MG.import_reference()
    for tag in what:
        run(tag, R, T)
