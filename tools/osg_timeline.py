"""Per-stage times of the OSG frame (use_NeRF_decoder=False), both use_trans values, beside the NeRF frame, from ONE process on one board (GPU box only):

    python tools/osg_timeline.py [--config cfg2_dense_ri] [--precision f16x3] [--frames 12] [--out profiles/<name>.txt]

Every arm renders the bench frame (bench.make_workload: 512 x 512 rays x 64 samples for cfg2_dense_ri) with the same renderer weights; the OSG arms swap the
decoder (a seeded OSGDecoder, last layer x 10 as in tools/make_golden_osg.py) and the renderer's switch.  Times are the native driver's HIP-event timeline
(sherf_profile_frames_*: ms since the frame's first event, mean and minimum over the frames; `mlp_ms` = the per-sample network's launch alone), arms
interleaved over three rounds after a warm-up.  bench.py is not touched."""
import argparse
import ctypes as ct
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NAMES = ('host_enqueue', 'smpl_tables_done', 'encoder_done', 'rays_at_encoder_join', 'gather_done', 'mlp_done', 'frame_done', 'mlp_ms')


def timeline(bench, w, frames):
    from sherf_amd import _lib
    for _ in range(3):
        bench.render_frame(w)
    torch.cuda.synchronize()
    _lib.call('sherf_profile_frames', 1)
    for _ in range(frames):
        bench.render_frame(w)
    torch.cuda.synchronize()
    ms = (ct.c_float * (64 * 8))(); n = ct.c_int32(0)
    _lib.call('sherf_profile_frames_read', ms, 64, ct.byref(n))
    _lib.call('sherf_profile_frames', 0)
    return np.array(ms[:n.value * 8], dtype=np.float64).reshape(-1, 8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--config', default='cfg2_dense_ri')
    ap.add_argument('--precision', default='f16x3', help="tables / encoder precision of every arm ('f16x3': fp32 tables, 'f16': fp16 tables)")
    ap.add_argument('--frames', type=int, default=12)
    ap.add_argument('--out', default='')
    a = ap.parse_args()
    import bench
    from sherf_amd.renderer import ImportanceRenderer
    from sherf_amd.triplane import OSGDecoder
    from synthdata import fixtures, synth
    dev = torch.device('cuda', 0)
    torch.cuda.set_device(0)
    nerf = bench.make_workload(argparse.Namespace(config=a.config, precision=a.precision, bn_mode='train'), 0.4, dev)
    nerf['opts']['mlp_form'] = 'pipelined'                      # (no form tuning inside the timed frames)
    arms = {'nerf': nerf}
    for use_trans in (True, False):
        rend = ImportanceRenderer(True, True, True, use_trans=use_trans, use_NeRF_decoder=False, smpl=synth.make_synth_smpl(0), mlp_precision=a.precision)
        fixtures.load_seeded_state(rend, 'renderer.', fixtures.variant_of(a.config))
        torch.manual_seed(1)
        dec = OSGDecoder(32, {'decoder_lr_mul': 1, 'decoder_output_dim': 3})
        with torch.no_grad():
            dec.net[2].weight.mul_(10.0)
        arms['osg' if use_trans else 'osg_notrans'] = dict(nerf, rend=rend.to(dev).train(), dec=dec.to(dev))
    rows = {k: [] for k in arms}
    for rnd in range(3):
        for k, w in arms.items():
            rows[k].append(timeline(bench, w, a.frames))
    lines = []
    for k, w in arms.items():
        last = w['rend'].last
        nv = int(last['ws']['counters'][0])
        prof = np.concatenate(rows[k][1:])                      # (round 0 warms up)
        rec = dict(arm=k, config=a.config, rays=last['R'], samples_per_ray=last['S'], valid_samples=nv, mlp_precision=last['mlp_precision'],
                   table_precision=last['table_precision'], encoder_precision=last['encoder_precision'], frames=int(prof.shape[0]),
                   mean_ms={n: round(float(v), 4) for n, v in zip(NAMES, prof.mean(0))}, min_ms={n: round(float(v), 4) for n, v in zip(NAMES, prof.min(0))},
                   acc_mean=round(float(last['ws']['acc'].mean()), 4), device=torch.cuda.get_device_name(0))
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, 'w').write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
