"""What does reusing the encoded observation buy a sweep?  (GPU box only.)

One observation, eight frames: a CAMERA sweep (theta = k * 2 pi / 8 around the subject: BASELINE config 4's cameras) and a POSE sweep of the same
length (eight target poses, one camera), at 512 x 512 x 64 on the workload bench.py times as `cfg2_dense_ri` -- rendered through
`ImportanceRenderer.forward` (rendering option `reuse_observation`) and through `TriPlaneGenerator.forward` with `use_cached_backbone`
(`use_cached_observation`).  Two arms alternate sweep by sweep in ONE process, same binary, same input tensors: reuse off (what the renderer
enqueues without the option) and reuse on.  Every shape is rendered in both arms before anything is timed.  HIP events on the caller's stream, one
frame in flight: `ms_per_frame` = events around the eight frames issued back to back on the one stream, / 8; `latency_ms_per_frame` = the same with
the host waiting for every frame before it issues the next.

    python tools/bench_sequence.py [--repeats 7] [--out profiles/<name>.json]

Prints ONE JSON line: per-frame ms of both arms with their spread over the repeats, the native {encoded, reused} counters and the generator's
{hits, misses} per arm, and `bit_identical` (every frame of the on arm against the off arm's, all outputs).  Without a GPU it fails."""
import argparse
import json
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

TARGET_KEYS = ('params', 'vertices', 'ray_o_all', 'ray_d_all', 'near_all', 'far_all', 'mask_at_box_all')


def sweep_targets(w, cfg_name, dev, kind, n):
    """n input_data dicts that share `w`'s observation-side tensor OBJECTS (the renderer keys them by identity) and differ on the target side:
    kind 'camera' -- theta = k * 2 pi / n; kind 'pose' -- n target poses under the workload's camera."""
    from synthdata import fixtures, synth
    c = fixtures.CONFIGS[cfg_name]
    smpl = synth.make_synth_smpl(0)
    out = []
    for k in range(n):
        theta, seed, novel = (k * 2.0 * math.pi / n, 1, c['novel_pose']) if kind == 'camera' else (0.4, 2 + k, True)
        other = synth.make_input_data(smpl, H=c['H'], W=c['W'], seed=seed, theta_tgt=theta, theta_obs=c['theta_obs'], novel_pose=novel, fill=c.get('fill', 2.2))
        d = dict(w['d'])
        for key in TARGET_KEYS:
            v = other[key]
            d[key] = ({kk: torch.from_numpy(np.ascontiguousarray(vv)).to(dev) for kk, vv in v.items()} if isinstance(v, dict)
                      else torch.from_numpy(np.ascontiguousarray(v)).to(dev))
        out.append(d)
    return out


def renderer_frame(w, d, reuse):
    opts = dict(w['opts'], reuse_observation=reuse)
    with torch.no_grad():
        return w['rend'](w['planes'], w['obs_img'], w['obs_feat'], w['sp'], None, w['sp_input'], w['dec'], d['ray_o_all'][:, 0], d['ray_d_all'][:, 0],
                         d['near_all'][:, 0], d['far_all'][:, 0], d, opts)


def generator_frame(gen, zc, d, reuse):
    kw = dict(use_sr_module=False, test_flag=True, noise_mode='const', cache_backbone=True, use_cached_backbone=True)
    if reuse:
        kw.update(use_cached_observation=True)                 # (a miss fills the cache: the first frame of the first sweep)
    with torch.no_grad():
        out = gen(d, zc[0], zc[1], **kw)
    return out['image_raw'], out['image_depth'], out['weights_image']


def measure(frame, targets, repeats, dev, mark, stats):
    """Both arms, alternating sweep by sweep.  -> {arm: {...}}, bit_identical"""
    from sherf_amd import _lib
    sync = lambda: torch.cuda.synchronize(dev)
    for _ in range(2):                                         # every shape, both arms: token buffers sized, precision calibrated, launch form tuned
        for reuse in (False, True):
            for d in targets:
                frame(d, reuse)
    sync()
    keep = {False: [], True: []}
    # the frames themselves, once per arm, kept for the comparison -- under the library's deterministic convolution algorithms: with the default ones
    # ResNet-18's code (recomputed every frame in the off arm) moves by 1e-7 from run to run, reuse or not.  The timed sweeps run on the defaults.
    was = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True
    try:
        for reuse in (False, True):
            for d in targets:
                keep[reuse].append([t.clone() for t in frame(d, reuse)])
        sync()
    finally:
        torch.backends.cudnn.deterministic = was
    same = all(torch.equal(a, b) for fa, fb in zip(keep[False], keep[True]) for a, b in zip(fa, fb))
    finite = all(bool(torch.isfinite(t).all()) for f in keep[True] for t in f)
    del keep
    res = {arm: dict(sweep=[], latency=[], first=[], rest=[]) for arm in ('off', 'on')}
    counters = {arm: dict(encoded=0, reused=0, hits=0, misses=0) for arm in ('off', 'on')}       # over the timed sweeps of the arm
    for _ in range(repeats):
        for arm, reuse in (('off', False), ('on', True)):
            n0, g0 = _lib.frame_observation_stats(), dict(stats())
            sync()
            e0, e1 = mark(), mark()                            # back to back on the one stream
            e0.record()
            for d in targets:
                frame(d, reuse)
            e1.record()
            sync()
            res[arm]['sweep'].append(e0.elapsed_time(e1) / len(targets))
            per = []
            for d in targets:                                  # the host waits for every frame
                a, b = mark(), mark()
                a.record()
                frame(d, reuse)
                b.record()
                sync()
                per.append(a.elapsed_time(b))
            res[arm]['latency'].append(float(np.mean(per)))
            res[arm]['first'].append(per[0])
            res[arm]['rest'].append(float(np.mean(per[1:])))
            n1, g1 = _lib.frame_observation_stats(), dict(stats())
            c = counters[arm]
            c['encoded'] += n1[0] - n0[0]
            c['reused'] += n1[1] - n0[1]
            for k in g1:
                c[k] += g1[k] - g0[k]

    def summary(v):
        return dict(mean=round(float(np.mean(v)), 4), min=round(float(np.min(v)), 4), max=round(float(np.max(v)), 4), std=round(float(np.std(v)), 4))
    out = {}
    for arm in ('off', 'on'):
        r, c = res[arm], counters[arm]
        out[arm] = dict(ms_per_frame=summary(r['sweep']), latency_ms_per_frame=summary(r['latency']), latency_ms_first_frame_of_sweep=summary(r['first']),
                        latency_ms_later_frames=summary(r['rest']),
                        native_observation_stats=dict(encoded=c['encoded'], reused=c['reused']), generator_cache_stats=dict(hits=c['hits'], misses=c['misses']))
    out['saving_ms_per_frame'] = round(out['off']['ms_per_frame']['mean'] - out['on']['ms_per_frame']['mean'], 4)
    out['saving_latency_ms_per_frame'] = round(out['off']['latency_ms_per_frame']['mean'] - out['on']['latency_ms_per_frame']['mean'], 4)
    out['bit_identical'] = bool(same)
    out['finite'] = bool(finite)
    return out


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--config', default='cfg2_dense_ri')
    ap.add_argument('--precision', default='auto')
    ap.add_argument('--frames', type=int, default=8)
    ap.add_argument('--repeats', type=int, default=7)
    ap.add_argument('--out', default=None, help='also write the JSON line to this file')
    ap.add_argument('--no-generator', action='store_true')
    ap.add_argument('--small-backbone', action='store_true', help='TEST ONLY: a narrow tri-plane generator (the host-build dry run of this script)')
    a = ap.parse_args(argv)
    import bench
    import bench_generator as BG
    if os.environ.get('SHERF_HIPCPU_LIB'):                     # TEST INFRASTRUCTURE (bench._use_host_build): the script's plumbing on the host build
        bench._use_host_build()
        BG._Mark.on_gpu = False
    elif not torch.cuda.is_available():
        raise SystemExit('tools/bench_sequence.py measures on a GPU; none is available (there is no fall-back)')
    dev = bench._device(int(os.environ.get('LOCAL_RANK', 0)))
    w = bench.make_workload(argparse.Namespace(config=a.config, precision=a.precision, bn_mode='train', table_precision=None, encoder_precision=None), 0.4, dev)
    sweeps = {kind: sweep_targets(w, a.config, dev, kind, a.frames) for kind in ('camera', 'pose')}
    R = w['d']['ray_o_all'].shape[2]
    res = dict(metric='ms per frame of an eight-frame sweep over one observation, reuse of the encoded observation off / on', unit='ms', frames=a.frames,
               repeats=a.repeats, config=dict(workload=a.config, rays=R, samples_per_ray=int(w['opts']['depth_resolution']),
                                              cameras='theta = k * 2 pi / %d' % a.frames, poses='%d target poses (seeds 2..), theta 0.4' % a.frames,
                                              timing='HIP events on the caller stream, one frame in flight; arms alternate sweep by sweep'))
    no_stats = lambda: {}
    res['renderer'] = {kind: measure(lambda d, reuse: renderer_frame(w, d, reuse), t, a.repeats, dev, BG._Mark, no_stats) for kind, t in sweeps.items()}
    res['config']['mlp_precision'], res['config']['mlp_form'] = w['rend'].last.get('mlp_precision'), w['rend'].last.get('mlp_form')
    res['config']['table_precision'], res['config']['encoder_precision'] = w['rend'].last.get('table_precision'), w['rend'].last.get('encoder_precision')
    if not a.no_generator:
        gen = BG.build_generator(w, dev, small=a.small_backbone)
        zc = (torch.randn(1, 512, generator=torch.Generator().manual_seed(1)).to(dev), torch.zeros(1, 25, device=dev))
        res['generator_use_cached_backbone'] = {kind: measure(lambda d, reuse: generator_frame(gen, zc, d, reuse), t, a.repeats, dev, BG._Mark,
                                                              lambda: gen.observation_cache_stats) for kind, t in sweeps.items()}
        res['config']['graph_producers'] = bool(gen.graph_producers)
    res['bit_identical'] = all(v['bit_identical'] for grp in ('renderer', 'generator_use_cached_backbone') if grp in res for v in res[grp].values())
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(line + '\n')
    return res


if __name__ == '__main__':
    main()
