"""What does importance sampling cost a frame?  (GPU box only.)

Three frames on the workload bench.py times (`cfg2_dense_ri`, 512 x 512), through `ImportanceRenderer.forward`, interleaved round by round in ONE process:

    S = 48, N = 48      the reference's own setting (train.py:354-355): coarse pass + fine pass + merged compositing
    S = 48, N = 0       the coarse pass alone
    S = 96, N = 0       as many samples per ray, all of them coarse

and the two new kernels alone on the buffers the S = 48 + N = 48 frame left (`sherf_importance_depths`, `sherf_composite_merged`), so that their share of
the frame is a measurement.  HIP events on the caller's stream; `ms_per_frame` = `--frames` frames issued back to back / their number (the importance
frame waits once per frame for its two counts, so its back-to-back figure contains that wait); best and mean over `--repeats` rounds.  The draws `u` are
fixed (one tensor for all frames), the token buffers are sized and the launch form tuned before anything is timed.

    python tools/bench_importance.py [--repeats 7] [--frames 10] [--out profiles/<name>.json]

Prints ONE JSON line.  Without a GPU it fails."""
import argparse
import ctypes
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ARMS = (('S48_N48', 48, 48), ('S48_N0', 48, 0), ('S96_N0', 96, 0))


def frame(w, S, N, u):
    d = w['d']
    opts = dict(w['opts'], depth_resolution=S, depth_resolution_importance=N)
    if N:
        opts['importance_u'] = u
    with torch.no_grad():
        return w['rend'](w['planes'], w['obs_img'], w['obs_feat'], w['sp'], None, w['sp_input'], w['dec'], d['ray_o_all'][:, 0], d['ray_d_all'][:, 0],
                         d['near_all'][:, 0], d['far_all'][:, 0], d, opts)


def time_kernels(w, S, N, u, reps, dev):
    """The two new kernels alone, on what the importance frame just left in the workspaces (the outputs they rewrite are the frame's own: same values)."""
    from sherf_amd import _lib
    frame(w, S, N, u)
    torch.cuda.synchronize(dev)
    last = w['rend'].last
    ws, fw, d = last['ws'], last['importance']['ws'], w['d']
    P = _lib.ptr
    R = last['R']
    rd, nr, fa = (d[k][:, 0].contiguous() for k in ('ray_d_all', 'near_all', 'far_all'))
    ro = d['ray_o_all'][:, 0].contiguous()
    bits = _lib.composite_bits(w['opts'].get('white_back', False), w['opts'].get('clamp_mode', 'relu'))
    out = torch.empty(5 * R, device=dev)
    st = lambda: ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)

    def depths():
        _lib.call('sherf_importance_depths', P(ws['ray_base']), P(ws['ray_cnt']), P(ws['cs_idx']), P(ws['sample_out']), P(ro), P(rd), P(nr), P(fa), R, S, bits,
                  last['cap'], P(u), N, P(fw['depths_fine']), P(fw['points']), st())

    def merged():
        _lib.call('sherf_composite_merged', P(ws['counters']), P(ws['ray_base']), P(ws['ray_cnt']), P(ws['cs_idx']), P(ws['sample_out']), last['cap'],
                  P(fw['depths_fine']), P(fw['ray_mask']), P(fw['ray_base']), P(fw['sample_out']), fw['tok_cap'], P(rd), P(nr), P(fa), R, S, N, bits,
                  ctypes.c_void_p(out.data_ptr()), ctypes.c_void_p(out.data_ptr() + 12 * R), ctypes.c_void_p(out.data_ptr() + 16 * R), st())
    res = {}
    for name, fn in (('sherf_importance_depths', depths), ('sherf_composite_merged', merged)):
        for _ in range(3):
            fn()
        torch.cuda.synchronize(dev)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize(dev)
        res[name] = round(e0.elapsed_time(e1) / reps, 4)
    return res, dict(n_coarse=last['importance']['n_coarse'], n_fine=last['importance']['n_fine'])


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--config', default='cfg2_dense_ri')
    ap.add_argument('--precision', default='auto')
    ap.add_argument('--frames', type=int, default=10)
    ap.add_argument('--repeats', type=int, default=7)
    ap.add_argument('--out', default=None, help='also write the JSON line to this file')
    a = ap.parse_args(argv)
    import bench
    if not torch.cuda.is_available():
        raise SystemExit('tools/bench_importance.py measures on a GPU; none is available (there is no fall-back)')
    dev = bench._device(int(os.environ.get('LOCAL_RANK', 0)))
    w = bench.make_workload(argparse.Namespace(config=a.config, precision=a.precision, bn_mode='train', table_precision=None, encoder_precision=None), 0.4, dev)
    R = w['d']['ray_o_all'].shape[2]
    u = torch.rand(R, 48, generator=torch.Generator().manual_seed(1)).to(dev)
    # the workspace is keyed by (R, S): the S = 48 and S = 96 frames alternate on ONE workspace, which would re-size it every frame -- so each arm is timed in
    # rounds of its own, `frames` frames back to back, the arms interleaved round by round; the first frame of a round (re-sizing, sizing probe) is not timed
    times = {name: [] for name, _, _ in ARMS}
    valid = {}
    for rnd in range(a.repeats + 1):                               # (round 0 warms up: token buffers sized, precision calibrated, launch form tuned)
        for name, S, N in ARMS:
            for _ in range(3):
                frame(w, S, N, u)
            torch.cuda.synchronize(dev)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.frames):
                frame(w, S, N, u)
            e1.record()
            torch.cuda.synchronize(dev)
            if rnd:
                times[name].append(e0.elapsed_time(e1) / a.frames)
            valid[name] = int(w['rend'].last['ws']['counters'][0])
    kernels, counts = time_kernels(w, 48, 48, u, 20, dev)
    last = w['rend'].last
    res = dict(metric='ms per frame at 512x512: S=48 + N=48 importance samples against S=48 and S=96 without', unit='ms', frames=a.frames, repeats=a.repeats,
               ms_per_frame={k: dict(min=round(float(np.min(v)), 4), mean=round(float(np.mean(v)), 4), max=round(float(np.max(v)), 4)) for k, v in times.items()},
               new_kernels_ms=kernels,
               new_kernels_share_of_S48_N48={k: round(v / float(np.mean(times['S48_N48'])), 4) for k, v in kernels.items()},
               valid_samples=dict(coarse_S48=valid['S48_N0'], coarse_S96=valid['S96_N0'], fine_N48=counts['n_fine']),
               config=dict(workload=a.config, rays=R, mlp_precision=last.get('mlp_precision'), mlp_form=last.get('mlp_form'), table_precision=last.get('table_precision'),
                           timing='HIP events on the caller stream; arms interleaved round by round; an importance frame waits once for its two counts'))
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(line + '\n')
    return res


if __name__ == '__main__':
    main()
