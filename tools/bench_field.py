"""What does a field query cost?  (GPU box only.)

A 256^3 `sherf_amd.field.density_grid` over the posed subject's box on the workload bench.py times as `cfg2_dense_ri` (the workload's own planes and
feature map stand in for the producers' outputs: the hot path is ImportanceRenderer.query_points), against the FRAME of that workload (512 x 512 x 64)
timed in the same process with the same binary.  The expectation from the code: a query costs what a frame with the same number of valid samples costs,
less the compositing, plus ~17 B / point of coalesced stores and the 12 B / point the point sampler reads.

    python tools/bench_field.py [--resolution 256] [--repeats 10] [--out profiles/<name>.json]

HIP events on the caller's stream around whole calls (a query waits once per chunk for its count, so this is its wall time on the device); the per-stage
split comes from the native driver's own event ring (sherf_profile_frames).  Prints ONE JSON line.  Without a GPU it fails."""
import argparse
import ctypes
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


class WorkloadField:
    """density_grid's view of a generator whose producers' outputs are the workload's tensors."""

    def __init__(self, w):
        self.w = w

    def sample_mixed(self, points, dirs, ws, input_data=None):
        w = self.w
        return w['rend'].query_points(w['planes'], w['obs_img'], w['obs_feat'], w['sp'], None, w['sp_input'], w['dec'], points, dirs, input_data, w['opts'])


def stage_split(run, n):
    """Mean over `n` profiled runs of the driver's timeline [ms since the call's first event]."""
    from sherf_amd import _lib
    _lib.call('sherf_profile_frames', 1)
    try:
        for _ in range(n):
            run()
        torch.cuda.synchronize()
        buf, got = (ctypes.c_float * (8 * 64))(), ctypes.c_int32(0)
        _lib.call('sherf_profile_frames_read', buf, 64, ctypes.byref(got))
    finally:
        _lib.call('sherf_profile_frames', 0)
    rows = np.array(list(buf)[:8 * got.value], np.float64).reshape(-1, 8)[-n:]
    m = rows.mean(0)
    return dict(first_phase_until_encoder_join=round(m[3], 4), gather=round(m[4] - m[3], 4), network=round(m[5] - m[4], 4), last_stage=round(m[6] - m[5], 4),
                total=round(m[6], 4), encoder_done=round(m[2], 4), host_enqueue=round(m[0], 4), calls=int(len(rows)))


def timed(run, repeats, dev):
    ms = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize(dev)
        a.record()
        run()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return dict(median=round(float(np.median(ms)), 4), min=round(float(np.min(ms)), 4), max=round(float(np.max(ms)), 4), n=repeats)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--config', default='cfg2_dense_ri')
    ap.add_argument('--precision', default='auto')
    ap.add_argument('--resolution', type=int, default=256)
    ap.add_argument('--repeats', type=int, default=10)
    ap.add_argument('--out', default=None, help='also write the JSON line to this file')
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit('tools/bench_field.py measures on a GPU; none is available (there is no fall-back)')
    import bench
    from sherf_amd import field
    dev = bench._device(int(os.environ.get('LOCAL_RANK', 0)))
    w = bench.make_workload(argparse.Namespace(config=a.config, precision=a.precision, bn_mode='train', table_precision=None, encoder_precision=None), 0.4, dev)
    rend, d = w['rend'], w['d']
    G = WorkloadField(w)
    ws = torch.zeros(1, 1, 1, device=dev)                       # (3-D: density_grid takes the sample_mixed route)
    frame = lambda: bench.render_frame(w)
    grid = lambda: field.density_grid(G, ws, None, d, a.resolution)
    for _ in range(3):                                          # token buffers sized, launch form tuned -- for both
        frame()
        sigma, _, mask, bounds = grid()
    torch.cuda.synchronize(dev)
    n_pts = int(mask.numel())
    nv_q = int(sum(rend.last_query['counts']))
    nv_f = int(rend.last['ws']['counters'][0])
    assert int(mask.sum()) == nv_q and bool(torch.isfinite(sigma).all())
    t_f, t_q = timed(frame, a.repeats, dev), timed(grid, a.repeats, dev)
    s_f, s_q = stage_split(frame, 5), stage_split(grid, 5)
    R, S = d['ray_o_all'].shape[2], int(w['opts']['depth_resolution'])
    res = dict(metric='a %d^3 density grid through the field query against the frame of the same workload' % a.resolution, unit='ms',
               config=dict(workload=a.config, mlp_precision=rend.last_query['mlp_precision'], table_precision=rend.last_query['table_precision'],
                           encoder_precision=rend.last_query['encoder_precision'], mlp_form=rend.last_query['mlp_form'], chunks=len(rend.last_query['counts']),
                           bounds=[[round(float(v), 4) for v in r] for r in bounds.tolist()],
                           timing='HIP events on the caller stream around whole calls; stage split from the driver\'s event ring'),
               query=dict(points=n_pts, valid=nv_q, valid_fraction=round(nv_q / n_pts, 5), ms=t_q, points_per_s=round(n_pts / (t_q['median'] * 1e-3)),
                          ns_per_valid_point=round(t_q['median'] * 1e6 / max(nv_q, 1), 3), stages_ms=s_q, token_capacity=rend.last_query['cap']),
               frame=dict(samples=R * S, valid=nv_f, valid_fraction=round(nv_f / (R * S), 5), ms=t_f, ns_per_valid_sample=round(t_f['median'] * 1e6 / max(nv_f, 1), 3),
                          stages_ms=s_f))
    res['query_ms_per_frame_ms_at_equal_valid_count'] = round((t_q['median'] / max(nv_q, 1)) / (t_f['median'] / max(nv_f, 1)), 4)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(line + '\n')
    return res


if __name__ == '__main__':
    main()
