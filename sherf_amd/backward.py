"""Backward of the rendering hot path (BASELINE config 5: forward render + backward through HIP kernels).

How it is verified:
  * the mathematics: oracle/backward_explicit.py (hand-derived backward) == autograd through the oracle == the unmodified
    reference's gradients (tests/test_backward_math.py, tests/golden/grad_*.npz);
  * the orchestration (shapes, strides, transposition flags, accumulation, order): the functions below run on the CPU against
    a torch emulation of every C entry point and reproduce those gradients (tests/test_backward_dense.py);
  * the kernels (csrc/bwd_dense.hip, csrc/bwd_gemm.hip, csrc/bwd_encoder.hip, and the backward entry points of the forward library):
    from their unchanged source on the CPU (tests/test_hipcpu_kernels.py, tests/test_hipcpu_frame.py) and on the MI355X against the
    reference's gradient fingerprints (tests/test_gpu_backward.py, part of `-m gpu`).

Stages (backward order):  composite  ->  dense (decoder + transformer; NeRFDecoder: backward_dense.py, OSGDecoder: backward_osg.py)  ->  taps / slot fusion
->  sparse encoder.
"""
import ctypes

import torch

from . import _lib
from .backward_dense import HipOps, Mat, dense_backward
from .backward_encoder import encoder_backward
from .backward_osg import head_gains, osg_dense_backward
from .backward_taps import taps_backward


def composite_backward(renderer, d_rgb, d_acc, ray_directions, near, far, white_back=False, clamp_mode='relu'):
    """Gradient of the loss w.r.t. the per-sample (rgb, sigma) produced by the last `renderer.forward` call.

    d_rgb [1,R,3], d_acc [1,R,1] (or [R,3] / [R]): gradients w.r.t. the outputs of ImportanceRenderer.forward; the ray
    tensors are the ones that call was given.  Returns [Nv, 4] in the compact sample order of the forward
    (renderer.last['ws']['cs_idx']): columns dL/d rgb (3), dL/d sigma (raw: before the clamp mode's relu / softplus(sigma - 1),
    which must be the mode that forward rendered under)."""
    last = renderer.last
    if last is None:
        raise RuntimeError('composite_backward needs the workspace of a preceding forward call')
    ws, R, S, cap = last['ws'], last['R'], last['S'], last['cap']
    f32 = lambda t, *shape: t.detach().to(dtype=torch.float32).contiguous().view(*shape)
    P = _lib.ptr
    nv, _, _, flags = ws['counters'][:4].tolist()                 # (the forward is long done: the loss has been formed from its output)
    if flags & 2:
        # the kernel walks every ray's base .. base + count; sample_out has only `cap` rows (a no-grad forward sizes the token workspace from the
        # frame's count or a given number; a training forward sizes it for the worst case and cannot get here)
        raise RuntimeError(f'composite_backward: the forward overflowed its token workspace ({cap} rows for {nv} valid samples; its rays beyond the '
                           f'capacity are NaN): render the frame again with a token workspace re-sized from counters[0] = {nv} before a backward')
    # rows of the frame's valid samples only: the kernel touches rows < nv (every ray's base + count lies below it), and the buffer used to be
    # capacity = R x S rows -- a 268 MB zero fill per step at 512 x 512 x 64 for 12 MB of gradient
    out = torch.zeros(max(nv, 1), 4, device=ws['sample_out'].device)
    _lib.call('sherf_composite_compact_bwd', P(ws['ray_base']), P(ws['ray_cnt']), P(ws['cs_idx']), P(ws['sample_out']),
              P(f32(ray_directions, R, 3)), P(f32(near, R)), P(f32(far, R)), R, S, _lib.composite_bits(white_back, clamp_mode),
              P(f32(d_rgb, R, 3)), P(f32(d_acc, R)), P(out), _lib.stream())
    return out[:nv]


def render_backward(renderer, decoder, d_rgb, d_acc):
    """Full backward of the last `renderer.forward(...)` (training mode).  d_rgb [1,R,3], d_acc [1,R,1].
    -> dict(params={reference name: grad}, planes [1,3,32,P,P], obs_feat [1,64,Hf,Wf], vertex_feat [N,32]).
    A renderer with a feature branch switched off (renderer.feature_branches()): the dense stage and the tap backward read the EFFECTIVE reprojection
    matrix, the scatter leaves the absent branches' taps out (sherf_gather_tokens_bwd_masked), the sparse encoder's backward runs only with the voxel
    branch; `params` holds the parameters the reference's autograd reaches, and an absent branch's input gradient is None."""
    last = renderer.last
    if last is None or 'bwd' not in last:
        raise RuntimeError('render_backward needs a preceding forward call')
    ws, pl, b = last['ws'], last['plan'], last['bwd']
    dev = ws['sample_out'].device
    # ---- a16 ----  (first: it refuses a frame whose forward overflowed its token workspace before anything is launched)
    d_sample = composite_backward(renderer, d_rgb, d_acc, b['ray_d'], b['near'], b['far'], b['white_back'], b.get('clamp_mode', 'relu')).contiguous()
    f32 = lambda t: t.detach().to(dtype=torch.float32).contiguous()
    state = {'renderer.' + k: v for k, v in renderer.state_dict().items()}
    state.update({'decoder.' + k: v for k, v in decoder.state_dict().items()})
    on = renderer.feature_branches()
    if sum(on) != 3:
        # the forward's effective [32, 96] matrix + bias under the module's names (as _pack_stream / _pack_osg read it): the slot-2 completion and the
        # tap backward see a zero block for an absent branch, the identity for the tri-planes alone
        Wr, br = renderer._effective_reprojection()
        state['renderer.conv1d_reprojection.weight'], state['renderer.conv1d_reprojection.bias'] = Wr[:, :, None], br
    ops = HipOps()
    n = d_sample.shape[0]
    if n == 0:
        raise RuntimeError('render_backward: no valid sample in the last frame')
    # ---- a13 + a14 ----
    tok, ext = Mat.empty(n, 96, dev), Mat.empty(n, 12, dev)                 # (sherf_bwd_untile writes both in full)
    ops.untile(ws['tokens'], ws['extras'], n, tok, ext)
    use_trans = getattr(renderer, 'transformer', None) is not None
    if renderer.use_NeRF_decoder:
        d_tin, grads, dWb_pe = dense_backward(ops, state, tok, ext, Mat(d_sample.view(-1), n, 4), use_trans=use_trans)
    else:                                                                   # OSGDecoder: one fused kernel for the head (backward_osg.py)
        d_tin, grads, dWb_pe = osg_dense_backward(ops, state, tok, ext, Mat(d_sample.view(-1), n, 4), use_trans, head_gains(decoder))
    # ---- a10-a13 ----
    planes, obs_feat = f32(b['planes']), f32(b['obs_feat'])
    P_, (Hf, Wf) = planes.shape[-1], obs_feat.shape[-2:]
    L, meta, shapes = pl['L'], pl['meta'], pl['shapes']
    tap_meta = [m for m in meta if m['tap']]
    levels_ctx = [dict(raw=Mat.of(m['out']), bnparam=Mat(m['bnp'].view(-1), 1, 3 * m['cout']), n_rows=L[m['lev']]['n_rows'],
                       cap=L[m['lev']]['cap'], C=m['cout']) for m in tap_meta]
    bounds, vox_min = f32(b['bounds']).view(6), f32(b['vox_min']).view(3)
    vox_sh = (ctypes.c_int32 * 3)(*b['vox_sh'])

    def scatter(d_tiled, d_planes_f, d_feat_f, d_rows, d_bias):
        # samples binned by coarse voxel cell, accumulated in LDS windows, one device atomic per touched address per bin (the direct
        # form, sherf_gather_tokens_bwd: 20.3 ms of same-address atomics per step at 512 x 512 x 64)
        words = ctypes.c_int64(0)
        _lib.call('sherf_gather_bwd_scratch_words', last['levels_struct'], last['cap'], ctypes.byref(words))
        scratch = torch.empty(words.value, dtype=torch.int32, device=dev)
        p = lambda m: None if m is None else ops._p(m)                 # (an absent branch has no table: NULL, never dereferenced)
        d_rows = d_rows or (None, None, None)
        args = (_lib.ptr(ws['counters']), _lib.ptr(ws['geom']), _lib.ptr(d_tiled), P_, Hf, Wf, b['H'], b['W'],
                last['levels_struct'], _lib.ptr(bounds), _lib.ptr(vox_min), vox_sh, last['cap'], p(d_planes_f), p(d_feat_f),
                p(d_rows[0]), p(d_rows[1]), p(d_rows[2]), ops._p(d_bias), _lib.ptr(scratch), words.value)
        if sum(on) == 3:
            _lib.call('sherf_gather_tokens_bwd_binned', *args, _lib.stream())
        else:                                                          # the taps of the absent branches left out of the kernel
            _lib.call('sherf_gather_tokens_bwd_masked', *args, _lib.branch_mask(on), _lib.stream())

    ctx = dict(n=n, P=P_, Hf=Hf, Wf=Wf, planes=Mat(planes.view(-1), 96, P_ * P_), obs_feat=Mat(obs_feat.view(-1), 64, Hf * Wf),
               levels=levels_ctx, scatter=scatter)
    taps = taps_backward(ops, state, ctx, d_tin, dWb_pe, on)
    grads.update(taps['grads'])
    grad_in = lambda m, *shape: None if m is None else m.tensor().view(*shape).clone()
    d_planes, d_obs = grad_in(taps['d_planes'], 1, 3, 32, P_, P_), grad_in(taps['d_obs_feat'], 1, 64, Hf, Wf)
    if not on[2]:                                                           # no voxel taps: nothing reaches the sparse encoder (renderer.py:345-352)
        return dict(params=grads, planes=d_planes, obs_feat=d_obs, vertex_feat=None)
    # ---- a11 ----
    lev_ctx = [dict(keys=L[i]['keys'], wp=L[i]['wp'], n_rows=L[i]['n_rows'], dims=tuple(shapes[i]), cap=L[i]['cap']) for i in range(4)]
    layers = [dict(wname='renderer.encoder_3d.' + m['wname'], bname='renderer.encoder_3d.' + m['bname'], cin=m['cin'], cout=m['cout'],
                   down=m['down'], tap=m['tap'], lev_in=m['lev_in'], lev_out=m['lev'], raw=Mat.of(m['out']),
                   bnparam=Mat(m['bnp'].view(-1), 1, 3 * m['cout']), stats=Mat(pl['stats_flat'], 1, 2 * m['cout'], off=m['stats_off']))
              for m in meta]
    N = b['coord'].shape[0]
    ectx = dict(levels=lev_ctx, mult=L[0]['mult'], n_total=L[0]['n_total'], coord=b['coord'], N=N, g0=Mat.of(L[0]['g0']), layers=layers)
    d_feat, g_enc = encoder_backward(ops, state, ectx, taps['d_levels'])
    grads.update(g_enc)
    return dict(params=grads, planes=d_planes, obs_feat=d_obs, vertex_feat=d_feat.tensor().clone())


class RenderFunction(torch.autograd.Function):
    """autograd node around ImportanceRenderer.forward: (planes, obs_input_feature, sparse-voxel features, *parameters) ->
    (rgb, depth, acc).  Opt-in per renderer (`renderer.enable_autograd = True`; `sherf_amd.install()` sets it for the class; a renderer built with
    use_NeRF_decoder=False also needs `renderer.enable_osg_autograd = True`: staged).
    The depth output carries no gradient (as in the reference's losses, loss.py:103-176)."""

    @staticmethod
    def forward(ctx, renderer, decoder, call, planes, obs_feat, vox_feat, *params):
        with torch.no_grad():
            rgb, depth, acc = call()
        ctx.renderer, ctx.decoder = renderer, decoder
        ctx.names = [n for n, _ in _named_params(renderer, decoder)]
        # the backward reads the frame's compact samples, taps and encoder activations from the renderer's WORKSPACE (renderer.last), which
        # the next forward of the same renderer on the same stream overwrites: the node remembers WHICH frame it recorded
        ctx.frame = renderer.last
        ctx.mark_non_differentiable(depth)
        return rgb, depth, acc

    @staticmethod
    def backward(ctx, d_rgb, d_depth, d_acc):
        if ctx.renderer.last is not ctx.frame:
            raise RuntimeError('sherf_amd: backward of a frame whose workspace has been overwritten -- the same ImportanceRenderer rendered another '
                               'frame between this forward and its backward (gradient accumulation over several forwards, a second generator pass, '
                               'a grad-enabled forward in between).  Run every backward before the next forward of the same renderer, as the '
                               'reference loop does (training_loop.py:354-386), or use one renderer per frame in flight.')
        out = render_backward(ctx.renderer, ctx.decoder, d_rgb, d_acc)
        grads = []
        for name, p in _named_params(ctx.renderer, ctx.decoder):
            g = out['params'].get(name)
            grads.append(None if g is None else g.view(p.shape).to(p.dtype))
        return (None, None, None, out['planes'], out['obs_feat'], out['vertex_feat'], *grads)


def _named_params(renderer, decoder):
    return [('renderer.' + n, p) for n, p in renderer.named_parameters()] + [('decoder.' + n, p) for n, p in decoder.named_parameters()]
