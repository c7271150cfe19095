"""MI355X-native `MipRayMarcher2`: drop-in for
the reference's training/volumetric_rendering/ray_marcher.py:20-70 on dense inputs, both clamp modes ('relu', 'softplus'),
differentiable w.r.t. colors and densities.
(ImportanceRenderer itself composites its compacted samples with sherf_composite_compact.)"""
import torch
import torch.nn as nn

from . import _lib


def _composite_dense(c, s, t, d, dminmax, bits):
    """colors [N,S,3], sigma [N,S], depths [N,S], rays_d [N,3] (fp32, contiguous) -> rgb [N,3], depth [N], weights [N,S]."""
    N, S = s.shape
    rgb = torch.empty(N, 3, device=c.device); dep = torch.empty(N, device=c.device)
    w = torch.empty(N, S, device=c.device)
    P = _lib.ptr
    _lib.call('sherf_composite_dense', P(c), P(s), P(t), P(d), N, S, bits, P(dminmax), P(rgb), P(dep), P(w), _lib.stream())
    return rgb, dep, w


class _DenseComposite(torch.autograd.Function):
    """autograd node around sherf_composite_dense; its backward is sherf_composite_dense_bwd (csrc/composite.hip): gradients w.r.t. colors
    and densities of all three outputs.  A ray whose depth was replaced (empty ray) or clamped takes no depth gradient."""

    @staticmethod
    def forward(ctx, colors, densities, t, d, dminmax, bits):
        shp = densities.shape[:3]
        N, S = shp[0] * shp[1], shp[2]
        c = colors.detach().to(torch.float32).contiguous().view(N, S, 3)
        s = densities.detach().to(torch.float32).contiguous().view(N, S)
        rgb, dep, w = _composite_dense(c, s, t, d, dminmax, bits)
        ctx.save_for_backward(c, s, t, d, dminmax)
        ctx.bits, ctx.shapes, ctx.dtypes = bits, (colors.shape, densities.shape), (colors.dtype, densities.dtype)
        return rgb.view(shp[0], shp[1], 3), dep.view(shp[0], shp[1], 1), w.view(*shp, 1)

    @staticmethod
    def backward(ctx, d_rgb, d_depth, d_w):
        c, s, t, d, dminmax = ctx.saved_tensors
        N, S = s.shape
        f32 = lambda g: None if g is None else g.detach().to(torch.float32).contiguous()
        d_rgb, d_depth, d_w = f32(d_rgb), f32(d_depth), f32(d_w)
        d_c, d_s = torch.empty_like(c), torch.empty_like(s)
        P = _lib.ptr
        _lib.call('sherf_composite_dense_bwd', P(c), P(s), P(t), P(d), N, S, ctx.bits, P(dminmax), P(d_rgb), P(d_depth), P(d_w),
                  P(d_c), P(d_s), _lib.stream())
        return d_c.view(ctx.shapes[0]).to(ctx.dtypes[0]), d_s.view(ctx.shapes[1]).to(ctx.dtypes[1]), None, None, None, None


class MipRayMarcher2(nn.Module):
    def __init__(self):
        super().__init__()

    def run_forward(self, colors, densities, depths, rays_d, rendering_options):
        bits = _lib.composite_bits(rendering_options.get('white_back', False), rendering_options['clamp_mode'])
        if not colors.is_cuda:
            raise RuntimeError('sherf_amd.MipRayMarcher2 runs on the GPU only (no CPU fallback)')
        if colors.shape[-1] != 3:
            raise RuntimeError(f'sherf_amd.MipRayMarcher2 composites 3 colour channels (SHERF: rgb), got {colors.shape[-1]}')
        grad = torch.is_grad_enabled()
        if grad and (depths.requires_grad or rays_d.requires_grad):
            raise RuntimeError('sherf_amd.MipRayMarcher2 (dense) is differentiable w.r.t. colors and densities only: gradients w.r.t. depths / '
                               'rays_d are not implemented; detach them')
        B, R, S = densities.shape[:3]
        f32 = lambda t: t.detach().to(torch.float32).contiguous()
        t, d = f32(depths).view(B * R, S), f32(rays_d).view(B * R, 3)
        mn, mx = torch.aminmax(t)                       # global clamp range (ray_marcher.py:57)
        dminmax = torch.stack([mn, mx]).contiguous()
        if grad and (colors.requires_grad or densities.requires_grad):
            return _DenseComposite.apply(colors, densities, t, d, dminmax, bits)
        rgb, dep, w = _composite_dense(f32(colors).view(B * R, S, 3), f32(densities).view(B * R, S), t, d, dminmax, bits)
        return rgb.view(B, R, 3), dep.view(B, R, 1), w.view(B, R, S, 1)

    def forward(self, colors, densities, depths, rays_d, rendering_options):
        return self.run_forward(colors, densities, depths, rays_d, rendering_options)
