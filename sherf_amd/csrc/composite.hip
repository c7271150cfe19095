// Alpha compositing (gfx950): rows a15 + a16 of SURVEY.md section 8.
//
// MipRayMarcher2.run_forward (ray_marcher.py:25-64, clamp_mode 'relu'):
//   delta_k = (t_{k+1}-t_k)*|d|, last = 1e10*|d|;  alpha = 1-exp(-relu(sigma)*delta);
//   T_k = prod_{i<k} (1-alpha_i+1e-10);  w = alpha*T;  rgb = sum w c;  depth = sum w t / sum w -> nan->inf
//   -> clamp to the GLOBAL [min t, max t];  (+1-acc if white_back);  rgb*2-1.
// Samples the shell mask rejected carry (rgb 0, sigma -80) in the reference (renderer.py:364-368): relu makes
// alpha exactly 0, the transmittance factor is fl(1+1e-10) == 1 and the weight is 0, so skipping them is exact.
// The compact kernel therefore walks only a ray's valid samples (ascending k): HBM-bound, 20 B/ray out.
//
// clamp_mode 'softplus' (ray_marcher.py:37-38): the density is softplus(sigma - 1) as F.softplus evaluates it in fp32 (beta 1, threshold 20):
//   x = sigma - 1;  s = x > 20 ? x : log1pf(expf(x));  ds/dsigma = x > 20 ? 1 : z / (z + 1), z = expf(x)  (autograd's softplus backward;
//   no sigma > 0 mask: every valid sample receives a density gradient).
// Skipping the rejected samples stays exact: softplus(-80 - 1) ~ 6.6e-36; times the largest delta (1e10 |d|) that is ~1e-25 |d|, expf of its
// negative rounds to 1 for every |d| < ~1e17, so alpha is exactly 0, the transmittance factor is fl(1 + 1e-10) == 1 and the weight is 0 -- the
// same three facts as under relu (tests/test_gpu_softplus.py compares the dense and the compact kernel bit for bit on a scattered frame).
// The mode travels in bit 1 of the `white_back` argument of every entry point (bit 0: white background; include/sherf_hip.h,
// SHERF_COMPOSITE_*); each kernel is a template on it, and the relu instantiations are the code these kernels were before.
#include "common.h"

namespace {

// (density<MODE>, density_grad<MODE>, depth_at and the CLAMP_* modes: csrc/passes.h, shared with the sampler and the importance depths)
template <int BATCH, int MODE>
__global__ void __launch_bounds__(256) composite_compact_kernel(const int32_t* __restrict__ counters,
                                                                const int32_t* __restrict__ ray_base,
                                                                const int32_t* __restrict__ ray_cnt,
                                                                const int32_t* __restrict__ cs_idx,
                                                                const float4* __restrict__ sample_out,
                                                                const float* __restrict__ ray_d, const float* __restrict__ near,
                                                                const float* __restrict__ far, int R, int S, int white_back,
                                                                int64_t tok_cap, int32_t* __restrict__ flags,
                                                                float* __restrict__ rgb, float* __restrict__ depth,
                                                                float* __restrict__ acc) {
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r >= R) return;
    if ((int64_t)ray_base[r] + ray_cnt[r] > tok_cap) {
        // the frame holds more valid samples than the token-side buffers (sherf_frame.tok_capacity): this ray's samples were not
        // evaluated.  Loud, not wrong: NaN pixels + counters[3] bit 1; the caller re-sizes from counters[0] and renders again.
        const float qnan = __int_as_float(0x7fc00000);
        rgb[r * 3] = rgb[r * 3 + 1] = rgb[r * 3 + 2] = qnan; depth[r] = qnan; acc[r] = qnan;
        if (flags) atomicOr(flags, 2);
        return;
    }
    const float dmin = ord2f(counters[1]), dmax = ord2f(counters[2]);
    const float d0 = ray_d[r * 3], d1 = ray_d[r * 3 + 1], d2 = ray_d[r * 3 + 2];
    const float dn = sqrtf(d0 * d0 + d1 * d1 + d2 * d2);
    const float nr = near[r], range = __fsub_rn(far[r], nr);
    const int base = ray_base[r], cnt = ray_cnt[r];
    float T = 1.f, cr = 0.f, cg = 0.f, cb = 0.f, wsum = 0.f, dsum = 0.f;
    // A ray's samples in batches of BATCH = 4 (1: round 5's loop, SHERF_EXPERIMENT bit 20): the eight loads of a batch are requested together, then its samples enter the running products in order (the same arithmetic in the
    // same order).  One sample per trip made a wave wait for memory once per sample of its longest ray -- up to 64 dependent round trips at the tail of every frame.
    for (int i0 = 0; i0 < cnt; i0 += BATCH) {
        int kk[BATCH];
        float4 oo[BATCH];
#pragma unroll
        for (int j = 0; j < BATCH; ++j) {
            const int i = min(i0 + j, cnt - 1);
            kk[j] = cs_idx[base + i] - r * S;
            oo[j] = sample_out[base + i];
        }
#pragma unroll
        for (int j = 0; j < BATCH; ++j) {
            if (i0 + j >= cnt) break;
            const int k = kk[j];
            const float4 o = oo[j];
            const float t = depth_at(nr, range, k, S);
            const float delta = (k == S - 1 ? 1e10f : depth_at(nr, range, k + 1, S) - t) * dn;
            const float alpha = 1.f - expf(-(density<MODE>(o.w) * delta));
            const float w = alpha * T;
            T = T * (1.f - alpha + 1e-10f);
            cr += w * o.x; cg += w * o.y; cb += w * o.z; wsum += w; dsum += w * t;
        }
    }
    float dep = dsum / wsum;                                   // 0/0 -> NaN for empty rays
    if (dep != dep) dep = __int_as_float(0x7f800000);          // nan_to_num(.., inf)
    dep = fminf(fmaxf(dep, dmin), dmax);
    if (white_back) { cr += 1.f - wsum; cg += 1.f - wsum; cb += 1.f - wsum; }
    rgb[r * 3] = cr * 2.f - 1.f; rgb[r * 3 + 1] = cg * 2.f - 1.f; rgb[r * 3 + 2] = cb * 2.f - 1.f;
    depth[r] = dep;
    acc[r] = wsum;
}

template <int MODE>
__global__ void __launch_bounds__(256) composite_dense_kernel(const float* __restrict__ colors, const float* __restrict__ sigma,
                                                              const float* __restrict__ depths, const float* __restrict__ rays_d,
                                                              int R, int S, int white_back, const float* __restrict__ dminmax,
                                                              float* __restrict__ rgb, float* __restrict__ depth,
                                                              float* __restrict__ weights) {
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r >= R) return;
    const float dmin = dminmax[0], dmax = dminmax[1];
    const float d0 = rays_d[r * 3], d1 = rays_d[r * 3 + 1], d2 = rays_d[r * 3 + 2];
    const float dn = sqrtf(d0 * d0 + d1 * d1 + d2 * d2);
    const float* c = colors + (size_t)r * S * 3;
    const float* sg = sigma + (size_t)r * S;
    const float* tt = depths + (size_t)r * S;
    float T = 1.f, cr = 0.f, cg = 0.f, cb = 0.f, wsum = 0.f, dsum = 0.f;
    for (int k = 0; k < S; ++k) {
        const float t = tt[k];
        const float delta = (k == S - 1 ? 1e10f : tt[k + 1] - t) * dn;
        const float alpha = 1.f - expf(-(density<MODE>(sg[k]) * delta));
        const float w = alpha * T;
        T = T * (1.f - alpha + 1e-10f);
        weights[(size_t)r * S + k] = w;
        cr += w * c[k * 3]; cg += w * c[k * 3 + 1]; cb += w * c[k * 3 + 2]; wsum += w; dsum += w * t;
    }
    float dep = dsum / wsum;
    if (dep != dep) dep = __int_as_float(0x7f800000);
    dep = fminf(fmaxf(dep, dmin), dmax);
    if (white_back) { cr += 1.f - wsum; cg += 1.f - wsum; cb += 1.f - wsum; }
    rgb[r * 3] = cr * 2.f - 1.f; rgb[r * 3 + 1] = cg * 2.f - 1.f; rgb[r * 3 + 2] = cb * 2.f - 1.f;
    depth[r] = dep;
}

// Backward of composite_compact_kernel w.r.t. the per-sample (rgb, sigma), for a loss that reads rgb_final and acc
// (the reference's losses never read the depth map: loss.py:103-176).  With g_c = 2 dL/drgb_final and
//   g_w[k] = g_c . c_k + dL/dacc - white_back * sum(g_c):
//   dL/dc_k     = g_c w_k
//   dL/dalpha_k = g_w[k] T_k - (sum_{m>k} g_w[m] w_m) / (1 - alpha_k + 1e-10)        (T_m carries the factor of sample k)
//               = T_k (g_w[k] - Q_k),   Q_k = sum_{m>k} g_w[m] alpha_m prod_{k<j<m} f_j,   f_j = 1 - alpha_j + 1e-10
//   dL/dsigma_k = dL/dalpha_k * delta_k * exp(-s_k delta_k) * ds_k/dsigma_k,   s = relu(sigma): [sigma_k > 0];  s = softplus(sigma - 1): z / (z + 1)
// Two sweeps over the ray's compact samples.  The first runs BACKWARDS and builds Q by its recurrence Q_{k-1} = g_w[k] alpha_k + f_k Q_k (Q behind
// the last sample is 0), leaving Q_k in the .w of the sample's output row; the second runs forwards, rebuilds T, alpha, w and overwrites the row.
// (Until the per-ray edge tests, the suffix sum was `total - prefix` of two forward sweeps, divided by f_k: behind an exactly opaque sample both are
// O(1) while the suffix is O(1e-10), so the difference was rounding noise, 1e-10 of it a division by 1e-10 later -- gradients of the samples behind
// the opaque one wrong by several times their size.  Q needs no difference and no division.)  Same thread-per-ray shape as the forward.
template <int MODE>
__global__ void __launch_bounds__(256) composite_compact_bwd_kernel(const int32_t* __restrict__ ray_base, const int32_t* __restrict__ ray_cnt,
                                                                    const int32_t* __restrict__ cs_idx, const float4* __restrict__ sample_out,
                                                                    const float* __restrict__ ray_d, const float* __restrict__ near,
                                                                    const float* __restrict__ far, int R, int S, int white_back,
                                                                    const float* __restrict__ d_rgb, const float* __restrict__ d_acc,
                                                                    float4* __restrict__ d_sample_out) {
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r >= R) return;
    const float d0 = ray_d[r * 3], d1 = ray_d[r * 3 + 1], d2 = ray_d[r * 3 + 2];
    const float dn = sqrtf(d0 * d0 + d1 * d1 + d2 * d2);
    const float nr = near[r], range = __fsub_rn(far[r], nr);
    const int base = ray_base[r], cnt = ray_cnt[r];
    const float gx = 2.f * d_rgb[r * 3], gy = 2.f * d_rgb[r * 3 + 1], gz = 2.f * d_rgb[r * 3 + 2];
    const float gconst = d_acc[r] - (white_back ? gx + gy + gz : 0.f);
    float Q = 0.f;
    for (int i = cnt - 1; i >= 0; --i) {
        const int k = cs_idx[base + i] - r * S;
        const float4 o = sample_out[base + i];
        const float t = depth_at(nr, range, k, S);
        const float delta = (k == S - 1 ? 1e10f : depth_at(nr, range, k + 1, S) - t) * dn;
        const float alpha = 1.f - expf(-(density<MODE>(o.w) * delta));
        d_sample_out[base + i].w = Q;
        Q = (gx * o.x + gy * o.y + gz * o.z + gconst) * alpha + (1.f - alpha + 1e-10f) * Q;
    }
    float T = 1.f;
    for (int i = 0; i < cnt; ++i) {
        const int k = cs_idx[base + i] - r * S;
        const float4 o = sample_out[base + i];
        const float t = depth_at(nr, range, k, S);
        const float delta = (k == S - 1 ? 1e10f : depth_at(nr, range, k + 1, S) - t) * dn;
        const float e = expf(-(density<MODE>(o.w) * delta));
        const float alpha = 1.f - e, w = alpha * T;
        const float gw = gx * o.x + gy * o.y + gz * o.z + gconst;
        const float dalpha = T * (gw - d_sample_out[base + i].w);
        const float dsigma = MODE == CLAMP_RELU ? (o.w > 0.f ? dalpha * delta * e : 0.f) : dalpha * delta * e * density_grad<MODE>(o.w);
        d_sample_out[base + i] = make_float4(gx * w, gy * w, gz * w, dsigma);
        T = T * (1.f - alpha + 1e-10f);
    }
}

// Backward of composite_dense_kernel (MipRayMarcher2 on dense inputs, all three outputs) w.r.t. colors and sigma.  With g_c = 2 dL/drgb,
// W = sum w, D = sum w t, depth = D / W and g_d = dL/ddepth where the depth is the quotient itself, 0 where it was replaced (empty ray: 0 / 0 ->
// nan_to_num) or moved by the global clamp (autograd passes no gradient through either; its quotient then turns that zero into 0 / 0 = NaN on an
// empty ray -- here the ray's depth term is dropped):
//   g_w[k]      = g_c . c_k - white_back * sum(g_c) + dL/dw_k + (g_d / W) (t_k - depth)
//   dL/dc_k     = g_c w_k
//   dL/dalpha_k = g_w[k] T_k - (sum_{m>k} g_w[m] w_m) / (1 - alpha_k + 1e-10) = T_k (g_w[k] - Q_k)                (Q: see the compact backward)
//   dL/dsigma_k = dL/dalpha_k * delta_k * exp(-s_k delta_k) * ds_k/dsigma_k
// Three sweeps, one thread per ray: forwards for W and D (the depth and whether it is live), backwards for Q (left in d_sigma[k]), forwards again to
// rebuild T, alpha, w and write the gradients.  No suffix is taken as a difference of totals.
// A null upstream gradient is zero.  No gradient w.r.t. depths / rays_d.
template <int MODE>
__global__ void __launch_bounds__(256) composite_dense_bwd_kernel(const float* __restrict__ colors, const float* __restrict__ sigma,
                                                                  const float* __restrict__ depths, const float* __restrict__ rays_d,
                                                                  int R, int S, int white_back, const float* __restrict__ dminmax,
                                                                  const float* __restrict__ d_rgb, const float* __restrict__ d_depth,
                                                                  const float* __restrict__ d_weights, float* __restrict__ d_colors,
                                                                  float* __restrict__ d_sigma) {
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r >= R) return;
    const float dmin = dminmax[0], dmax = dminmax[1];
    const float d0 = rays_d[r * 3], d1 = rays_d[r * 3 + 1], d2 = rays_d[r * 3 + 2];
    const float dn = sqrtf(d0 * d0 + d1 * d1 + d2 * d2);
    const float* c = colors + (size_t)r * S * 3;
    const float* sg = sigma + (size_t)r * S;
    const float* tt = depths + (size_t)r * S;
    const float* dw = d_weights ? d_weights + (size_t)r * S : nullptr;
    float* dc = d_colors + (size_t)r * S * 3;
    float* ds = d_sigma + (size_t)r * S;
    const float gx = d_rgb ? 2.f * d_rgb[r * 3] : 0.f, gy = d_rgb ? 2.f * d_rgb[r * 3 + 1] : 0.f, gz = d_rgb ? 2.f * d_rgb[r * 3 + 2] : 0.f;
    const float gconst = white_back ? -(gx + gy + gz) : 0.f;
    float T = 1.f, wsum = 0.f, dsum = 0.f;
    for (int k = 0; k < S; ++k) {
        const float t = tt[k];
        const float delta = (k == S - 1 ? 1e10f : tt[k + 1] - t) * dn;
        const float alpha = 1.f - expf(-(density<MODE>(sg[k]) * delta));
        const float w = alpha * T;
        T = T * (1.f - alpha + 1e-10f);
        wsum += w; dsum += w * t;
    }
    const float dep = dsum / wsum;
    const bool live = d_depth && dep == dep && dep >= dmin && dep <= dmax;
    const float gdw = live ? d_depth[r] / wsum : 0.f;
    float Q = 0.f;
    for (int k = S - 1; k >= 0; --k) {
        const float t = tt[k];
        const float delta = (k == S - 1 ? 1e10f : tt[k + 1] - t) * dn;
        const float alpha = 1.f - expf(-(density<MODE>(sg[k]) * delta));
        const float base = gx * c[k * 3] + gy * c[k * 3 + 1] + gz * c[k * 3 + 2] + gconst + (dw ? dw[k] : 0.f);
        const float gw = live ? base + gdw * (t - dep) : base;
        ds[k] = Q;
        Q = gw * alpha + (1.f - alpha + 1e-10f) * Q;
    }
    T = 1.f;
    for (int k = 0; k < S; ++k) {
        const float t = tt[k];
        const float delta = (k == S - 1 ? 1e10f : tt[k + 1] - t) * dn;
        const float e = expf(-(density<MODE>(sg[k]) * delta));
        const float alpha = 1.f - e, w = alpha * T;
        const float base = gx * c[k * 3] + gy * c[k * 3 + 1] + gz * c[k * 3 + 2] + gconst + (dw ? dw[k] : 0.f);
        const float gw = live ? base + gdw * (t - dep) : base;
        const float dalpha = T * (gw - ds[k]);
        const float dg = density_grad<MODE>(sg[k]);
        ds[k] = dg == 0.f ? 0.f : dalpha * delta * e * dg;          // (relu: the sigma > 0 mask, as a select -- not 0 * a product that may overflow)
        dc[k * 3] = gx * w; dc[k * 3 + 1] = gy * w; dc[k * 3 + 2] = gz * w;
        T = T * (1.f - alpha + 1e-10f);
    }
}

// Compositing over TWO sample lists merged by depth (importance sampling: unify_samples + MipRayMarcher2, renderer.py:389-393, 446-456): a ray's S analytic
// coarse depths and the N ascending depths of depths_fine[r], walked in merged order -- a coarse sample before a fine one of the same depth, fine samples in
// their stored order (the stable order of the concatenation [coarse, fine]; torch.sort promises none, so the goldens hold no tie).  EVERY depth takes part in
// the deltas, whatever its mask: a valid sample's delta is the distance to the next depth of the merged list, the last of the S + N takes 1e10.  Only valid
// samples are read and enter the products -- coarse ones from the frame's compact list as in composite_compact_kernel, fine ones from the point sampler's
// rows of 64 (point r N + j; csrc/field.hip: field_scatter_kernel finds a point's compact row the same way); a rejected sample's weight is exactly 0 and its
// transmittance factor exactly 1 (file header).  Same arithmetic in the same order as composite_dense_kernel on the merged, densely scattered samples.
// A ray with no valid sample in either list skips the walk: the loop would leave every accumulator at its initial value.
// Token overflow in either list: NaN pixels + flag bit 1, as composite_compact_kernel.
template <int MODE>
__global__ void __launch_bounds__(256) composite_merged_kernel(const int32_t* __restrict__ counters, const int32_t* __restrict__ ray_base,
                                                               const int32_t* __restrict__ ray_cnt, const int32_t* __restrict__ cs_idx,
                                                               const float4* __restrict__ sample_out, int64_t tok_cap,
                                                               const float* __restrict__ depths_fine, const uint64_t* __restrict__ fine_mask,
                                                               const int32_t* __restrict__ fine_base, const float4* __restrict__ fine_out,
                                                               int64_t fine_tok_cap, const float* __restrict__ ray_d, const float* __restrict__ near,
                                                               const float* __restrict__ far, int R, int S, int N, int white_back,
                                                               int32_t* __restrict__ flags, float* __restrict__ rgb, float* __restrict__ depth,
                                                               float* __restrict__ acc) {
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r >= R) return;
    const float qnan = __int_as_float(0x7fc00000);
    const int base = ray_base[r], cnt = ray_cnt[r];
    bool bad = (int64_t)base + cnt > tok_cap;
    // the ray's fine points: bits r N .. r N + N - 1 of the rows' mask words
    const int64_t p0 = (int64_t)r * N, p1 = p0 + N;
    bool any_fine = false;
    for (int64_t row = p0 >> 6; row <= (p1 - 1) >> 6; ++row) {
        uint64_t m = fine_mask[row];
        const int64_t lo = row << 6;
        if (p0 > lo) m &= ~0ull << (p0 - lo);
        if (p1 < lo + 64) m &= (1ull << (p1 - lo)) - 1ull;
        if (m) {
            any_fine = true;
            const int top = 63 - __builtin_clzll(m);                                      // the ray's last valid point of this row
            if ((int64_t)fine_base[row] + __popcll(fine_mask[row] & ((1ull << top) - 1ull)) >= fine_tok_cap) bad = true;
        }
    }
    if (bad) {
        rgb[r * 3] = rgb[r * 3 + 1] = rgb[r * 3 + 2] = qnan; depth[r] = qnan; acc[r] = qnan;
        if (flags) atomicOr(flags, 2);
        return;
    }
    const float dmin = ord2f(counters[1]), dmax = ord2f(counters[2]);
    float T = 1.f, cr = 0.f, cg = 0.f, cb = 0.f, wsum = 0.f, dsum = 0.f;
    if (cnt > 0 || any_fine) {
        const float d0 = ray_d[r * 3], d1 = ray_d[r * 3 + 1], d2 = ray_d[r * 3 + 2];
        const float dn = sqrtf(d0 * d0 + d1 * d1 + d2 * d2);
        const float nr = near[r], range = __fsub_rn(far[r], nr);
        const float* tf = depths_fine + (size_t)r * N;
        const float inf = __int_as_float(0x7f800000);
        int k = 0, j = 0, ci = 0;                                     // heads: coarse depth, fine depth, coarse compact sample
        int knext = cnt > 0 ? cs_idx[base] - r * S : -1;              // dense index of the next valid coarse sample
        int64_t row = -1;
        uint64_t word = 0;
        int rbase = 0;
        float tc = depth_at(nr, range, 0, S), tn = tf[0];
        for (int step = 0; step < S + N; ++step) {
            const bool coarse = k < S && (j >= N || tc <= tn);        // (a tie: the coarse sample first)
            const float t = coarse ? tc : tn;
            bool valid = false;
            float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
            if (coarse) {
                if (k == knext) {
                    valid = true;
                    o = sample_out[base + ci];
                    ++ci;
                    knext = ci < cnt ? cs_idx[base + ci] - r * S : -1;
                }
                ++k;
                tc = k < S ? depth_at(nr, range, k, S) : inf;
            } else {
                const int64_t p = p0 + j;
                if ((p >> 6) != row) { row = p >> 6; word = fine_mask[row]; rbase = fine_base[row]; }
                const int b = (int)(p & 63);
                if ((word >> b) & 1ull) {
                    valid = true;
                    o = fine_out[(int64_t)rbase + __popcll(word & ((1ull << b) - 1ull))];
                }
                ++j;
                tn = j < N ? tf[j] : inf;
            }
            if (!valid) continue;
            const bool last = k >= S && j >= N;
            const float tnext = (k < S && (j >= N || tc <= tn)) ? tc : tn;
            const float delta = (last ? 1e10f : tnext - t) * dn;
            const float alpha = 1.f - expf(-(density<MODE>(o.w) * delta));
            const float w = alpha * T;
            T = T * (1.f - alpha + 1e-10f);
            cr += w * o.x; cg += w * o.y; cb += w * o.z; wsum += w; dsum += w * t;
        }
    }
    float dep = dsum / wsum;                                   // 0/0 -> NaN for empty rays
    if (dep != dep) dep = __int_as_float(0x7f800000);          // nan_to_num(.., inf)
    dep = fminf(fmaxf(dep, dmin), dmax);
    if (white_back) { cr += 1.f - wsum; cg += 1.f - wsum; cb += 1.f - wsum; }
    rgb[r * 3] = cr * 2.f - 1.f; rgb[r * 3 + 1] = cg * 2.f - 1.f; rgb[r * 3 + 2] = cb * 2.f - 1.f;
    depth[r] = dep;
    acc[r] = wsum;
}

// The frame's depth range (counters[1..2], ordered ints: ray_marcher.py:57 clamps with the min / max over ALL S + N depths) widened by the fine depths: a
// ray's are ascending, so its first and last.  sherf_importance_depths keeps every fine depth inside its own ray's coarse span and this changes nothing
// then; depths from elsewhere (the unit tests put a fine sample behind the last coarse one) are folded in.  A wave reduces, lane 0 issues the two atomics.
__global__ void __launch_bounds__(256) fine_range_kernel(const float* __restrict__ depths_fine, int R, int N, int32_t* __restrict__ counters) {
    const int r = blockIdx.x * 256 + threadIdx.x;
    int lo = 0x7fffffff, hi = (int)0x80000000;
    if (r < R) { lo = f2ord(depths_fine[(size_t)r * N]); hi = f2ord(depths_fine[(size_t)r * N + N - 1]); }
    for (int m = 32; m > 0; m >>= 1) { lo = min(lo, __shfl_xor(lo, m)); hi = max(hi, __shfl_xor(hi, m)); }
    if ((threadIdx.x & 63) == 0) { atomicMin(counters + 1, lo); atomicMax(counters + 2, hi); }
}

// bit 0 of the entry points' `white_back`: white background; bit 1: clamp_mode 'softplus' (include/sherf_hip.h); anything else is refused
constexpr int kCompositeBits = SHERF_COMPOSITE_WHITE_BACK | SHERF_COMPOSITE_SOFTPLUS;

}  // namespace

extern "C" int sherf_composite_compact_cap(int32_t* counters, const int32_t* ray_base, const int32_t* ray_cnt,
                                           const int32_t* cs_idx, const float* sample_out, const float* ray_d,
                                           const float* near, const float* far, int R, int S, int white_back, int64_t tok_cap,
                                           float* rgb, float* depth, float* acc, sherf_stream_t stream) {
    SHERF_CHECK_ARG(counters && ray_base && ray_cnt && cs_idx && sample_out && ray_d && near && far && rgb && depth && acc);
    SHERF_CHECK_ARG(R > 0 && S >= 2 && tok_cap > 0);
    SHERF_CHECK_ARG((white_back & ~kCompositeBits) == 0);
    const int wb = white_back & SHERF_COMPOSITE_WHITE_BACK;
    if (white_back & SHERF_COMPOSITE_SOFTPLUS)
        hipLaunchKernelGGL((composite_compact_kernel<4, CLAMP_SOFTPLUS>), dim3(cdiv(R, 256)), dim3(256), 0, as_stream(stream), counters, ray_base,
                           ray_cnt, cs_idx, reinterpret_cast<const float4*>(sample_out), ray_d, near, far, R, S, wb, tok_cap,
                           counters + 3, rgb, depth, acc);
    else if (sherf_experiment() & (1 << 20))
        hipLaunchKernelGGL((composite_compact_kernel<1, CLAMP_RELU>), dim3(cdiv(R, 256)), dim3(256), 0, as_stream(stream), counters, ray_base,
                           ray_cnt, cs_idx, reinterpret_cast<const float4*>(sample_out), ray_d, near, far, R, S, wb, tok_cap,
                           counters + 3, rgb, depth, acc);
    else
    hipLaunchKernelGGL((composite_compact_kernel<4, CLAMP_RELU>), dim3(cdiv(R, 256)), dim3(256), 0, as_stream(stream), counters, ray_base,
                       ray_cnt, cs_idx, reinterpret_cast<const float4*>(sample_out), ray_d, near, far, R, S, wb, tok_cap,
                       counters + 3, rgb, depth, acc);
    SHERF_LAUNCH_CHECK();
}

extern "C" int sherf_composite_compact(const int32_t* counters, const int32_t* ray_base, const int32_t* ray_cnt,
                                       const int32_t* cs_idx, const float* sample_out, const float* ray_d,
                                       const float* near, const float* far, int R, int S, int white_back, float* rgb,
                                       float* depth, float* acc, sherf_stream_t stream) {
    SHERF_CHECK_ARG(counters && ray_base && ray_cnt && cs_idx && sample_out && ray_d && near && far && rgb && depth && acc);
    SHERF_CHECK_ARG(R > 0 && S >= 2);
    SHERF_CHECK_ARG((white_back & ~kCompositeBits) == 0);
    const int wb = white_back & SHERF_COMPOSITE_WHITE_BACK;
    if (white_back & SHERF_COMPOSITE_SOFTPLUS)
        hipLaunchKernelGGL((composite_compact_kernel<4, CLAMP_SOFTPLUS>), dim3(cdiv(R, 256)), dim3(256), 0, as_stream(stream), counters, ray_base,
                           ray_cnt, cs_idx, reinterpret_cast<const float4*>(sample_out), ray_d, near, far, R, S, wb,
                           (int64_t)R * S, static_cast<int32_t*>(nullptr), rgb, depth, acc);
    else
    hipLaunchKernelGGL((composite_compact_kernel<4, CLAMP_RELU>), dim3(cdiv(R, 256)), dim3(256), 0, as_stream(stream), counters, ray_base,
                       ray_cnt, cs_idx, reinterpret_cast<const float4*>(sample_out), ray_d, near, far, R, S, wb,
                       (int64_t)R * S, static_cast<int32_t*>(nullptr), rgb, depth, acc);
    SHERF_LAUNCH_CHECK();
}

extern "C" int sherf_composite_dense(const float* colors, const float* sigma, const float* depths, const float* rays_d,
                                     int R, int S, int white_back, const float* dminmax, float* rgb, float* depth,
                                     float* weights, sherf_stream_t stream) {
    SHERF_CHECK_ARG(colors && sigma && depths && rays_d && dminmax && rgb && depth && weights);
    SHERF_CHECK_ARG(R > 0 && S >= 1);
    SHERF_CHECK_ARG((white_back & ~kCompositeBits) == 0);
    const int wb = white_back & SHERF_COMPOSITE_WHITE_BACK;
    if (white_back & SHERF_COMPOSITE_SOFTPLUS)
        hipLaunchKernelGGL(composite_dense_kernel<CLAMP_SOFTPLUS>, dim3(cdiv(R, 256)), dim3(256), 0, as_stream(stream), colors, sigma, depths,
                           rays_d, R, S, wb, dminmax, rgb, depth, weights);
    else
    hipLaunchKernelGGL(composite_dense_kernel<CLAMP_RELU>, dim3(cdiv(R, 256)), dim3(256), 0, as_stream(stream), colors, sigma, depths,
                       rays_d, R, S, wb, dminmax, rgb, depth, weights);
    SHERF_LAUNCH_CHECK();
}

extern "C" int sherf_composite_dense_bwd(const float* colors, const float* sigma, const float* depths, const float* rays_d,
                                         int R, int S, int white_back, const float* dminmax, const float* d_rgb,
                                         const float* d_depth, const float* d_weights, float* d_colors, float* d_sigma,
                                         sherf_stream_t stream) {
    SHERF_CHECK_ARG(colors && sigma && depths && rays_d && dminmax && d_colors && d_sigma);
    SHERF_CHECK_ARG(R > 0 && S >= 1);
    SHERF_CHECK_ARG((white_back & ~kCompositeBits) == 0);
    const int wb = white_back & SHERF_COMPOSITE_WHITE_BACK;
    if (white_back & SHERF_COMPOSITE_SOFTPLUS)
        hipLaunchKernelGGL(composite_dense_bwd_kernel<CLAMP_SOFTPLUS>, dim3(cdiv(R, 256)), dim3(256), 0, as_stream(stream), colors, sigma,
                           depths, rays_d, R, S, wb, dminmax, d_rgb, d_depth, d_weights, d_colors, d_sigma);
    else
        hipLaunchKernelGGL(composite_dense_bwd_kernel<CLAMP_RELU>, dim3(cdiv(R, 256)), dim3(256), 0, as_stream(stream), colors, sigma,
                           depths, rays_d, R, S, wb, dminmax, d_rgb, d_depth, d_weights, d_colors, d_sigma);
    SHERF_LAUNCH_CHECK();
}

extern "C" int sherf_composite_compact_bwd(const int32_t* ray_base, const int32_t* ray_cnt, const int32_t* cs_idx,
                                           const float* sample_out, const float* ray_d, const float* near, const float* far,
                                           int R, int S, int white_back, const float* d_rgb, const float* d_acc,
                                           float* d_sample_out, sherf_stream_t stream) {
    SHERF_CHECK_ARG(ray_base && ray_cnt && cs_idx && sample_out && ray_d && near && far && d_rgb && d_acc && d_sample_out);
    SHERF_CHECK_ARG(R > 0 && S >= 2);
    SHERF_CHECK_ARG((white_back & ~kCompositeBits) == 0);
    const int wb = white_back & SHERF_COMPOSITE_WHITE_BACK;
    if (white_back & SHERF_COMPOSITE_SOFTPLUS)
        hipLaunchKernelGGL(composite_compact_bwd_kernel<CLAMP_SOFTPLUS>, dim3(cdiv(R, 256)), dim3(256), 0, as_stream(stream), ray_base, ray_cnt,
                           cs_idx, reinterpret_cast<const float4*>(sample_out), ray_d, near, far, R, S, wb, d_rgb, d_acc,
                           reinterpret_cast<float4*>(d_sample_out));
    else
    hipLaunchKernelGGL(composite_compact_bwd_kernel<CLAMP_RELU>, dim3(cdiv(R, 256)), dim3(256), 0, as_stream(stream), ray_base, ray_cnt, cs_idx,
                       reinterpret_cast<const float4*>(sample_out), ray_d, near, far, R, S, wb, d_rgb, d_acc,
                       reinterpret_cast<float4*>(d_sample_out));
    SHERF_LAUNCH_CHECK();
}

extern "C" int sherf_composite_merged(int32_t* counters, const int32_t* ray_base, const int32_t* ray_cnt, const int32_t* cs_idx,
                                      const float* sample_out, int64_t tok_cap, const float* depths_fine, const uint64_t* fine_mask,
                                      const int32_t* fine_base, const float* fine_out, int64_t fine_tok_cap, const float* ray_d,
                                      const float* near, const float* far, int R, int S, int N, int white_back, float* rgb, float* depth,
                                      float* acc, sherf_stream_t stream) {
    SHERF_CHECK_ARG(counters && ray_base && ray_cnt && cs_idx && sample_out && depths_fine && fine_mask && fine_base && fine_out);
    SHERF_CHECK_ARG(ray_d && near && far && rgb && depth && acc);
    SHERF_CHECK_ARG(R > 0 && S >= 2 && N >= 1 && tok_cap > 0 && fine_tok_cap > 0 && (int64_t)R * N < 2147483648LL && (int64_t)R * S < 2147483648LL);
    SHERF_CHECK_ARG((white_back & ~kCompositeBits) == 0);
    const int wb = white_back & SHERF_COMPOSITE_WHITE_BACK;
    hipLaunchKernelGGL(fine_range_kernel, dim3(cdiv(R, 256)), dim3(256), 0, as_stream(stream), depths_fine, R, N, counters);
    if (white_back & SHERF_COMPOSITE_SOFTPLUS)
        hipLaunchKernelGGL(composite_merged_kernel<CLAMP_SOFTPLUS>, dim3(cdiv(R, 256)), dim3(256), 0, as_stream(stream), counters, ray_base, ray_cnt,
                           cs_idx, reinterpret_cast<const float4*>(sample_out), tok_cap, depths_fine, fine_mask, fine_base,
                           reinterpret_cast<const float4*>(fine_out), fine_tok_cap, ray_d, near, far, R, S, N, wb, counters + 3, rgb, depth, acc);
    else
        hipLaunchKernelGGL(composite_merged_kernel<CLAMP_RELU>, dim3(cdiv(R, 256)), dim3(256), 0, as_stream(stream), counters, ray_base, ray_cnt,
                           cs_idx, reinterpret_cast<const float4*>(sample_out), tok_cap, depths_fine, fine_mask, fine_base,
                           reinterpret_cast<const float4*>(fine_out), fine_tok_cap, ray_d, near, far, R, S, N, wb, counters + 3, rgb, depth, acc);
    SHERF_LAUNCH_CHECK();
}
