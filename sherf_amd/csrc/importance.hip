// Importance sampling (gfx950): the fine pass's depths -- ImportanceRenderer.sample_importance / sample_pdf (renderer.py:483-542) on the weights the coarse
// marcher gives (renderer.py:376 with the ray directions handed in, as :395 does).
//
// Per ray:   w_k      the coarse compositing weights: composite_compact_kernel's operations in its order over the ray's valid samples; a sample the shell
//                     mask rejected has weight exactly 0 under both clamp modes (csrc/composite.hip, file header), so the dense weight row is the compact
//                     one scattered into zeros
//            p_i      = (max(w_{i-1}, w_i) + max(w_i, w_{i+1})) / 2 + 0.01 + 1e-5,  i = 1 .. S-2       (max_pool1d(2, 1, padding 1), avg_pool1d(2, 1), + 0.01,
//                     weights[:, 1:-1], sample_pdf's + eps)
//            cdf_j    = sum_{i <= j} p_i / sum p,  cdf_0 = 0                                            (S-1 knots over the S-1 mid-point bins)
//            t(u)     searchsorted(cdf, u, right=True) -> below = max(inds - 1, 0), above = min(inds, S-2); denom = cdf[above] - cdf[below], < 1e-5 -> 1;
//                     t = bin[below] + (u - cdf[below]) / denom * (bin[above] - bin[below]),  bin_i = (z_i + z_{i+1}) / 2
//            the N results in ascending order.
// Everything behind the weights is evaluated in fp64: the reference runs these steps in fp32 and only approximates its own formulas (its cumsum carries
// ~S ulps into a quotient by a pdf of ~0.01), the tests measure both against the formulas in fp64 (tests/test_gpu_importance.py), and fp64 costs nothing
// here -- a ray is a few hundred operations.  The result is clamped to [bin_0, bin_{S-2}], which it cannot leave but for rounding (and a NaN weight): a fine
// depth therefore lies strictly inside its own ray's coarse span, so the frame's global depth range (counters[1..2]) is the coarse one.
//
// Shape: ONE WAVE PER RAY, four rays per workgroup.  A lane holds up to four weights and up to four draws (S, N <= 256); the weights, the CDF and the draws
// live in the wave's 5 KiB of LDS; the sort is a bitonic network over the LDS row.  The two inherently serial steps -- the transmittance product over the
// ray's valid samples and the running sum of the CDF -- run in lane 0 over LDS (<= 256 dependent adds); a ray without a valid coarse sample (most rays of a
// body frame) has the uniform CDF j / (S-2) and skips both.  Why not a thread per ray: its CDF would be S doubles of LDS per THREAD (2 KiB at S = 256: 80
// threads per CU) or a re-walk per draw, its sort N values of private memory, and the loads of a ray's samples would be 64 scattered rows per wave
// instruction instead of one contiguous run.  Only wave collectives the host shim has are used (LDS + __builtin_amdgcn_wave_barrier).
#include "common.h"

namespace {

// (density<MODE> / depth_at: the compositing's, csrc/passes.h)
constexpr int kMaxS = 256, kMaxN = 256;

template <int MODE>
__global__ void __launch_bounds__(256) importance_depths_kernel(const int32_t* __restrict__ ray_base, const int32_t* __restrict__ ray_cnt,
                                                                const int32_t* __restrict__ cs_idx, const float4* __restrict__ sample_out,
                                                                const float* __restrict__ ray_o, const float* __restrict__ ray_d,
                                                                const float* __restrict__ near, const float* __restrict__ far, int R, int S, int N,
                                                                int64_t tok_cap, const float* __restrict__ u, float* __restrict__ depths_fine,
                                                                float* __restrict__ points) {
    __shared__ float s_w[4][kMaxS];          // the dense weight row
    __shared__ double s_cdf[4][kMaxS];       // the S-1 knots
    __shared__ int s_k[4][kMaxS];            // the valid samples' dense indices (a row of its own: no int / double view of one row)
    __shared__ float s_t[4][kMaxN];          // the draws' depths (before that: the valid samples' alphas)
    __shared__ double s_sum[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int r = (int)blockIdx.x * 4 + wave;
    if (r >= R) return;                      // (the whole wave: nothing below is a workgroup barrier)
    float* w = s_w[wave];
    double* cdf = s_cdf[wave];
    float* ts = s_t[wave];
    int* kk = s_k[wave];
    const float nr = near[r], range = __fsub_rn(far[r], nr);
    const int base = ray_base[r];
    int cnt = ray_cnt[r];
    if ((int64_t)base + cnt > tok_cap) cnt = 0;          // not evaluated (the compositing renders this ray as NaN and raises the flag): the uniform pdf
    cnt = min(cnt, S);
    const int M = S - 2;                                  // inner weights = bins; knots 0 .. M
    if (cnt > 0) {
        const float d0 = ray_d[r * 3], d1 = ray_d[r * 3 + 1], d2 = ray_d[r * 3 + 2];
        const float dn = sqrtf(d0 * d0 + d1 * d1 + d2 * d2);
        for (int k = lane; k < S; k += 64) w[k] = 0.f;
        for (int i = lane; i < cnt; i += 64) {
            const int k = min(max(cs_idx[base + i] - r * S, 0), S - 1);
            const float4 o = sample_out[base + i];
            const float t = depth_at(nr, range, k, S);
            const float delta = (k == S - 1 ? 1e10f : depth_at(nr, range, k + 1, S) - t) * dn;
            const float alpha = 1.f - expf(-(density<MODE>(o.w) * delta));
            ts[i] = alpha;
            kk[i] = k;
        }
        __builtin_amdgcn_wave_barrier();
        if (lane == 0) {
            float T = 1.f;
            for (int i = 0; i < cnt; ++i) {
                const float alpha = ts[i];
                const float wt = alpha * T;
                T = T * (1.f - alpha + 1e-10f);
                w[kk[i]] = wt;
            }
        }
        __builtin_amdgcn_wave_barrier();
        double p[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int j = lane + 64 * q;                  // inner weight j = sample j + 1
            p[q] = 0.0;
            if (j < M) {
                const float a = w[j], b = w[j + 1], c = w[j + 2];
                p[q] = ((double)fmaxf(a, b) + (double)fmaxf(b, c)) * 0.5 + 0.01 + 1e-5;
            }
        }
#pragma unroll
        for (int q = 0; q < 4; ++q)
            if (lane + 64 * q < M) cdf[lane + 64 * q + 1] = p[q];
        __builtin_amdgcn_wave_barrier();
        if (lane == 0) {
            double s = 0.0;
            for (int j = 1; j <= M; ++j) s += cdf[j];
            s_sum[wave] = s;
        }
        __builtin_amdgcn_wave_barrier();
        const double sum = s_sum[wave];
#pragma unroll
        for (int q = 0; q < 4; ++q)
            if (lane + 64 * q < M) cdf[lane + 64 * q + 1] = p[q] / sum;
        __builtin_amdgcn_wave_barrier();
        if (lane == 0) {
            double c = 0.0;
            cdf[0] = 0.0;
            for (int j = 1; j <= M; ++j) { c += cdf[j]; cdf[j] = c; }
        }
    } else {
        for (int j = lane; j <= M; j += 64) cdf[j] = (double)j / (double)M;
    }
    __builtin_amdgcn_wave_barrier();
    const double bin_lo = ((double)depth_at(nr, range, 0, S) + (double)depth_at(nr, range, 1, S)) * 0.5;
    const double bin_hi = ((double)depth_at(nr, range, M, S) + (double)depth_at(nr, range, M + 1, S)) * 0.5;
    int P = 1;
    while (P < N) P <<= 1;
    for (int n = lane; n < P; n += 64) {
        float t = __int_as_float(0x7f800000);             // padding of the sorting network
        if (n < N) {
            const double uu = (double)u[(size_t)r * N + n];
            int lo = 0, hi = M + 1;                       // searchsorted(right=True): the number of knots <= u
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (cdf[mid] <= uu) lo = mid + 1; else hi = mid;
            }
            const int below = max(lo - 1, 0), above = min(lo, M);
            const double c0 = cdf[below], c1 = cdf[above];
            double denom = c1 - c0;
            if (denom < 1e-5) denom = 1.0;
            const double b0 = ((double)depth_at(nr, range, below, S) + (double)depth_at(nr, range, below + 1, S)) * 0.5;
            const double b1 = ((double)depth_at(nr, range, above, S) + (double)depth_at(nr, range, above + 1, S)) * 0.5;
            const double s = b0 + (uu - c0) / denom * (b1 - b0);
            t = (float)fmin(fmax(s, bin_lo), bin_hi);     // (fmax / fmin drop a NaN: the first bin)
        }
        ts[n] = t;
    }
    __builtin_amdgcn_wave_barrier();
    for (int k = 2; k <= P; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = lane; i < P; i += 64) {
                const int l = i ^ j;
                if (l > i) {
                    const float a = ts[i], b = ts[l];
                    if (((i & k) == 0) ? (a > b) : (a < b)) { ts[i] = b; ts[l] = a; }
                }
            }
            __builtin_amdgcn_wave_barrier();
        }
    const float ox = ray_o ? ray_o[r * 3] : 0.f, oy = ray_o ? ray_o[r * 3 + 1] : 0.f, oz = ray_o ? ray_o[r * 3 + 2] : 0.f;
    const float dx = ray_d[r * 3], dy = ray_d[r * 3 + 1], dz = ray_d[r * 3 + 2];
    for (int n = lane; n < N; n += 64) {
        const float t = ts[n];
        depths_fine[(size_t)r * N + n] = t;
        if (points) {                                     // renderer.py:381 == :304: o + t d, a product and a sum (csrc/sample.hip forms a frame's samples so)
            float* pt = points + ((size_t)r * N + n) * 3;
            pt[0] = __fadd_rn(ox, __fmul_rn(t, dx)); pt[1] = __fadd_rn(oy, __fmul_rn(t, dy)); pt[2] = __fadd_rn(oz, __fmul_rn(t, dz));
        }
    }
}

// The fine samples' positions from depths handed in (sherf_importance.u == NULL: the tests pin the fine pass to recorded depths): the same product and sum.
__global__ void __launch_bounds__(256) importance_points_kernel(const float* __restrict__ ray_o, const float* __restrict__ ray_d,
                                                                const float* __restrict__ depths_fine, int64_t n, int N, float* __restrict__ points) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int64_t r = i / N;
    const float t = depths_fine[i];
    points[i * 3] = __fadd_rn(ray_o[r * 3], __fmul_rn(t, ray_d[r * 3]));
    points[i * 3 + 1] = __fadd_rn(ray_o[r * 3 + 1], __fmul_rn(t, ray_d[r * 3 + 1]));
    points[i * 3 + 2] = __fadd_rn(ray_o[r * 3 + 2], __fmul_rn(t, ray_d[r * 3 + 2]));
}

}  // namespace

extern "C" int sherf_importance_points(const float* ray_o, const float* ray_d, const float* depths_fine, int R, int N, float* points, sherf_stream_t stream) {
    SHERF_CHECK_ARG(ray_o && ray_d && depths_fine && points);
    SHERF_CHECK_ARG(R > 0 && N >= 1 && N <= kMaxN && (int64_t)R * N < 2147483648LL);
    const int64_t n = (int64_t)R * N;
    hipLaunchKernelGGL(importance_points_kernel, dim3(cdiv(n, 256)), dim3(256), 0, as_stream(stream), ray_o, ray_d, depths_fine, n, N, points);
    SHERF_LAUNCH_CHECK();
}

extern "C" int sherf_importance_depths(const int32_t* ray_base, const int32_t* ray_cnt, const int32_t* cs_idx, const float* sample_out,
                                       const float* ray_o, const float* ray_d, const float* near, const float* far, int R, int S,
                                       int white_back, int64_t tok_cap, const float* u, int N, float* depths_fine, float* points,
                                       sherf_stream_t stream) {
    SHERF_CHECK_ARG(ray_base && ray_cnt && cs_idx && sample_out && ray_d && near && far && u && depths_fine);
    SHERF_CHECK_ARG((points == nullptr) == (ray_o == nullptr));
    SHERF_CHECK_ARG(R > 0 && S >= 3 && S <= kMaxS && N >= 1 && N <= kMaxN && tok_cap > 0);
    SHERF_CHECK_ARG((int64_t)R * N < 2147483648LL && (int64_t)R * S < 2147483648LL);
    SHERF_CHECK_ARG((white_back & ~(SHERF_COMPOSITE_WHITE_BACK | SHERF_COMPOSITE_SOFTPLUS)) == 0);
    if (white_back & SHERF_COMPOSITE_SOFTPLUS)
        hipLaunchKernelGGL(importance_depths_kernel<CLAMP_SOFTPLUS>, dim3(cdiv(R, 4)), dim3(256), 0, as_stream(stream), ray_base, ray_cnt, cs_idx,
                           reinterpret_cast<const float4*>(sample_out), ray_o, ray_d, near, far, R, S, N, tok_cap, u, depths_fine, points);
    else
        hipLaunchKernelGGL(importance_depths_kernel<CLAMP_RELU>, dim3(cdiv(R, 4)), dim3(256), 0, as_stream(stream), ray_base, ray_cnt, cs_idx,
                           reinterpret_cast<const float4*>(sample_out), ray_o, ray_d, near, far, R, S, N, tok_cap, u, depths_fine, points);
    SHERF_LAUNCH_CHECK();
}
