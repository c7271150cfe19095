// Per-sample network of the OSGDecoder path (use_NeRF_decoder = False; gfx950, fp32 VALU, no MFMA):
//
//   slot-2 token += W_b . PE5(rgb)[:32]                          (rest of conv1d_reprojection, renderer.py:423-424)
//   3-token pre-norm transformer, dim 32, 3 heads x 16            (renderer.py:949-993; only when the renderer has one)
//   OSGDecoder: mean over the 3 tokens -> FC 32 -> 64, softplus -> FC 64 -> 4; sigma = y0, rgb = sigmoid(y1..3) * 1.002 - 0.001
//                                                                 (triplane.py:242-265)
//
// Same inputs and outputs as the NeRF network kernel (csrc/mlp.hip): the gather's tile-major tokens / extras and counters[0] in, sample_out rows
// (r, g, b, sigma) out.  The head does ~4.6 kFLOP per sample against the NeRF decoder's 429 kFLOP: without the transformer this is a streaming
// kernel over the tokens (~430 B per sample).
//
// Layout: FOUR LANES PER SAMPLE (a quad; 16 samples per wave, 256 per 4-wave workgroup in four trips).  Lanes 0-2 of a quad hold one token each
// (32 registers), lane 3 holds a zero token, so that
//   - LayerNorm and every projection of the transformer are lane-local; their weights are the same for every lane and are read through
//     wave-uniform (scalar) loads straight from the weight block -- the transformer's 33 KiB never touch LDS;
//   - the 3 x 3 attention takes each key / value component from the quad's three token lanes with __shfl;
//   - the mean over the tokens is a sum over the quad (lane 3 adds zero);
//   - PE5(rgb) is split over the quad: lane L evaluates the sin / cos of angles L, L + 4, L + 8, L + 12 of the 15, multiplies them by ITS columns of
//     W_b and the quad sums the four partial products (the NeRF kernel skips this step without a transformer because its decoder never reads
//     token 2; the mean here reads all three tokens, so the step always runs);
//   - the head's 64 hidden units are split over the quad, 16 each, and the four partial outputs summed.
// What depends on the lane within the quad (the W_b columns, the head) is read from LDS, laid out by the host packer so that the four lanes of a
// quad read four consecutive 16-byte words (conflict-free ds_read_b128, identical addresses across quads broadcast): 14 KiB per workgroup.
// Transcendentals are libm's (sincosf, expf, erff, log1pf), not the hardware approximations of csrc/mlp.hip: the results are fp32-grade
// (tests/test_hipcpu_osg.py bounds them by the distance of an fp32 torch evaluation from the float64 one).
#include "common.h"

#include <math.h>

namespace {

// ---- the weight block (include/sherf_hip.h: sherf_osg_decoder), offsets in floats ----
constexpr int OSG_WBP = 0;                  // [9 slots][8][4 lanes][4]: W_b columns of the lane's PE features, zero where a slot has none
constexpr int OSG_H0 = 1152;                // [16][8][4 lanes][4]: net.0.weight * gain, unit 16 L + i
constexpr int OSG_HB0 = 3200;               // [16][4 lanes]
constexpr int OSG_H1 = 3264;                // [16][4 lanes][4 outputs]: net.2.weight * gain
constexpr int OSG_HB1 = 3520;               // [4]
constexpr int OSG_HEAD_FLOATS = 3524;       // what a workgroup keeps in LDS
constexpr int T_LN1G = 0, T_LN1B = 32, T_QKV = 64, T_OUT = 4672, T_BOUT = 6208, T_LN2G = 6240, T_LN2B = 6272, T_W1 = 6304, T_B1 = 7328, T_W2 = 7360,
              T_B2 = 8384;                  // the transformer's parameters behind the head (8416 floats)

constexpr int OSG_THREADS = 256, OSG_TRIPS = 4, OSG_BLOCK_SAMPLES = OSG_THREADS / 4 * OSG_TRIPS;

__device__ __forceinline__ float quad_sum(float v) {
    v += __shfl_xor(v, 1);
    return v + __shfl_xor(v, 2);
}

// nn.LayerNorm(32), eps 1e-5 (renderer.py:931): two passes, lane-local
__device__ __forceinline__ void layer_norm32(const float (&x)[32], const float* __restrict__ g, const float* __restrict__ b, float (&y)[32]) {
    float s = 0.f;
#pragma unroll
    for (int k = 0; k < 32; ++k) s += x[k];
    const float mean = s * (1.0f / 32.0f);
    float q = 0.f;
#pragma unroll
    for (int k = 0; k < 32; ++k) { const float d = x[k] - mean; q += d * d; }
    const float inv = 1.0f / sqrtf(q * (1.0f / 32.0f) + 1e-5f);
#pragma unroll
    for (int k = 0; k < 32; ++k) y[k] = (x[k] - mean) * inv * g[k] + b[k];
}

__device__ __forceinline__ float dot32(const float* __restrict__ w, const float (&x)[32]) {
    float a = 0.f;
#pragma unroll
    for (int k = 0; k < 32; ++k) a += w[k] * x[k];
    return a;
}

// the 3-token transformer on the quad's tokens: x = this lane's token in, the layer's output token out.  `tw`: wave-uniform
__device__ __forceinline__ void transformer_quad(const float* __restrict__ tw, int qb, float (&x)[32]) {
    float y[32];
    {
        float ln[32];
        layer_norm32(x, tw + T_LN1G, tw + T_LN1B, ln);
#pragma unroll
        for (int o = 0; o < 32; ++o) y[o] = x[o] + tw[T_BOUT + o];                  // residual + to_out's bias (renderer.py:925, 962)
#pragma unroll
        for (int h = 0; h < 3; ++h) {
            float d0 = 0.f, d1 = 0.f, d2 = 0.f;                                     // this token's query against the three keys
#pragma unroll 2
            for (int d = 0; d < 16; ++d) {
                const float* wq = tw + T_QKV + (h * 16 + d) * 32;
                const float qd = dot32(wq, ln), kd = dot32(wq + 48 * 32, ln);
                d0 += qd * __shfl(kd, qb); d1 += qd * __shfl(kd, qb + 1); d2 += qd * __shfl(kd, qb + 2);
            }
            d0 *= 0.25f; d1 *= 0.25f; d2 *= 0.25f;                                  // dim_head ** -0.5 (renderer.py:956, 971)
            const float m = fmaxf(d0, fmaxf(d1, d2));
            const float e0 = expf(d0 - m), e1 = expf(d1 - m), e2 = expf(d2 - m);
            const float inv = 1.0f / (e0 + e1 + e2);
            const float p0 = e0 * inv, p1 = e1 * inv, p2 = e2 * inv;
#pragma unroll 2
            for (int d = 0; d < 16; ++d) {
                const float vd = dot32(tw + T_QKV + (96 + h * 16 + d) * 32, ln);
                const float od = p0 * __shfl(vd, qb) + p1 * __shfl(vd, qb + 1) + p2 * __shfl(vd, qb + 2);
                const float* wo = tw + T_OUT + (h * 16 + d) * 32;                   // column h * 16 + d of to_out (stored transposed)
#pragma unroll
                for (int o = 0; o < 32; ++o) y[o] += wo[o] * od;
            }
        }
    }
    float l2[32];
    layer_norm32(y, tw + T_LN2G, tw + T_LN2B, l2);
#pragma unroll
    for (int o = 0; o < 32; ++o) x[o] = y[o] + tw[T_B2 + o];
#pragma unroll 2
    for (int i = 0; i < 32; ++i) {
        const float a = tw[T_B1 + i] + dot32(tw + T_W1 + i * 32, l2);
        const float g = 0.5f * a * (1.0f + erff(a * 0.70710678118654752f));         // nn.GELU() (renderer.py:941)
        const float* w2 = tw + T_W2 + i * 32;                                       // column i of the second layer (stored transposed)
#pragma unroll
        for (int o = 0; o < 32; ++o) x[o] += w2[o] * g;
    }
}

template <bool TRANS>
__global__ void __launch_bounds__(OSG_THREADS) osg_decoder_kernel(const int32_t* __restrict__ counters, const float4* __restrict__ tokens,
                                                                  const float* __restrict__ extras, const float* __restrict__ weights,
                                                                  int64_t capacity, float4* __restrict__ out) {
    __shared__ __attribute__((aligned(16))) float lds[OSG_HEAD_FLOATS];
    const int64_t nv = min((int64_t)counters[0], capacity);
    const int64_t base = (int64_t)blockIdx.x * OSG_BLOCK_SAMPLES;
    if (base >= nv) return;                                                          // (the whole workgroup: nothing staged, nothing written)
    for (int i = threadIdx.x; i < OSG_HEAD_FLOATS / 4; i += OSG_THREADS)
        reinterpret_cast<float4*>(lds)[i] = reinterpret_cast<const float4*>(weights)[i];
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, L = lane & 3, qb = lane & ~3;
    const float4* wb4 = reinterpret_cast<const float4*>(lds + OSG_WBP);
    const float4* h04 = reinterpret_cast<const float4*>(lds + OSG_H0);
    const float4* h14 = reinterpret_cast<const float4*>(lds + OSG_H1);
    for (int trip = 0; trip < OSG_TRIPS; ++trip) {
        const int64_t c0 = base + (trip * (OSG_THREADS / 64) + wave) * 16;
        if (c0 >= nv) break;                                                         // (wave-uniform)
        const int64_t c = c0 + (lane >> 2);
        const bool live = c < nv;
        const int64_t cc = live ? c : c0;                                            // lanes past the count redo the wave's first sample and store nothing
        const int64_t tile = cc >> 5;
        const int j = (int)(cc & 31);
        // ---- this lane's token (lane 3: zeros) ----
        float x[32];
        {
            const float4* tp = tokens + ((tile * 3 + (L < 3 ? L : 0)) * 8) * 32 + j;
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                const float4 v = tp[q * 32];
                x[4 * q] = v.x; x[4 * q + 1] = v.y; x[4 * q + 2] = v.z; x[4 * q + 3] = v.w;
            }
            if (L == 3) {
#pragma unroll
                for (int k = 0; k < 32; ++k) x[k] = 0.f;
            }
        }
        // ---- slot-2 completion: token 2 += W_b . PE5(rgb)[:32].  PE5 = [rgb, sin(2^q rgb), cos(2^q rgb), q = 0..4] (renderer.py:875-916), angle
        //      n = 3 q + a: sin at feature 3 + 6 q + a, cos at 6 + 6 q + a.  Lane L: angles L + 4 m (slots 2 m, 2 m + 1) and the raw colour L (slot 8);
        //      a slot whose feature does not exist or lies beyond the 32 kept has zero weights ----
        {
            const float* ex = extras + tile * (12 * 32) + j;
            const float r0 = ex[6 * 32], r1 = ex[7 * 32], r2 = ex[8 * 32];
            float val[9];
#pragma unroll
            for (int m = 0; m < 4; ++m) {
                const int n = L + 4 * m, q = n / 3, a = n - 3 * q;
                const float v = a == 0 ? r0 : a == 1 ? r1 : r2;
                sincosf(v * (float)(1 << q), &val[2 * m], &val[2 * m + 1]);          // 2^q v is exact in fp32
            }
            val[8] = L == 0 ? r0 : L == 1 ? r1 : r2;
            float p[32];
#pragma unroll
            for (int o = 0; o < 32; ++o) p[o] = 0.f;
#pragma unroll
            for (int sl = 0; sl < 9; ++sl)
#pragma unroll
                for (int oq = 0; oq < 8; ++oq) {
                    const float4 w = wb4[(sl * 8 + oq) * 4 + L];
                    p[4 * oq] += w.x * val[sl]; p[4 * oq + 1] += w.y * val[sl]; p[4 * oq + 2] += w.z * val[sl]; p[4 * oq + 3] += w.w * val[sl];
                }
#pragma unroll
            for (int o = 0; o < 32; ++o) {
                const float s = quad_sum(p[o]);
                if (L == 2) x[o] += s;
            }
        }
        if constexpr (TRANS) {
            transformer_quad(weights + OSG_HEAD_FLOATS, qb, x);
            if (L == 3) {
#pragma unroll
                for (int k = 0; k < 32; ++k) x[k] = 0.f;
            }
        }
        // ---- OSGDecoder: mean over the tokens, 16 of the 64 hidden units per lane ----
#pragma unroll
        for (int k = 0; k < 32; ++k) x[k] = quad_sum(x[k]) * (1.0f / 3.0f);
        float y0 = 0.f, y1 = 0.f, y2 = 0.f, y3 = 0.f;
#pragma unroll 4
        for (int i = 0; i < 16; ++i) {
            float a = lds[OSG_HB0 + i * 4 + L];
#pragma unroll
            for (int kq = 0; kq < 8; ++kq) {
                const float4 w = h04[(i * 8 + kq) * 4 + L];
                a += w.x * x[4 * kq] + w.y * x[4 * kq + 1] + w.z * x[4 * kq + 2] + w.w * x[4 * kq + 3];
            }
            const float sp = a > 20.0f ? a : log1pf(expf(a));                        // torch.nn.Softplus(): beta 1, linear above 20
            const float4 w1 = h14[i * 4 + L];
            y0 += w1.x * sp; y1 += w1.y * sp; y2 += w1.z * sp; y3 += w1.w * sp;
        }
        y0 = quad_sum(y0) + lds[OSG_HB1]; y1 = quad_sum(y1) + lds[OSG_HB1 + 1]; y2 = quad_sum(y2) + lds[OSG_HB1 + 2]; y3 = quad_sum(y3) + lds[OSG_HB1 + 3];
        if (live && L == 0) {
            // sigma = y0; rgb = sigmoid(y1..3) * (1 + 2 * 0.001) - 0.001 (triplane.py:263-264)
            const float r = 1.0f / (1.0f + expf(-y1)) * 1.002f - 0.001f, g = 1.0f / (1.0f + expf(-y2)) * 1.002f - 0.001f,
                        b = 1.0f / (1.0f + expf(-y3)) * 1.002f - 0.001f;
            out[c] = make_float4(r, g, b, y0);
        }
    }
}

}  // namespace

extern "C" int sherf_osg_decoder(const int32_t* counters, const float* tokens, const float* extras, const float* weights, int flags,
                                 int64_t capacity, float* out, sherf_stream_t stream) {
    SHERF_CHECK_ARG(counters && tokens && extras && weights && out);
    SHERF_CHECK_ARG((flags & ~1) == 0 && capacity > 0);
    const dim3 grid((unsigned)((capacity + OSG_BLOCK_SAMPLES - 1) / OSG_BLOCK_SAMPLES)), block(OSG_THREADS);
    if (flags & 1)
        hipLaunchKernelGGL((osg_decoder_kernel<false>), grid, block, 0, as_stream(stream), counters, reinterpret_cast<const float4*>(tokens), extras,
                           weights, capacity, reinterpret_cast<float4*>(out));
    else
        hipLaunchKernelGGL((osg_decoder_kernel<true>), grid, block, 0, as_stream(stream), counters, reinterpret_cast<const float4*>(tokens), extras,
                           weights, capacity, reinterpret_cast<float4*>(out));
    SHERF_LAUNCH_CHECK();
}
