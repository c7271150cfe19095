// Field query (gfx950): density and colour at caller-supplied 3-D points -- ImportanceRenderer.forward from the SMPL-frame transform to the scatter-back
// (renderer.py:307-368) with `sample_coordinates` / `sample_directions` handed in instead of derived from rays; what TriPlaneGenerator.sample /
// sample_mixed declare (triplane.py:219-230).  Two stages are new, the rest is the frame's (csrc/frame.hip: sherf_query_field):
//   point sampler   the N points are laid out as rows of 64 (row r = points 64 r .. 64 r + 63, the last row ragged): a row is to the candidate search, the
//                   scans and the bookkeeping buffers (ray_mask / dense_vid / ray_base / ray_cnt) what a ray of S = 64 samples is, so all of those run
//                   unchanged (csrc/sample.hip: search_and_scan).  point_mark_kernel reads x = points[i] where cand_mark_kernel forms o + t d, then applies
//                   the same (x - Th) R arithmetic (csrc/common.h: to_smpl_frame) and the same near-mask test; compact_points_kernel writes the compact
//                   records in ascending point order -- the reference's boolean-mask order (renderer.py:320) -- from the rows' masks and scanned bases:
//                   deterministic, no atomics.
//   scatter-back    colors_coarse / densities_coarse of renderer.py:364-368 materialised: one lane per point, the point's compact position recomputed from its
//                   row's mask word and base, one pass, no separate fill.
#include "common.h"

namespace {

constexpr int kMarkRows = 4;          // rows in flight per wave of the mark pass (cand_mark_kernel: kMarkRays)
constexpr int kRowsPerWg = 16;        // a workgroup of four waves stages at most 16 * 64 = 1024 candidate records (16 KiB of LDS)

// Pass 1 of the point sampler.  A wave takes four consecutive rows (256 consecutive points: the loads of a row are 768 contiguous bytes), every row's
// near-mask word is requested before the first one is looked at.  A candidate's record (x_s, point index) is staged in LDS and the workgroup's records are
// appended to the global list with ONE reservation per workgroup; their order in the list is irrelevant (results land in per-row bit masks).  Absent
// points of the ragged last row never become candidates.  The row's mask word is zeroed here: the search ORs the valid bits in.
__global__ void __launch_bounds__(256) point_mark_kernel(const float* __restrict__ points, int64_t N, int rows, const float* __restrict__ Rg,
                                                         const float* __restrict__ Th, const float* __restrict__ hdr,
                                                         const uint32_t* __restrict__ near_mask, float4* __restrict__ cand_list, int64_t list_cap,
                                                         int32_t* __restrict__ cand_count, uint64_t* __restrict__ ray_mask, int dbg) {
    __shared__ float4 s_rec[kRowsPerWg * 64];
    __shared__ int s_n, s_base;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (threadIdx.x == 0) s_n = 0;
    __syncthreads();
    const CellGrid g = load_grid(hdr);
    const float fs = g.inv_cell * (float)g.sub;
    const int row0 = (int)blockIdx.x * kRowsPerWg + wave * kMarkRows;
    float xs[kMarkRows], ys[kMarkRows], zs[kMarkRows];
    uint32_t word[kMarkRows];
    int bit[kMarkRows];
#pragma unroll
    for (int u = 0; u < kMarkRows; ++u) {
        const int64_t i = (int64_t)(row0 + u) * 64 + lane;
        bit[u] = -1; word[u] = 0u; xs[u] = ys[u] = zs[u] = 0.f;
        if (row0 + u < rows && i < N) {
            const float* p = points + (size_t)i * 3;
            to_smpl_frame(p[0], p[1], p[2], Rg, Th, xs[u], ys[u], zs[u]);
            // (cand_mark_kernel's sub-cell arithmetic on the same floats)
            const int sx = (int)floorf((xs[u] - g.ox) * fs), sy = (int)floorf((ys[u] - g.oy) * fs), sz = (int)floorf((zs[u] - g.oz) * fs);
            const int cx = g.sub == 2 ? sx >> 1 : sx, cy = g.sub == 2 ? sy >> 1 : sy, cz = g.sub == 2 ? sz >> 1 : sz;
            if (sx >= 0 && cx < g.nx && sy >= 0 && cy < g.ny && sz >= 0 && cz < g.nz) {
                const int q = (sz * (g.ny * g.sub) + sy) * (g.nx * g.sub) + sx;
                bit[u] = q & 31;
                word[u] = near_mask[q >> 5];
            }
        }
    }
#pragma unroll
    for (int u = 0; u < kMarkRows; ++u) {
        const int row = row0 + u;
        const bool cand = bit[u] >= 0 && (((dbg & 2) || ((word[u] >> bit[u]) & 1u)) && !(dbg & 1));
        const unsigned long long cm = __ballot(cand);
        if (row < rows && lane == 0) ray_mask[row] = 0ull;
        if (cm) {
            int base = 0;
            if (lane == 0) base = atomicAdd(&s_n, __popcll(cm));
            base = __shfl(base, 0);
            if (cand) s_rec[base + __popcll(cm & ((1ull << lane) - 1ull))] = make_float4(xs[u], ys[u], zs[u], __int_as_float((int)((int64_t)row * 64 + lane)));
        }
    }
    __syncthreads();
    const int n = s_n;
    if (threadIdx.x == 0) s_base = n ? atomicAdd(cand_count, n) : 0;
    __syncthreads();
    const int64_t gb = s_base;
    for (int i = threadIdx.x; i < n; i += 256)
        if (gb + i < list_cap) cand_list[gb + i] = s_rec[i];
}

// Pass 2: one wave per row, a lane per point: the compact records in ascending point order.  cs_xs is evaluated again from the point (the candidate list
// it would otherwise be read from lives in the same buffer) with the operations of the mark pass: the same bits.
__global__ void __launch_bounds__(256) compact_points_kernel(const float* __restrict__ points, int rows, const float* __restrict__ Rg,
                                                             const float* __restrict__ Th, const int32_t* __restrict__ base_local,
                                                             const int32_t* __restrict__ chunk_off, const uint64_t* __restrict__ ray_mask,
                                                             const int32_t* __restrict__ dense_vid, int64_t capacity, int32_t* __restrict__ ray_base,
                                                             int32_t* __restrict__ cs_idx, int32_t* __restrict__ cs_vid, float4* __restrict__ cs_xs) {
    const int lane = threadIdx.x & 63;
    const int row = (int)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const int base = base_local[row] + chunk_off[row >> 10];
    if (lane == 0) ray_base[row] = base;
    const uint64_t m = ray_mask[row];
    if (!((m >> lane) & 1ull)) return;
    const int64_t c = (int64_t)base + __popcll(m & ((1ull << lane) - 1ull));
    if (c >= capacity) return;
    const int64_t i = (int64_t)row * 64 + lane;           // (< N: only present points were marked)
    const float* p = points + (size_t)i * 3;
    float xs, ys, zs;
    to_smpl_frame(p[0], p[1], p[2], Rg, Th, xs, ys, zs);
    cs_idx[c] = (int)i;
    cs_vid[c] = dense_vid[i];
    cs_xs[c] = make_float4(xs, ys, zs, 0.f);
}

// Scatter-back (renderer.py:364-368): rgb 0 / sigma -80 where the shell mask failed, the compact sample's outputs elsewhere.  A point whose compact position
// lies beyond what sample_out holds (tok_cap) was not evaluated: NaN and counters[3] |= 2, as the compositing treats such a ray; sample_out is not read there.
__global__ void __launch_bounds__(256) field_scatter_kernel(const uint64_t* __restrict__ ray_mask, const int32_t* __restrict__ ray_base,
                                                            const float4* __restrict__ sample_out, int64_t N, int64_t tok_cap, int32_t* __restrict__ flags,
                                                            float* __restrict__ rgb, float* __restrict__ sigma, uint8_t* __restrict__ mask) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= N) return;
    const int64_t row = i >> 6;
    const int k = (int)(i & 63);
    const uint64_t m = ray_mask[row];
    float4 o = make_float4(0.f, 0.f, 0.f, -80.0f);
    const bool valid = (m >> k) & 1ull;
    if (valid) {
        const int64_t c = (int64_t)ray_base[row] + __popcll(m & ((1ull << k) - 1ull));
        if (c < tok_cap) {
            o = sample_out[c];
        } else {
            const float qnan = __int_as_float(0x7fc00000);
            o = make_float4(qnan, qnan, qnan, qnan);
            atomicOr(flags, 2);
        }
    }
    float* c3 = rgb + (size_t)i * 3;
    c3[0] = o.x; c3[1] = o.y; c3[2] = o.z;
    sigma[i] = o.w;
    mask[i] = valid ? 1 : 0;
}

}  // namespace

int sherf_points_mask_nn_impl(const float* points, int64_t n, const SherfBodyIndex& bi, const SherfSamples& s, sherf_stream_t stream, int32_t* sticky) {
    SHERF_CHECK_ARG(points && bi.Rg && bi.Th && bi.grid_hdr && bi.cell_start && bi.cell_pts && bi.near_mask);
    SHERF_CHECK_ARG(s.counters && s.ray_base && s.ray_cnt && s.cs_idx && s.cs_vid && s.cs_xs && s.dense_vid && s.ray_mask && s.scan_ws);
    SHERF_CHECK_ARG(n > 0 && n < 2147483648LL && s.capacity > 0 && (bi.near_hdr == nullptr) == (bi.near_list == nullptr));
    SHERF_CHECK_ARG(s.capacity >= n);                   // (cs_xs doubles as the candidate list: it must hold a record per point)
    hipStream_t st = as_stream(stream);
    const int rows = (int)((n + 63) / 64);
    const SherfScanWs w = sherf_scan_ws(s.scan_ws, rows);
    SHERF_RUN(sherf_points_begin_impl(s.counters, s.scan_ws, rows, sticky, stream));
    hipLaunchKernelGGL(point_mark_kernel, dim3(cdiv(rows, kRowsPerWg)), dim3(256), 0, st, points, n, rows, bi.Rg, bi.Th, bi.grid_hdr, bi.near_mask,
                       reinterpret_cast<float4*>(s.cs_xs), s.capacity, w.cand_count, s.ray_mask, g_sherf_debug);
    SHERF_RUN(sherf_points_search_impl(rows, bi, s, stream));
    hipLaunchKernelGGL(compact_points_kernel, dim3(cdiv(rows, 4)), dim3(256), 0, st, points, rows, bi.Rg, bi.Th, w.base_local, w.chunk_sum, s.ray_mask, s.dense_vid,
                       s.capacity, s.ray_base, s.cs_idx, s.cs_vid, reinterpret_cast<float4*>(s.cs_xs));
    SHERF_LAUNCH_CHECK();
}

extern "C" int sherf_points_mask_nn(const float* points, int64_t n, const float* Rg, const float* Th, const float* grid_hdr, const int32_t* cell_start,
                                    const float* cell_pts, const uint32_t* near_mask, int64_t capacity, int32_t* counters, int32_t* ray_base,
                                    int32_t* ray_cnt, int32_t* cs_idx, int32_t* cs_vid, float* cs_xs, int32_t* dense_vid, uint64_t* ray_mask,
                                    int32_t* scan_ws, const int32_t* near_hdr, const uint16_t* near_list, sherf_stream_t stream) {
    return sherf_points_mask_nn_impl(points, n, {Rg, Th, grid_hdr, cell_start, cell_pts, near_mask, near_hdr, near_list},
                                     {counters, ray_base, ray_cnt, cs_idx, cs_vid, cs_xs, dense_vid, ray_mask, scan_ws, capacity}, stream, nullptr);
}

extern "C" int sherf_field_scatter(int32_t* counters, const uint64_t* ray_mask, const int32_t* ray_base, const float* sample_out, int64_t n, int64_t tok_cap,
                                   float* rgb, float* sigma, uint8_t* mask, sherf_stream_t stream) {
    SHERF_CHECK_ARG(counters && ray_mask && ray_base && sample_out && rgb && sigma && mask);
    SHERF_CHECK_ARG(n > 0 && n < 2147483648LL && tok_cap > 0);
    hipLaunchKernelGGL(field_scatter_kernel, dim3(cdiv(n, 256)), dim3(256), 0, as_stream(stream), ray_mask, ray_base,
                       reinterpret_cast<const float4*>(sample_out), n, tok_cap, counters + 3, rgb, sigma, mask);
    SHERF_LAUNCH_CHECK();
}
