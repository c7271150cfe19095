// What the sources of libsherf_hip.so share about a frame's SAMPLE PASS -- included from the end of common.h, never on its own.
//
// A sample pass is the body index (the posed vertices' cell lists, near mask and near lists: built once per frame, read only from then on) plus
// ONE SET OF BUFFERS: the sampler's (compact records per valid sample, the per-ray bookkeeping) and the token side's (warp, gather and network
// outputs).  A frame has one pass (sherf_frame), an importance frame a second one on buffers of its own (sherf_importance) over the same index.
// The samplers and the warp (csrc/sample.hip, csrc/field.hip) take a pass as these two values; csrc/frame.hip builds them from the descriptors.
#pragma once
#include <functional>

struct SherfBodyIndex {
    const float* Rg; const float* Th;                   // world -> SMPL frame
    const float* grid_hdr; const int32_t* cell_start; const float* cell_pts;
    const uint32_t* near_mask;
    const int32_t* near_hdr; const uint16_t* near_list; // both or neither (NULL: the cell-walk search)
};

struct SherfSamples {
    int32_t* counters; int32_t* ray_base; int32_t* ray_cnt; int32_t* cs_idx; int32_t* cs_vid; float* cs_xs;
    int32_t* dense_vid; uint64_t* ray_mask; int32_t* scan_ws;
    int64_t capacity;                                   // records that cs_idx / cs_vid / cs_xs hold
    float* geom; int32_t* cs_tvid; float* tokens; float* extras; float* sample_out;
    int64_t tok_cap;                                    // samples that geom / tokens / extras / sample_out hold: resolved, never 0
};

// a frame's rays: R rays of S samples between near[r] and far[r]
struct SherfRays { const float* o; const float* d; const float* near; const float* far; int R, S; };

static inline SherfBodyIndex body_index(const sherf_frame& f) {
    const bool lists = f.near_hdr && f.near_list;       // exact vertex list per near-mask sub-cell: its counts also give the mask
    return {f.Rg, f.Th, f.grid_hdr, f.cell_start, f.cell_pts, f.near_mask, lists ? f.near_hdr : nullptr, lists ? f.near_list : nullptr};
}
// token-side capacity: what geom / tokens / extras / sample_out hold (0, or more than the sampler's: `capacity`)
static inline int64_t sherf_tok_cap(int64_t tok_capacity, int64_t capacity) { return (tok_capacity > 0 && tok_capacity < capacity) ? tok_capacity : capacity; }
static inline SherfSamples samples(const sherf_frame& f) {
    return {f.counters, f.ray_base, f.ray_cnt, f.cs_idx, f.cs_vid, f.cs_xs, f.dense_vid, f.ray_mask, f.scan_ws, f.capacity,
            f.geom, f.cs_tvid, f.tokens, f.extras, f.sample_out, sherf_tok_cap(f.tok_capacity, f.capacity)};
}
static inline SherfSamples samples(const sherf_importance& i) {
    return {i.counters, i.ray_base, i.ray_cnt, i.cs_idx, i.cs_vid, i.cs_xs, i.dense_vid, i.ray_mask, i.scan_ws, i.capacity,
            i.geom, i.cs_tvid, i.tokens, i.extras, i.sample_out, sherf_tok_cap(i.tok_capacity, i.capacity)};
}

// ---- the internals one source calls in another: declared here and nowhere else ----
// csrc/svox.hip
int sherf_svox_encode_impl(const sherf_svox_plan* p, const int32_t* coord, const float* feat, int n, int training,
                           sherf_vox_level* levels_out_host, sherf_stream_t stream, hipEvent_t ev, int ev_layer,
                           sherf_stream_t aux, hipEvent_t* lev_ev, const std::function<int()>* after_levels, int fold_half);
// csrc/sample.hip.  The ray sampler (`sticky`: see init_counters_kernel; `cell_ws`: the workspace of the search by sub-cell, or NULL)
int sherf_sample_mask_nn_impl(const SherfRays& rays, const SherfBodyIndex& bi, const SherfSamples& s, sherf_stream_t stream, int32_t* sticky,
                              int32_t* cell_ws, int64_t cell_ws_len);
// The point sampler's use of the ray sampler's machinery (`rows` rows of 64 points).  _begin resets the counters and the candidate count ahead of
// point_mark_kernel; _search runs the candidate search on the list in s.cs_xs and both scan kernels behind it: counters[0] = the valid points.
int sherf_points_begin_impl(int32_t* counters, int32_t* scan_ws, int rows, int32_t* sticky, sherf_stream_t stream);
int sherf_points_search_impl(int rows, const SherfBodyIndex& bi, const SherfSamples& s, sherf_stream_t stream);
// The warp of a pass's s.tok_cap first samples into s.geom / s.cs_tvid.  `target`: Rg and the cell list of the TARGET-pose vertices `t_verts`.
// `dir_stride`: how many consecutive dense indices share one row of `dirs` -- S for a frame's rays (the exported entry point, which refuses S < 2),
// 1 for the field query's per-point view directions (dirs[cs_idx[c]]).  The kernel divides cs_idx by it either way.
int sherf_warp_geom_impl(const SherfBodyIndex& target, const float* T2C, const float* C2S, const float* t_verts, const SherfSamples& s,
                         sherf_stream_t stream, const float* dirs, int dir_stride);
// csrc/field.hip.  The point sampler
int sherf_points_mask_nn_impl(const float* points, int64_t n, const SherfBodyIndex& bi, const SherfSamples& s, sherf_stream_t stream, int32_t* sticky);

// ---- marcher arithmetic that the sampler, the compositing and the importance depths must evaluate to the same bits: ONE definition ----
__device__ __forceinline__ float depth_at(float near, float range, int k, int S) {
    // math_utils.py:101-118: steps = arange(S)/(S-1);  t = near + steps * (far - near)
    float step = __fdiv_rn((float)k, (float)(S - 1));
    return __fadd_rn(near, __fmul_rn(step, range));
}

enum { CLAMP_RELU = 0, CLAMP_SOFTPLUS = 1 };

// the density activation of ray_marcher.py:37-40
template <int MODE>
__device__ __forceinline__ float density(float sigma) {
    if (MODE == CLAMP_RELU) return fmaxf(sigma, 0.f);
    const float x = sigma - 1.f;
    return x > 20.f ? x : log1pf(expf(x));
}

// d density / d sigma (threshold_backward / softplus_backward)
template <int MODE>
__device__ __forceinline__ float density_grad(float sigma) {
    if (MODE == CLAMP_RELU) return sigma > 0.f ? 1.f : 0.f;
    const float x = sigma - 1.f;
    const float z = expf(x);
    return x > 20.f ? 1.f : z / (z + 1.f);
}
