// What the position-attention layers beside the main mesh path share: ragged batches (pit_ragged.hip), mesh gradients
// (pit_dmesh.hip), caller-supplied distance matrices (pit_distmat.hip) and candidate lists (pit_distlist.hip).  Their kernels
// differ - the geometry, the tile machines, the order of every sum - and stay in their files.  The operands around the geometry,
// the small device helpers and the host side's checks of those operands are the same for all of them and live here, once.
// Nothing below knows which path calls it.
#pragma once
#include "pit_common.h"

namespace {

// The layer's operands apart from its geometry.  The argument structs of the kernels derive from it and add their geometry and
// extras; they are passed by value as before.  (rank_w stays with them: a float for matrices and lists, per sample for ragged.)
struct LayerIO {
    const float* values; int dim; long ld_values, values_bstride;
    const float* head; int n_head, head_is_scale;
    const float* stats; int masked;
    float* out; long ld_out, out_bstride; int out_col0, copy_inputs;
    float* rowstat; float* scale_out;
    const float* d_out; long ld_dout, dout_bstride;
    float* d_values; long ld_dvalues, dvalues_bstride; int add_residual;
    double* dscale_acc;
    int colgroups;                               // groups of 256 value columns
    unsigned values_bytes, dout_bytes;           // of ONE sample's rows: the sizes of the buffer descriptors
};

// ---- device ---------------------------------------------------------------------------------------------------------------
// the head's scale c (a: anything with head and head_is_scale)
template <class Args>
__device__ __forceinline__ float head_c(const Args& a, int h) {
    return a.head_is_scale ? a.head[h] : head_scale_from_lmda(a.head[h]);
}

// {T, S_min, 1/rowsum, mbar} the forward saved for a row of list set / mesh mb and head h
__device__ __forceinline__ float4 row_stat(const float* rowstat, int n_head, int n_out, int mb, int h, int row) {
    return *reinterpret_cast<const float4*>(rowstat + (((long)mb * n_head + h) * n_out + row) * 4);
}

// the forward's unnormalised weight of one pair (pit_posatt.hip: exp(S_min - S), kept if S <= T)
__device__ __forceinline__ float weight_raw(float m, float c, float T, float smin, bool valid, int masked) {
    const float sv = __fmul_rn(m, c);
    const bool keep = valid && (!masked || sv <= T);
    return keep ? __expf(smin - sv) : 0.0f;
}

// A sample's point count on one side of a ragged batch, clamped into [1, n].  len == NULL: a side without lengths - every sample
// has the full width (the shared mesh of a mixed pair, or a cloud side given without lengths); a wave-uniform branch on a
// kernel argument
__device__ __forceinline__ int clamp_len(const int* len, int s, int n) { return len ? max(1, min(len[s], n)) : n; }

// torch.quantile's rank in ATen's fp32 arithmetic for a sample of `li` keys (ops.quantile_rank: fp32 product, floor, fp32
// difference); q = fl32(locality).  Returns k, w in `w`.
__device__ __forceinline__ int sample_rank(float q, int li, float& w) {
    const float rank = __fmul_rn(q, (float)(li - 1));
    const int k = (int)floorf(rank);
    w = __fsub_rn(rank, (float)k);
    return k;
}

// lane src's v, in every lane (src wave-uniform)
__device__ __forceinline__ float lane_f(float v, int src) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), src)); }

// gv tile: acc[r] of lane l = sum_d g[i0 + acc_row(r, half)][d] * v[j0 + (l & 31)][d].  gbase / vbase: the byte offsets in
// the descriptors rg / rv of channel 0 of the lane's row i0 + (l & 31) and key j0 + (l & 31) (0 where rvalid / kvalid is
// false).  A lane holds channels d0 + 4*half + u (u = 0..3) of its row / key: four MFMAs per group of 8 channels; channels,
// rows and keys out of range read 0 through the buffer descriptors.
__device__ __forceinline__ f32x16 gv_tile(__amdgpu_buffer_rsrc_t rg, __amdgpu_buffer_rsrc_t rv, unsigned gbase, bool rvalid,
                                          unsigned vbase, bool kvalid, int dim, unsigned dout_bytes, unsigned values_bytes) {
    const int half = (threadIdx.x & 63) >> 5;
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.0f;
    for (int d0 = 0; d0 < dim; d0 += 8) {
        float ga[4], vb[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int d = d0 + 4 * half + u;
            const bool ok = d < dim;
            ga[u] = buf_load(rg, (rvalid && ok) ? gbase + (unsigned)d * 4u : dout_bytes);
            vb[u] = buf_load(rv, (kvalid && ok) ? vbase + (unsigned)d * 4u : values_bytes);
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) acc = mfma_32x32x2(ga[u], vb[u], acc);
    }
    return acc;
}

// ---- host -----------------------------------------------------------------------------------------------------------------
unsigned long long rows_bytes(int rows, long ld, long width) { return ((unsigned long long)(rows - 1) * ld + width) * 4ull; }

// the operands of a forward entry
void layer_set_fwd(LayerIO& a, const float* values, int dim, long ld_values, long values_bstride,
                   const float* head, int n_head, int head_is_scale, const float* stats, int masked,
                   float* out, long ld_out, long out_bstride, int out_col0, int copy_inputs, float* rowstat, float* scale_out) {
    a.values = values; a.dim = dim; a.ld_values = ld_values; a.values_bstride = values_bstride;
    a.head = head; a.n_head = n_head; a.head_is_scale = head_is_scale;
    a.stats = stats; a.masked = masked ? 1 : 0;
    a.out = out; a.ld_out = ld_out; a.out_bstride = out_bstride; a.out_col0 = out_col0; a.copy_inputs = copy_inputs ? 1 : 0;
    a.rowstat = rowstat; a.scale_out = scale_out;
}

// the operands of a backward entry; the forward's scale_out, where the caller kept it, is read in place of the head
void layer_set_bwd(LayerIO& a, const float* values, int dim, long ld_values, long values_bstride,
                   const float* head, int n_head, int head_is_scale, const float* scale, const float* rowstat, int masked,
                   const float* d_out, long ld_dout, long dout_bstride, int out_col0,
                   float* d_values, long ld_dvalues, long dvalues_bstride, int add_residual, float* d_head, double* workspace) {
    a.values = values; a.dim = dim; a.ld_values = ld_values; a.values_bstride = values_bstride;
    a.head = scale ? scale : head; a.n_head = n_head; a.head_is_scale = (scale || head_is_scale) ? 1 : 0;
    a.rowstat = const_cast<float*>(rowstat); a.masked = masked ? 1 : 0;
    a.d_out = d_out; a.ld_dout = ld_dout; a.dout_bstride = dout_bstride; a.out_col0 = out_col0;
    a.d_values = d_values; a.ld_dvalues = ld_dvalues; a.dvalues_bstride = dvalues_bstride; a.add_residual = add_residual ? 1 : 0;
    a.dscale_acc = d_head ? workspace : nullptr;
}

// The two checks of the operands every path shares; an entry's grid limits and its out and d_values operands are its own to
// check.  The values operands (n_in rows): fills colgroups and the size of the per-sample descriptor.
int layer_check_values(LayerIO& a, int n_in) {
    if (a.dim <= 0 || a.n_head <= 0 || a.ld_values < a.dim || a.values_bstride < 0) return PIT_ERR_SIZE;
    const unsigned long long vb = rows_bytes(n_in, a.ld_values, a.dim);
    if (vb > PIT_MAX_BUFFER_BYTES) return PIT_ERR_UNSUPPORTED;
    a.values_bytes = (unsigned)vb;
    a.colgroups = (a.dim + 255) / 256;
    return 0;
}

// The d_out operands (dout_rows rows of the head columns; after layer_check_values): fills the size of the per-sample descriptor.
int layer_check_dout(LayerIO& a, int dout_rows) {
    if (a.out_col0 < 0 || a.ld_dout < a.out_col0 + (long)a.n_head * a.dim || a.dout_bstride < 0) return PIT_ERR_SIZE;
    const unsigned long long db = rows_bytes(dout_rows, a.ld_dout, a.out_col0 + (long)a.n_head * a.dim);
    if (db > PIT_MAX_BUFFER_BYTES) return PIT_ERR_UNSUPPORTED;
    a.dout_bytes = (unsigned)db;
    return 0;
}

// The tail of a backward entry: unless the caller defers it, drain the fp64 slots of d(scale) and apply d c / d lmda
// (pit_posatt_dhead_finish for this one layer).
int layer_finish_head(const float* head, const float* scale, float* d_head, double* workspace, int n_head, int accumulate_head,
                      int head_is_scale, void* stream) {
    if (!d_head || (accumulate_head & PIT_HEAD_DEFER)) return 0;
    double* ws[1] = {workspace};
    float* dh[1] = {d_head};
    const float* hd[1] = {head};
    const float* sc[1] = {scale};
    const int nh[1] = {n_head};
    const int fl[1] = {(accumulate_head & PIT_HEAD_ACCUMULATE) | (head_is_scale ? PIT_HEAD_IS_SCALE : 0)};
    return pit_posatt_dhead_finish(1, ws, dh, hd, sc, nh, fl, nullptr, stream);
}

}  // namespace
