// Gradients of the position attention w.r.t. the mesh coordinates (Euclidean metric, fp32), for gfx950.
//
// The reference forms m = sum((mesh_out[:,None] - mesh_in[None])**2) with ordinary tensor ops (pit.py:47,134), so autograd
// differentiates through the coordinates.  Per head h (c = c_h), with P the kept softmax weights the forward used,
// g_i = d_out[i, out_col0 + h*dim : +dim], gv_ij = g_i . v_j and a_i = sum_j P_ij gv_ij:
//     s_ij = P_ij (gv_ij - a_i)                      (d loss / d logit, logit = -c m)
//     d mesh_out[i] = 2c sum_j s_ij (y_j - x_i)      (= 2c sum_j s_ij y_j, since sum_j s_ij = 0)
//     d mesh_in[j]  = 2c sum_i s_ij (x_i - y_j)
// summed over heads and, for batch-free meshes, over the samples.  The quantile threshold only feeds a comparison: no term.
//
//   rows pass (d mesh_out; also writes a_i for the cols pass): a wave owns 32 rows of one sample.  The dense layers form
//       the 32 x 32 tiles of gv with v_mfma_f32_32x32x2_f32 (A = d_out rows, B = value rows, the channel axis contracted),
//       once for a_i and once for the centred sum sum_j P (gv - a) (y - x) - no cancellation between two large sums.
//   cols pass (d mesh_in): a wave owns 32 keys of one sample; the same tiles, the weighted sum taken per key.
//   candidate lists: a wave per row (row -> keys lists) / per key (transposed lists, plus the rows whose list overflowed,
//       which are scanned densely as pit_posatt_bwd does); the dot products are wave reductions, the sums fp64.
// No atomics: every pass writes per-sample partials into the caller's workspace and one reduction kernel per output sums
// them in sample order, so the result is the same bits on every run.
#include "pit_layer.h"

namespace {

struct DmArgs {
    const float* mesh_out; const float* mesh_in;
    int mesh_batch, n_out, n_in, sdim;
    const float* values; int batch, dim; long ld_values, values_bstride;
    const float* head; const float* scale; int n_head, head_is_scale;
    const float* rowstat; int masked;
    const float* d_out; long ld_dout, dout_bstride; int out_col0;
    const int* nbr_idx; const int* nbr_cnt; int cap, complete;
    const int* rev_ptr; const int* rev_row;
    float* a_ws;                // (batch, n_head, n_out): a_i
    float* rows_ws;             // (batch, n_out, sdim): per-sample d mesh_out
    float* cols_ws;             // (batch, n_in, sdim): per-sample d mesh_in
    unsigned values_bytes, dout_bytes;
};

// the forward's scale_out, where the caller kept it, in place of the head
__device__ __forceinline__ float scale_c(const DmArgs& a, int h) { return a.scale ? a.scale[h] : head_c(a, h); }

__device__ __forceinline__ void load_pt(const float* mesh, long idx, int sdim, float& x, float& y, float& z) {
    const float* p = mesh + idx * sdim;
    x = p[0];
    y = sdim > 1 ? p[1] : 0.0f;
    z = sdim > 2 ? p[2] : 0.0f;
}

// the forward's weight of one (row, key) pair (pit_posatt.hip: P = exp(S_min - S) / rowsum, kept if S <= T)
__device__ __forceinline__ float weight(float m, float c, float4 rs, bool valid, int masked) {
    const float sv = __fmul_rn(m, c);
    const bool keep = valid && (!masked || sv <= rs.x);
    return keep ? __expf(rs.y - sv) * rs.z : 0.0f;
}

// gv tile (pit_layer.h) for sample s, head h, rows i0 .. i0 + 31 and keys j0 .. j0 + 31; the descriptors span the whole batch
__device__ __forceinline__ f32x16 gv_tile_at(const DmArgs& a, __amdgpu_buffer_rsrc_t rdo, __amdgpu_buffer_rsrc_t rv,
                                             int s, int h, int i0, int j0) {
    const int l31 = threadIdx.x & 31;
    const int row = i0 + l31, key = j0 + l31;
    const bool rvalid = row < a.n_out, kvalid = key < a.n_in;
    const unsigned gbase = rvalid ? (unsigned)(((long)s * a.dout_bstride + (long)row * a.ld_dout + a.out_col0 + (long)h * a.dim) * 4) : 0u;
    const unsigned vbase = kvalid ? (unsigned)(((long)s * a.values_bstride + (long)key * a.ld_values) * 4) : 0u;
    return gv_tile(rdo, rv, gbase, rvalid, vbase, kvalid, a.dim, a.dout_bytes, a.values_bytes);
}

// sum over the 32 lanes of a half-wave (lanes l and l ^ 32 keep their own sums)
__device__ __forceinline__ float half_sum(float v) {
#pragma unroll
    for (int o = 1; o < 32; o <<= 1) v += __shfl_xor(v, o);
    return v;
}

// ---- dense layers ----------------------------------------------------------------------------------------------------
// grid (ceil(n_out / 32), batch), one wave
__global__ __launch_bounds__(64) void dmesh_rows_dense(DmArgs a) {
    __shared__ float4 s_x[32];
    __shared__ float4 s_rs[32];
    const int lane = threadIdx.x & 63, half = lane >> 5, l31 = lane & 31;
    const int i0 = blockIdx.x * 32, s = blockIdx.y;
    const int mb = a.mesh_batch == 1 ? 0 : s;
    const __amdgpu_buffer_rsrc_t rdo = make_rsrc(a.d_out, a.dout_bytes);
    const __amdgpu_buffer_rsrc_t rv = make_rsrc(a.values, a.values_bytes);
    float dx[16][3];
#pragma unroll
    for (int r = 0; r < 16; ++r) dx[r][0] = dx[r][1] = dx[r][2] = 0.0f;
    if (lane < 32) {
        const int row = min(i0 + lane, a.n_out - 1);
        float4 p; load_pt(a.mesh_out, (long)mb * a.n_out + row, a.sdim, p.x, p.y, p.z); p.w = 0.0f;
        s_x[lane] = p;
    }
    for (int h = 0; h < a.n_head; ++h) {
        const float c = scale_c(a, h);
        __syncthreads();
        if (lane < 32) s_rs[lane] = row_stat(a.rowstat, a.n_head, a.n_out, mb, h, min(i0 + lane, a.n_out - 1));
        __syncthreads();
        float ap[16];
#pragma unroll
        for (int r = 0; r < 16; ++r) ap[r] = 0.0f;
        for (int pass = 0; pass < 2; ++pass) {
            float w2[16][3];
#pragma unroll
            for (int r = 0; r < 16; ++r) w2[r][0] = w2[r][1] = w2[r][2] = 0.0f;
            for (int j0 = 0; j0 < a.n_in; j0 += 32) {
                const f32x16 gv = gv_tile_at(a, rdo, rv, s, h, i0, j0);
                const int key = j0 + l31;
                const bool kv = key < a.n_in;
                float yx, yy, yz;
                load_pt(a.mesh_in, (long)mb * a.n_in + (kv ? key : 0), a.sdim, yx, yy, yz);
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int ri = acc_row(r, half);
                    const float4 x = s_x[ri];
                    const float m = sq_dist3(x.x, x.y, x.z, yx, yy, yz, false, 0.0f);
                    const float p = weight(m, c, s_rs[ri], kv && i0 + ri < a.n_out, a.masked);
                    if (pass == 0) {
                        ap[r] += p * gv[r];
                    } else {
                        const float t = p * (gv[r] - ap[r]);
                        w2[r][0] += t * (yx - x.x);
                        w2[r][1] += t * (yy - x.y);
                        w2[r][2] += t * (yz - x.z);
                    }
                }
            }
            if (pass == 0) {
#pragma unroll
                for (int r = 0; r < 16; ++r) ap[r] = half_sum(ap[r]);
                if (l31 == 0) {
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const int row = i0 + acc_row(r, half);
                        if (row < a.n_out) a.a_ws[((long)s * a.n_head + h) * a.n_out + row] = ap[r];
                    }
                }
            } else {
                const float c2 = 2.0f * c;
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    dx[r][0] += c2 * w2[r][0];
                    dx[r][1] += c2 * w2[r][1];
                    dx[r][2] += c2 * w2[r][2];
                }
            }
        }
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        float v[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) v[k] = half_sum(dx[r][k]);
        const int row = i0 + acc_row(r, half);
        if (l31 == 0 && row < a.n_out) {
            for (int k = 0; k < a.sdim; ++k) a.rows_ws[((long)s * a.n_out + row) * a.sdim + k] = v[k];
        }
    }
}

// grid (ceil(n_in / 32), batch), one wave
__global__ __launch_bounds__(64) void dmesh_cols_dense(DmArgs a) {
    __shared__ float4 s_x[32];
    __shared__ float4 s_rs[32];
    __shared__ float s_a[32];
    const int lane = threadIdx.x & 63, half = lane >> 5, l31 = lane & 31;
    const int j0 = blockIdx.x * 32, s = blockIdx.y;
    const int mb = a.mesh_batch == 1 ? 0 : s;
    const __amdgpu_buffer_rsrc_t rdo = make_rsrc(a.d_out, a.dout_bytes);
    const __amdgpu_buffer_rsrc_t rv = make_rsrc(a.values, a.values_bytes);
    const int key = j0 + l31;
    const bool kv = key < a.n_in;
    float yx, yy, yz;
    load_pt(a.mesh_in, (long)mb * a.n_in + (kv ? key : 0), a.sdim, yx, yy, yz);
    float dy[3] = {0.0f, 0.0f, 0.0f};
    for (int h = 0; h < a.n_head; ++h) {
        const float c = scale_c(a, h);
        float acc[3] = {0.0f, 0.0f, 0.0f};
        for (int i0 = 0; i0 < a.n_out; i0 += 32) {
            __syncthreads();
            if (lane < 32) {
                const int row = min(i0 + lane, a.n_out - 1);
                float4 p; load_pt(a.mesh_out, (long)mb * a.n_out + row, a.sdim, p.x, p.y, p.z); p.w = 0.0f;
                s_x[lane] = p;
                s_rs[lane] = row_stat(a.rowstat, a.n_head, a.n_out, mb, h, row);
                s_a[lane] = a.a_ws[((long)s * a.n_head + h) * a.n_out + row];
            }
            __syncthreads();
            const f32x16 gv = gv_tile_at(a, rdo, rv, s, h, i0, j0);
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int ri = acc_row(r, half);
                const float4 x = s_x[ri];
                const float m = sq_dist3(x.x, x.y, x.z, yx, yy, yz, false, 0.0f);
                const float p = weight(m, c, s_rs[ri], kv && i0 + ri < a.n_out, a.masked);
                const float t = p * (gv[r] - s_a[ri]);
                acc[0] += t * (x.x - yx);
                acc[1] += t * (x.y - yy);
                acc[2] += t * (x.z - yz);
            }
        }
        const float c2 = 2.0f * c;
#pragma unroll
        for (int k = 0; k < 3; ++k) dy[k] += c2 * acc[k];
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) dy[k] += __shfl_xor(dy[k], 32);
    if (lane < 32 && kv)
        for (int k = 0; k < a.sdim; ++k) a.cols_ws[((long)s * a.n_in + key) * a.sdim + k] = dy[k];
}

// ---- candidate lists -------------------------------------------------------------------------------------------------
// g_i . v_j as a wave reduction (the channels spread over the lanes); every lane gets the sum
__device__ __forceinline__ float wave_dot(const DmArgs& a, int s, int h, int row, int key) {
    const int lane = threadIdx.x & 63;
    const float* g = a.d_out + (long)s * a.dout_bstride + (long)row * a.ld_dout + a.out_col0 + (long)h * a.dim;
    const float* v = a.values + (long)s * a.values_bstride + (long)key * a.ld_values;
    float part = 0.0f;
    for (int d = lane; d < a.dim; d += 64) part += g[d] * v[d];
    return wave_sum(part);
}

// grid (ceil(n_out / 4), batch), four waves, a wave per row
__global__ __launch_bounds__(256) void dmesh_rows_lists(DmArgs a) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int row = blockIdx.x * 4 + wave, s = blockIdx.y;
    if (row >= a.n_out) return;                                    // (wave-uniform; no barriers below)
    const int mb = a.mesh_batch == 1 ? 0 : s;
    const long rid = (long)mb * a.n_out + row;
    float xx, xy, xz;
    load_pt(a.mesh_out, rid, a.sdim, xx, xy, xz);
    const int cnt = a.nbr_cnt[rid];
    const bool scan_all = cnt > a.cap;                             // overflowed list: every key, as pit_posatt_bwd does
    const int total = scan_all ? a.n_in : cnt;
    const int* list = a.nbr_idx + rid * a.cap;
    double dx[3] = {0.0, 0.0, 0.0};
    for (int h = 0; h < a.n_head; ++h) {
        const float c = scale_c(a, h);
        const float4 rs = row_stat(a.rowstat, a.n_head, a.n_out, mb, h, row);
        double A = 0.0, B[3] = {0.0, 0.0, 0.0}, C[3] = {0.0, 0.0, 0.0};
        for (int base = 0; base < total; base += 64) {
            const int e = base + lane;
            const bool valid = e < total;
            const int j = valid ? (scan_all ? e : list[e]) : 0;
            float yx, yy, yz;
            load_pt(a.mesh_in, (long)mb * a.n_in + j, a.sdim, yx, yy, yz);
            const float m = sq_dist3(xx, xy, xz, yx, yy, yz, false, 0.0f);
            const float p = weight(m, c, rs, valid, 1);
            unsigned long long mask = __builtin_amdgcn_ballot_w64(p != 0.0f);
            while (mask) {
                const int src = __builtin_ctzll(mask);
                mask &= mask - 1ull;
                const int jj = __builtin_amdgcn_readlane(j, src);
                const double pp = (double)lane_f(p, src);
                const float d0 = __fsub_rn(lane_f(yx, src), xx);
                const float d1 = __fsub_rn(lane_f(yy, src), xy);
                const float d2 = __fsub_rn(lane_f(yz, src), xz);
                const double gv = (double)wave_dot(a, s, h, row, jj);
                A += pp * gv;
                B[0] += pp * gv * d0; B[1] += pp * gv * d1; B[2] += pp * gv * d2;
                C[0] += pp * d0; C[1] += pp * d1; C[2] += pp * d2;
            }
        }
        if (lane == 0) a.a_ws[((long)s * a.n_head + h) * a.n_out + row] = (float)A;
        const double c2 = 2.0 * (double)c;
#pragma unroll
        for (int k = 0; k < 3; ++k) dx[k] += c2 * (B[k] - A * C[k]);
    }
    if (lane == 0)
        for (int k = 0; k < a.sdim; ++k) a.rows_ws[((long)s * a.n_out + row) * a.sdim + k] = (float)dx[k];
}

// grid (ceil(n_in / 4), batch), four waves, a wave per key
__global__ __launch_bounds__(256) void dmesh_cols_lists(DmArgs a) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int key = blockIdx.x * 4 + wave, s = blockIdx.y;
    if (key >= a.n_in) return;
    const int mb = a.mesh_batch == 1 ? 0 : s;
    float yx, yy, yz;
    load_pt(a.mesh_in, (long)mb * a.n_in + key, a.sdim, yx, yy, yz);
    const int beg = a.rev_ptr[(long)mb * (a.n_in + 1) + key], end = a.rev_ptr[(long)mb * (a.n_in + 1) + key + 1];
    const int* rrow = a.rev_row + (long)mb * a.n_out * a.cap;
    double dy[3] = {0.0, 0.0, 0.0};
    for (int h = 0; h < a.n_head; ++h) {
        const float c = scale_c(a, h);
        const float* arow = a.a_ws + ((long)s * a.n_head + h) * a.n_out;
        double acc[3] = {0.0, 0.0, 0.0};
        auto add = [&](int nrow, float p, float xx, float xy, float xz) {
            unsigned long long mask = __builtin_amdgcn_ballot_w64(p != 0.0f);
            while (mask) {
                const int src = __builtin_ctzll(mask);
                mask &= mask - 1ull;
                const int ii = __builtin_amdgcn_readlane(nrow, src);
                const double pp = (double)lane_f(p, src);
                const float d0 = __fsub_rn(lane_f(xx, src), yx);
                const float d1 = __fsub_rn(lane_f(xy, src), yy);
                const float d2 = __fsub_rn(lane_f(xz, src), yz);
                const double t = pp * ((double)wave_dot(a, s, h, ii, key) - (double)arow[ii]);
                acc[0] += t * d0; acc[1] += t * d1; acc[2] += t * d2;
            }
        };
        for (int base = beg; base < end; base += 64) {
            const int e = base + lane;
            int nrow = (e < end) ? rrow[e] : -1;
            const bool valid = nrow >= 0;                          // -1: slot of a row that overflowed its list
            nrow = valid ? nrow : 0;
            float xx, xy, xz;
            load_pt(a.mesh_out, (long)mb * a.n_out + nrow, a.sdim, xx, xy, xz);
            const float m = sq_dist3(xx, xy, xz, yx, yy, yz, false, 0.0f);
            add(nrow, weight(m, c, row_stat(a.rowstat, a.n_head, a.n_out, mb, h, nrow), valid, 1), xx, xy, xz);
        }
        if (!a.complete) {                                         // rows that overflowed are not in the transposed lists
            for (int base = 0; base < a.n_out; base += 64) {
                int nrow = base + lane;
                const bool valid = nrow < a.n_out && a.nbr_cnt[(long)mb * a.n_out + nrow] > a.cap;
                nrow = valid ? nrow : 0;
                float xx, xy, xz;
                load_pt(a.mesh_out, (long)mb * a.n_out + nrow, a.sdim, xx, xy, xz);
                const float m = sq_dist3(xx, xy, xz, yx, yy, yz, false, 0.0f);
                add(nrow, weight(m, c, row_stat(a.rowstat, a.n_head, a.n_out, mb, h, nrow), valid, 1), xx, xy, xz);
            }
        }
        const double c2 = 2.0 * (double)c;
#pragma unroll
        for (int k = 0; k < 3; ++k) dy[k] += c2 * acc[k];
    }
    if (lane == 0)
        for (int k = 0; k < a.sdim; ++k) a.cols_ws[((long)s * a.n_in + key) * a.sdim + k] = (float)dy[k];
}

// ---- meshes with 4..8 coordinates (space_dim 4..8) ------------------------------------------------------------------
// The forward's distances (pit_common.h sq_dist8t: ATen-CPU's summation order) and the same closed form as above, with a
// wave per row / per key for dense and candidate-list layers alike: a dense layer scans every key / row (as an overflowed
// list does).  Not optimised.
__device__ __forceinline__ float pt8_at(const pt8& p, int k) { return pt_coord(p, k); }
__device__ __forceinline__ double pt8_sel(const double (&v)[8], int k) {
    double r = v[0];
#pragma unroll
    for (int i = 1; i < 8; ++i) r = (k == i) ? v[i] : r;
    return r;
}

// grid (ceil(n_out / 4), batch), four waves, a wave per row
__global__ __launch_bounds__(256) void dmesh_rows_wide(DmArgs a) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int row = blockIdx.x * 4 + wave, s = blockIdx.y;
    if (row >= a.n_out) return;                                    // (wave-uniform; no barriers below)
    const int mb = a.mesh_batch == 1 ? 0 : s;
    const long rid = (long)mb * a.n_out + row;
    const pt8 x = load_pt8(a.mesh_out, rid, a.sdim, a.sdim);
    const bool sparse = a.nbr_idx != nullptr;
    const int cnt = sparse ? a.nbr_cnt[rid] : a.n_in;
    const bool scan_all = !sparse || cnt > a.cap;
    const int total = scan_all ? a.n_in : cnt;
    const int* list = sparse ? a.nbr_idx + rid * a.cap : nullptr;
    const int masked = sparse ? 1 : a.masked;
    double dx[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int h = 0; h < a.n_head; ++h) {
        const float c = scale_c(a, h);
        const float4 rs = row_stat(a.rowstat, a.n_head, a.n_out, mb, h, row);
        double A = 0.0, B[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, C[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        for (int base = 0; base < total; base += 64) {
            const int e = base + lane;
            const bool valid = e < total;
            const int j = valid ? (scan_all ? e : list[e]) : 0;
            const pt8 y = load_pt8(a.mesh_in, (long)mb * a.n_in + j, a.sdim, a.sdim);
            const float p = weight(sq_dist8t<false>(x, y, a.sdim, 0.0f), c, rs, valid, masked);
            unsigned long long mask = __builtin_amdgcn_ballot_w64(p != 0.0f);
            while (mask) {
                const int src = __builtin_ctzll(mask);
                mask &= mask - 1ull;
                const int jj = __builtin_amdgcn_readlane(j, src);
                const double pp = (double)lane_f(p, src);
                const double gv = (double)wave_dot(a, s, h, row, jj);
                A += pp * gv;
#pragma unroll
                for (int k = 0; k < 8; ++k) {
                    const float yk = lane_f(pt8_at(y, k), src);
                    const float d = __fsub_rn(yk, pt8_at(x, k));
                    B[k] += pp * gv * d;
                    C[k] += pp * d;
                }
            }
        }
        if (lane == 0) a.a_ws[((long)s * a.n_head + h) * a.n_out + row] = (float)A;
        const double c2 = 2.0 * (double)c;
#pragma unroll
        for (int k = 0; k < 8; ++k) dx[k] += c2 * (B[k] - A * C[k]);
    }
    if (lane == 0)
        for (int k = 0; k < a.sdim; ++k) a.rows_ws[((long)s * a.n_out + row) * a.sdim + k] = (float)pt8_sel(dx, k);
}

// grid (ceil(n_in / 4), batch), four waves, a wave per key
__global__ __launch_bounds__(256) void dmesh_cols_wide(DmArgs a) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int key = blockIdx.x * 4 + wave, s = blockIdx.y;
    if (key >= a.n_in) return;
    const int mb = a.mesh_batch == 1 ? 0 : s;
    const pt8 y = load_pt8(a.mesh_in, (long)mb * a.n_in + key, a.sdim, a.sdim);
    const bool sparse = a.nbr_idx != nullptr;
    const int masked = sparse ? 1 : a.masked;
    double dy[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int h = 0; h < a.n_head; ++h) {
        const float c = scale_c(a, h);
        const float* arow = a.a_ws + ((long)s * a.n_head + h) * a.n_out;
        double acc[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        auto add = [&](int nrow, bool valid) {
            const pt8 x = load_pt8(a.mesh_out, (long)mb * a.n_out + nrow, a.sdim, a.sdim);
            const float p = weight(sq_dist8t<false>(x, y, a.sdim, 0.0f), c, row_stat(a.rowstat, a.n_head, a.n_out, mb, h, nrow), valid, masked);
            unsigned long long mask = __builtin_amdgcn_ballot_w64(p != 0.0f);
            while (mask) {
                const int src = __builtin_ctzll(mask);
                mask &= mask - 1ull;
                const int ii = __builtin_amdgcn_readlane(nrow, src);
                const double pp = (double)lane_f(p, src);
                const double t = pp * ((double)wave_dot(a, s, h, ii, key) - (double)arow[ii]);
#pragma unroll
                for (int k = 0; k < 8; ++k) {
                    const float xk = lane_f(pt8_at(x, k), src);
                    acc[k] += t * __fsub_rn(xk, pt8_at(y, k));
                }
            }
        };
        if (sparse) {
            const int beg = a.rev_ptr[(long)mb * (a.n_in + 1) + key], end = a.rev_ptr[(long)mb * (a.n_in + 1) + key + 1];
            const int* rrow = a.rev_row + (long)mb * a.n_out * a.cap;
            for (int base = beg; base < end; base += 64) {
                const int e = base + lane;
                const int nrow = (e < end) ? rrow[e] : -1;     // -1: slot of a row that overflowed its list
                add(nrow >= 0 ? nrow : 0, nrow >= 0);
            }
        }
        if (!sparse || !a.complete) {                          // dense layers: every row; lists: the rows that overflowed
            for (int base = 0; base < a.n_out; base += 64) {
                const int nrow = base + lane;
                const bool valid = nrow < a.n_out && (!sparse || a.nbr_cnt[(long)mb * a.n_out + nrow] > a.cap);
                add(valid ? nrow : 0, valid);
            }
        }
        const double c2 = 2.0 * (double)c;
#pragma unroll
        for (int k = 0; k < 8; ++k) dy[k] += c2 * acc[k];
    }
    if (lane == 0)
        for (int k = 0; k < a.sdim; ++k) a.cols_ws[((long)s * a.n_in + key) * a.sdim + k] = (float)pt8_sel(dy, k);
}

// ---- fixed-order reduction over the samples --------------------------------------------------------------------------
// out (mesh_batch, n, sdim) = [out +] sum over the samples that share the mesh of ws (batch, n, sdim), in sample order
__global__ __launch_bounds__(256) void dmesh_reduce(const float* __restrict__ ws, int batch, int mesh_batch, long per,
                                                    float* __restrict__ out, int accumulate) {
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (long)mesh_batch * per) return;
    float v;
    if (mesh_batch == 1) {
        v = 0.0f;
        for (int s = 0; s < batch; ++s) v += ws[(long)s * per + idx];
    } else {
        v = ws[idx];
    }
    out[idx] = accumulate ? out[idx] + v : v;
}

long ws_floats(int batch, int n_out, int n_in, int space_dim, int n_head) {
    return (long)batch * n_head * n_out + (long)batch * n_out * space_dim + (long)batch * n_in * space_dim;
}

}  // namespace

extern "C" long pit_posatt_dmesh_workspace(int mesh_batch, int n_out, int n_in, int space_dim, int batch, int n_head) {
    (void)mesh_batch;
    if (n_out <= 0 || n_in <= 0 || space_dim < 1 || space_dim > PIT_MAX_SPACE_DIM || batch <= 0 || n_head <= 0) return 0;
    return ws_floats(batch, n_out, n_in, space_dim, n_head) * 4;
}

extern "C" int pit_posatt_dmesh(const float* mesh_out, const float* mesh_in, int mesh_batch, int n_out, int n_in,
                                int space_dim, int metric, float period,
                                const float* values, int batch, int dim, long ld_values, long values_bstride,
                                const float* head, int n_head, int head_is_scale, const float* scale,
                                const float* rowstat, int masked,
                                const float* d_out, long ld_dout, long dout_bstride, int out_col0,
                                const int* nbr_idx, const int* nbr_cnt, int nbr_cap, int nbr_complete,
                                const int* rev_ptr, const int* rev_row,
                                float* d_mesh_out, float* d_mesh_in, int accumulate, void* workspace, void* stream) {
    (void)period;
    if (metric != PIT_METRIC_EUCLID) {
        if (metric < PIT_METRIC_EUCLID || metric > PIT_METRIC_PERIODIC2D) return PIT_ERR_METRIC;
        return PIT_ERR_UNSUPPORTED;                                 // periodic metrics: the period and the tie rules too
    }
    if (!mesh_out || !mesh_in || !values || !head || !rowstat || !d_out || !workspace) return PIT_ERR_NULL;
    if (mesh_batch <= 0 || n_out <= 0 || n_in <= 0 || batch <= 0 || dim <= 0 || n_head <= 0) return PIT_ERR_SIZE;
    if (space_dim < 1 || space_dim > PIT_MAX_SPACE_DIM || (mesh_batch != 1 && mesh_batch != batch) || out_col0 < 0) return PIT_ERR_SIZE;
    if (batch > 65535 || n_head > 65535) return PIT_ERR_UNSUPPORTED;
    if (ld_values < dim || ld_dout < out_col0 + (long)n_head * dim || values_bstride < 0 || dout_bstride < 0) return PIT_ERR_SIZE;
    const bool sparse = masked && nbr_idx && nbr_cnt;
    if (sparse && nbr_cap <= 0) return PIT_ERR_SIZE;
    if (sparse && d_mesh_in && !(rev_ptr && rev_row)) return PIT_ERR_NULL;
    if (!d_mesh_out && !d_mesh_in) return 0;
    DmArgs a = DmArgs();
    a.mesh_out = mesh_out; a.mesh_in = mesh_in; a.mesh_batch = mesh_batch; a.n_out = n_out; a.n_in = n_in; a.sdim = space_dim;
    a.values = values; a.batch = batch; a.dim = dim; a.ld_values = ld_values; a.values_bstride = values_bstride;
    a.head = head; a.scale = scale; a.n_head = n_head; a.head_is_scale = head_is_scale;
    a.rowstat = rowstat; a.masked = masked ? 1 : 0;
    a.d_out = d_out; a.ld_dout = ld_dout; a.dout_bstride = dout_bstride; a.out_col0 = out_col0;
    a.nbr_idx = nbr_idx; a.nbr_cnt = nbr_cnt; a.cap = nbr_cap; a.complete = nbr_complete ? 1 : 0;
    a.rev_ptr = rev_ptr; a.rev_row = rev_row;
    {
        const unsigned long long vb = ((unsigned long long)(batch - 1) * values_bstride + (unsigned long long)(n_in - 1) * ld_values + dim) * 4ull;
        const unsigned long long db = ((unsigned long long)(batch - 1) * dout_bstride + (unsigned long long)(n_out - 1) * ld_dout +
                                       out_col0 + (unsigned long long)n_head * dim) * 4ull;
        if (vb > PIT_MAX_BUFFER_BYTES || db > PIT_MAX_BUFFER_BYTES) return PIT_ERR_UNSUPPORTED;
        a.values_bytes = (unsigned)vb;
        a.dout_bytes = (unsigned)db;
    }
    float* ws = static_cast<float*>(workspace);
    a.a_ws = ws;
    a.rows_ws = ws + (long)batch * n_head * n_out;
    a.cols_ws = a.rows_ws + (long)batch * n_out * space_dim;
    hipStream_t st = (hipStream_t)stream;
    // rows pass: d mesh_out and the a_i the cols pass needs
    if (!sparse) { a.nbr_idx = nullptr; a.nbr_cnt = nullptr; }
    if (space_dim > 3) hipLaunchKernelGGL(dmesh_rows_wide, dim3((unsigned)((n_out + 3) / 4), (unsigned)batch), dim3(256), 0, st, a);
    else if (sparse) hipLaunchKernelGGL(dmesh_rows_lists, dim3((unsigned)((n_out + 3) / 4), (unsigned)batch), dim3(256), 0, st, a);
    else hipLaunchKernelGGL(dmesh_rows_dense, dim3((unsigned)((n_out + 31) / 32), (unsigned)batch), dim3(64), 0, st, a);
    PIT_CHECK_LAUNCH();
    if (d_mesh_out) {
        const long per = (long)n_out * space_dim;
        hipLaunchKernelGGL(dmesh_reduce, dim3((unsigned)((mesh_batch * per + 255) / 256)), dim3(256), 0, st,
                           (const float*)a.rows_ws, batch, mesh_batch, per, d_mesh_out, accumulate ? 1 : 0);
        PIT_CHECK_LAUNCH();
    }
    if (d_mesh_in) {
        if (space_dim > 3) hipLaunchKernelGGL(dmesh_cols_wide, dim3((unsigned)((n_in + 3) / 4), (unsigned)batch), dim3(256), 0, st, a);
        else if (sparse) hipLaunchKernelGGL(dmesh_cols_lists, dim3((unsigned)((n_in + 3) / 4), (unsigned)batch), dim3(256), 0, st, a);
        else hipLaunchKernelGGL(dmesh_cols_dense, dim3((unsigned)((n_in + 31) / 32), (unsigned)batch), dim3(64), 0, st, a);
        PIT_CHECK_LAUNCH();
        // self attention (d_mesh_in == d_mesh_out): the key terms add onto the row terms just written
        const int acc_in = (accumulate || (d_mesh_in == d_mesh_out)) ? 1 : 0;
        const long per = (long)n_in * space_dim;
        hipLaunchKernelGGL(dmesh_reduce, dim3((unsigned)((mesh_batch * per + 255) / 256)), dim3(256), 0, st,
                           (const float*)a.cols_ws, batch, mesh_batch, per, d_mesh_in, acc_in);
        PIT_CHECK_LAUNCH();
    }
    return 0;
}
