// Ragged batches of per-sample point clouds: padded tensors plus per-sample lengths that live on the DEVICE.
//
// Sample s of a (batch, n, ...) tensor holds len[s] real points followed by padding.  The kernels below read the
// lengths themselves (no host synchronisation: one captured hipGraph serves every mix of sizes up to the padded
// width) and follow three rules, so that sample s comes out as the reference computes it for that cloud alone:
//   - keys j >= len_in[s] are never read (neither their coordinates nor their value rows): padding may hold anything;
//   - rows i >= len_out[s] are written as zeros (forward), their d_out is never read (backward);
//   - d_values of keys j >= len_in[s] is written as zero.
// Lengths are clamped into [1, padded width] where they are read, so a bad length cannot address outside a buffer.
//
// These are kernels of their own (nothing in pit_select.hip / pit_posatt.hip changes): a streaming selection pass whose
// quantile rank is formed per sample, and ONE tiled attention kernel in three modes.  A workgroup owns RT = 16 "owner"
// items of one sample (rows for the forward and d(scale), keys for d(values)) and up to 256 value columns; the
// contracted axis is walked in tiles of KT = 64: all 256 threads form the 16 x 64 weights of the tile
// (exp(S_min - S)[S <= T], the expressions of pit_posatt.hip) into LDS, then every wave contracts them against its 64
// columns with plain FMAs, 16 accumulators per lane.  A tile's partial sums are fp32, tiles are added in fp64 in a
// fixed order: the same bits on every run (d(scale) meets in the fp64 slots of pit_posatt_bwd's workspace).
// Tiles and workgroups beyond the sample's length exit early and the contracted loop ends at the length.
//
// A mesh SHARED by the whole batch against per-sample clouds (the *_strided entries, ABI 28): every kernel takes a sample stride
// per mesh - 0 reads the one (n, space_dim) mesh in place for every sample, no expanded copy exists - and a length pointer that may
// be NULL (every sample has the full width: the shared side has no padding).  Both are kernel arguments, so the branch is uniform
// and the stride-0 address is the same for every sample; statistics, lists, rowstat, values and d(values) stay per sample.
#include "pit_layer.h"

namespace {

constexpr int RT = 16;     // owner items per workgroup
constexpr int KT = 64;     // contracted items per tile

__device__ __forceinline__ float4 load_pt3(const float* p, int sdim) {
    float4 v;
    v.x = p[0];
    v.y = sdim > 1 ? p[1] : 0.0f;
    v.z = sdim > 2 ? p[2] : 0.0f;
    v.w = 0.0f;
    return v;
}
__device__ __forceinline__ float dist3(const float4& o, const float4& i) {
    return sq_dist3(o.x, o.y, o.z, i.x, i.y, i.z, false, 0.0f);
}

// ---- selection: order statistics over the first len_in[s] keys of a row; one workgroup per row ----------------------
struct RagSelectArgs {
    const float* mesh_out; const float* mesh_in;
    long mo_stride, mi_stride;   // floats between two samples' meshes; 0 = one mesh shared by the batch (read in place)
    const int* len_out; const int* len_in;
    float* stats;        // [3][batch * n_out]
    float* rank_w;       // [batch]: fractional part of the sample's quantile rank
    int batch, n_out, n_in, sdim;
    float q;             // fl32(locality)
    int need_kth;
};

__global__ __launch_bounds__(256) void ragged_select_kernel(RagSelectArgs a) {
    __shared__ int s_cnt[4];
    __shared__ uint32_t s_min[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long rows = (long)a.batch * a.n_out;
    const long row = blockIdx.x;
    const int s = (int)(row / a.n_out), i = (int)(row - (long)s * a.n_out);
    const int lo = clamp_len(a.len_out, s, a.n_out), li = clamp_len(a.len_in, s, a.n_in);
    // torch.quantile's rank in ATen's fp32 arithmetic, for THIS sample's key count (ops.quantile_rank)
    float w;
    const int k = sample_rank(a.q, li, w);               // (pit_layer.h)
    if (i == 0 && threadIdx.x == 0) a.rank_w[s] = w;
    if (i >= lo) {                                        // padded row: defined statistics, nothing is read
        if (threadIdx.x == 0) { a.stats[row] = 0.0f; a.stats[rows + row] = 0.0f; a.stats[2 * rows + row] = 0.0f; }
        return;
    }
    const float4 xo = load_pt3(a.mesh_out + (long)s * a.mo_stride + (long)i * a.sdim, a.sdim);
    const float* pin = a.mesh_in + (long)s * a.mi_stride;
    auto key_at = [&](int j) -> uint32_t { return __float_as_uint(dist3(xo, load_pt3(pin + (long)j * a.sdim, a.sdim))); };
    auto block_count = [&](uint32_t cand, bool inclusive) -> int {
        int c = 0;
        for (int j = threadIdx.x; j < li; j += 256) {
            const uint32_t kk = key_at(j);
            c += inclusive ? (kk <= cand) : (kk < cand);
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o);
        __syncthreads();
        if (lane == 0) s_cnt[wave] = c;
        __syncthreads();
        return s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3];
    };
    auto block_min_above = [&](uint32_t bound, bool strictly_above) -> uint32_t {
        uint32_t m = 0xFFFFFFFFu;
        for (int j = threadIdx.x; j < li; j += 256) {
            const uint32_t kk = key_at(j);
            if (!strictly_above || kk > bound) m = min(m, kk);
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) m = min(m, (uint32_t)__shfl_xor((int)m, o));
        __syncthreads();
        if (lane == 0) s_min[wave] = m;
        __syncthreads();
        return min(min(s_min[0], s_min[1]), min(s_min[2], s_min[3]));
    };
    const uint32_t kmin = block_min_above(0, false);
    uint32_t vk = kmin, vk1 = kmin;
    if (a.need_kth) {
        uint32_t prefix = 0;
        for (int bit = 30; bit >= 0; --bit) {             // MSB-first bitwise search (pit_select.hip)
            const uint32_t cand = prefix | (1u << bit);
            if (block_count(cand, false) <= k) prefix = cand;
        }
        vk = prefix;
        const int cnt_le = block_count(vk, true);
        const uint32_t next = block_min_above(vk, true);
        vk1 = (cnt_le >= k + 2 || k + 1 > li - 1) ? vk : next;
    }
    if (threadIdx.x == 0) {
        a.stats[row] = __uint_as_float(vk);
        a.stats[rows + row] = __uint_as_float(vk1);
        a.stats[2 * rows + row] = __uint_as_float(kmin);
    }
}

// ---- attention ------------------------------------------------------------------------------------------------------
struct RagArgs : LayerIO {
    const float* mesh_out; const float* mesh_in;
    long mo_stride, mi_stride;   // as in RagSelectArgs
    const int* len_out; const int* len_in;
    int batch, n_out, n_in, sdim;
    const float* rank_w;
};

// the tile's contraction for one wave: acc[r] += w[t][r] * x[t][col] over the tile's first `cnt` items; x rows ldx apart.
// Items whose 16 weights are all zero (masked layers: most of them) are skipped - a wave-uniform branch.
__device__ __forceinline__ void tile_fma(const float (*w)[RT], const float* __restrict__ x, long ldx, int cnt, bool cvalid,
                                         bool skip_zero, float (&acc)[RT]) {
    for (int t = 0; t < cnt; ++t) {
        const float4 w0 = *reinterpret_cast<const float4*>(&w[t][0]);
        const float4 w1 = *reinterpret_cast<const float4*>(&w[t][4]);
        const float4 w2 = *reinterpret_cast<const float4*>(&w[t][8]);
        const float4 w3 = *reinterpret_cast<const float4*>(&w[t][12]);
        if (skip_zero) {
            const float any = fabsf(w0.x) + fabsf(w0.y) + fabsf(w0.z) + fabsf(w0.w) + fabsf(w1.x) + fabsf(w1.y) + fabsf(w1.z) + fabsf(w1.w) +
                              fabsf(w2.x) + fabsf(w2.y) + fabsf(w2.z) + fabsf(w2.w) + fabsf(w3.x) + fabsf(w3.y) + fabsf(w3.z) + fabsf(w3.w);
            if (__builtin_amdgcn_readfirstlane(__float_as_int(any)) == 0) continue;
        }
        const float v = cvalid ? x[(long)t * ldx] : 0.0f;
        acc[0] += w0.x * v;  acc[1] += w0.y * v;  acc[2] += w0.z * v;  acc[3] += w0.w * v;
        acc[4] += w1.x * v;  acc[5] += w1.y * v;  acc[6] += w1.z * v;  acc[7] += w1.w * v;
        acc[8] += w2.x * v;  acc[9] += w2.y * v;  acc[10] += w2.z * v; acc[11] += w2.w * v;
        acc[12] += w3.x * v; acc[13] += w3.y * v; acc[14] += w3.z * v; acc[15] += w3.w * v;
    }
}

// MODE 0: forward.  MODE 1: d(scale).  grid (row tiles, batch, n_head * colgroups)
template <int MODE>
__global__ __launch_bounds__(256) void ragged_rows_kernel(RagArgs a) {
    __shared__ __attribute__((aligned(16))) float s_w[KT][RT];
    __shared__ float4 s_xo[RT];
    __shared__ float4 s_rs[RT];          // {T, S_min, 1/rowsum, mbar} of the tile's rows
    __shared__ float s_sum[RT][RT + 1], s_q[RT][RT + 1];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int s = blockIdx.y, r0 = blockIdx.x * RT;
    const int h = blockIdx.z / a.colgroups, cg = blockIdx.z - h * a.colgroups;
    const int lo = clamp_len(a.len_out, s, a.n_out), li = clamp_len(a.len_in, s, a.n_in);
    const int col = cg * 256 + wave * 64 + lane;
    const bool cvalid = col < a.dim;
    const int rows_here = min(RT, a.n_out - r0);          // rows of this tile inside the padded width
    const int live = max(0, min(RT, lo - r0));            // ... inside the sample
    const float c = head_c(a, h);

    if (MODE == 0) {
        if (a.copy_inputs && h == 0 && cvalid)            // torch.cat((inputs, conv), -1): the copied columns as they are
            for (int r = 0; r < rows_here; ++r)
                a.out[(long)s * a.out_bstride + (long)(r0 + r) * a.ld_out + col] =
                    a.values[(long)s * a.values_bstride + (long)(r0 + r) * a.ld_values + col];
        if (cvalid)                                       // padded rows: zeros in every head column
            for (int r = live; r < rows_here; ++r)
                a.out[(long)s * a.out_bstride + (long)(r0 + r) * a.ld_out + a.out_col0 + (long)h * a.dim + col] = 0.0f;
        if (cg == 0 && tid >= live && tid < rows_here)
            *reinterpret_cast<float4*>(a.rowstat + (((long)s * a.n_head + h) * a.n_out + r0 + tid) * 4) = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (s == 0 && blockIdx.x == 0 && cg == 0 && tid == 0 && a.scale_out) a.scale_out[h] = c;
    }
    if (live == 0) return;                                // the whole tile is padding

    const long rows_total = (long)a.batch * a.n_out;
    if (tid < RT) {
        const int r = min(tid, live - 1);
        const long row = (long)s * a.n_out + r0 + r;
        s_xo[tid] = load_pt3(a.mesh_out + (long)s * a.mo_stride + (long)(r0 + r) * a.sdim, a.sdim);
        float4 st;
        if (MODE == 0) {
            st.x = a.masked ? quantile_lerp(__fmul_rn(c, a.stats[row]), __fmul_rn(c, a.stats[rows_total + row]), a.rank_w[s])
                            : __builtin_inff();
            st.y = __fmul_rn(c, a.stats[2 * rows_total + row]);
            st.z = 0.0f; st.w = 0.0f;
        } else {
            st = row_stat(a.rowstat, a.n_head, a.n_out, s, h, r0 + r);
        }
        s_rs[tid] = st;
    }
    __syncthreads();
    const int wr = tid & 15, wk = tid >> 4;               // this thread's row and its keys wk, wk + 16, ... of a tile
    const float4 xo = s_xo[wr];
    const float4 rs = s_rs[wr];
    const bool rlive = wr < live;
    const float* pin = a.mesh_in + (long)s * a.mi_stride;
    const float* vals = a.values + (long)s * a.values_bstride + col;
    float rsum = 0.0f, qsum = 0.0f;
    double tot[RT];
#pragma unroll
    for (int r = 0; r < RT; ++r) tot[r] = 0.0;

    for (int j0 = 0; j0 < li; j0 += KT) {
        const int cnt = min(KT, li - j0);
#pragma unroll
        for (int u = 0; u < KT / 16; ++u) {
            const int t = wk + 16 * u;
            float p = 0.0f;
            if (t < cnt && rlive) {
                const float m = dist3(xo, load_pt3(pin + (long)(j0 + t) * a.sdim, a.sdim));
                const float sv = __fmul_rn(m, c);
                if (sv <= rs.x) {
                    p = __expf(rs.y - sv);
                    if (MODE == 0) { rsum += p; qsum += p * m; }
                    else p = p * (m - rs.w) * rs.z;
                }
            }
            s_w[t][wr] = p;
        }
        __syncthreads();
        float acc[RT];
#pragma unroll
        for (int r = 0; r < RT; ++r) acc[r] = 0.0f;
        tile_fma(s_w, vals + (long)j0 * a.ld_values, a.ld_values, cnt, cvalid, a.masked != 0, acc);
#pragma unroll
        for (int r = 0; r < RT; ++r) tot[r] += (double)acc[r];
        __syncthreads();
    }

    if (MODE == 1) {
        double part = 0.0;
        if (cvalid) {
            const float* go = a.d_out + (long)s * a.dout_bstride + (long)r0 * a.ld_dout + a.out_col0 + (long)h * a.dim + col;
#pragma unroll
            for (int r = 0; r < RT; ++r)
                if (r < live) part += tot[r] * (double)go[(long)r * a.ld_dout];
        }
        part = wave_sum_d(part);
        const int slot = (int)((blockIdx.x + 131u * blockIdx.y + 977u * (cg * 4 + wave)) & (PIT_DSCALE_SLOTS - 1));
        if (lane == 0) atomicAdd(a.dscale_acc + (long)h * PIT_DSCALE_SLOTS + slot, -part);
        return;
    }
    s_sum[wr][wk] = rsum;
    s_q[wr][wk] = qsum;
    __syncthreads();
    if (tid < RT) {
        float rsm = 0.0f, qs = 0.0f;
        for (int u = 0; u < 16; ++u) { rsm += s_sum[tid][u]; qs += s_q[tid][u]; }
        const float inv = rsm > 0.0f ? 1.0f / rsm : 0.0f;
        float4 st = s_rs[tid];
        st.z = inv; st.w = qs * inv;
        s_rs[tid] = st;
        if (cg == 0 && tid < live)
            *reinterpret_cast<float4*>(a.rowstat + (((long)s * a.n_head + h) * a.n_out + r0 + tid) * 4) = st;
    }
    __syncthreads();
    if (cvalid) {
        float* o = a.out + (long)s * a.out_bstride + (long)r0 * a.ld_out + a.out_col0 + (long)h * a.dim + col;
#pragma unroll
        for (int r = 0; r < RT; ++r)
            if (r < live) o[(long)r * a.ld_out] = (float)tot[r] * s_rs[r].z;
    }
}

// d(values): a workgroup owns 16 keys; d_values[s, j, :] = (residual) + sum_h sum_n P_h[n, j] d_out[s, n, head h], rows in
// ascending order.  grid (key tiles, batch, colgroups)
__global__ __launch_bounds__(256) void ragged_cols_kernel(RagArgs a) {
    __shared__ __attribute__((aligned(16))) float s_w[KT][RT];
    __shared__ float4 s_xi[RT];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int s = blockIdx.y, k0 = blockIdx.x * RT, cg = blockIdx.z;
    const int lo = clamp_len(a.len_out, s, a.n_out), li = clamp_len(a.len_in, s, a.n_in);
    const int col = cg * 256 + wave * 64 + lane;
    const bool cvalid = col < a.dim;
    const int keys_here = min(RT, a.n_in - k0);
    const int live = max(0, min(RT, li - k0));
    float* dv = a.d_values + (long)s * a.dvalues_bstride + (long)k0 * a.ld_dvalues + col;
    if (cvalid)
        for (int r = live; r < keys_here; ++r) dv[(long)r * a.ld_dvalues] = 0.0f;       // padded keys: zero, residual included
    if (live == 0) return;
    if (tid < RT) s_xi[tid] = load_pt3(a.mesh_in + (long)s * a.mi_stride + (long)(k0 + min(tid, live - 1)) * a.sdim, a.sdim);
    __syncthreads();
    const int wr = tid & 15, wk = tid >> 4;
    const float4 xi = s_xi[wr];
    const bool klive = wr < live;
    double tot[RT];
#pragma unroll
    for (int r = 0; r < RT; ++r) tot[r] = 0.0;
    for (int h = 0; h < a.n_head; ++h) {
        const float c = head_c(a, h);
        const float* go = a.d_out + (long)s * a.dout_bstride + a.out_col0 + (long)h * a.dim + col;
        for (int n0 = 0; n0 < lo; n0 += KT) {
            const int cnt = min(KT, lo - n0);
#pragma unroll
            for (int u = 0; u < KT / 16; ++u) {
                const int t = wk + 16 * u;
                float p = 0.0f;
                if (t < cnt && klive) {
                    const float4 rs = *reinterpret_cast<const float4*>(a.rowstat + (((long)s * a.n_head + h) * a.n_out + n0 + t) * 4);
                    const float m = dist3(load_pt3(a.mesh_out + (long)s * a.mo_stride + (long)(n0 + t) * a.sdim, a.sdim), xi);
                    const float sv = __fmul_rn(m, c);
                    if (sv <= rs.x) p = __expf(rs.y - sv) * rs.z;
                }
                s_w[t][wr] = p;
            }
            __syncthreads();
            float acc[RT];
#pragma unroll
            for (int r = 0; r < RT; ++r) acc[r] = 0.0f;
            tile_fma(s_w, go + (long)n0 * a.ld_dout, a.ld_dout, cnt, cvalid, a.masked != 0, acc);
#pragma unroll
            for (int r = 0; r < RT; ++r) tot[r] += (double)acc[r];
            __syncthreads();
        }
    }
    if (cvalid) {
        const float* res = a.d_out + (long)s * a.dout_bstride + (long)k0 * a.ld_dout + col;   // self attention: n_out == n_in, lo == li
#pragma unroll
        for (int r = 0; r < RT; ++r)
            if (r < live) dv[(long)r * a.ld_dvalues] = (float)tot[r] + (a.add_residual ? res[(long)r * a.ld_dout] : 0.0f);
    }
}

// ---- candidate lists (masked layers with a small locality) ----------------------------------------------------------------
// The lists of pit_neighbors_fwd over the first len_in[s] keys: keys with m <= m_(k+1) * (1 + 2^-21), ascending; the capacity is
// chosen on the host from the PADDED width, nbr_cnt holds the true count and a row with count > cap is scanned densely by its
// consumers (the existing convention).  Padded rows get count 0, so the transposed lists (pit_lists_transpose) hold no padded
// row, and padded keys - never listed - have empty ranges.
__global__ __launch_bounds__(256) void ragged_neighbors_kernel(RagSelectArgs a, int cap, int* __restrict__ nbr_idx, int* __restrict__ nbr_cnt) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long rows = (long)a.batch * a.n_out;
    const long row = (long)blockIdx.x * 4 + wave;
    if (row >= rows) return;
    const int s = (int)(row / a.n_out), i = (int)(row - (long)s * a.n_out);
    const int lo = clamp_len(a.len_out, s, a.n_out), li = clamp_len(a.len_in, s, a.n_in);
    if (i >= lo) { if (lane == 0) nbr_cnt[row] = 0; return; }
    const float4 xo = load_pt3(a.mesh_out + (long)s * a.mo_stride + (long)i * a.sdim, a.sdim);
    const float* pin = a.mesh_in + (long)s * a.mi_stride;
    const float bound = a.stats[rows + row] * 1.00000047683715820312f;
    int total = 0;
    int* out = nbr_idx + row * cap;
    for (int j0 = 0; j0 < li; j0 += 64) {
        const int j = j0 + lane;
        const bool in = j < li && dist3(xo, load_pt3(pin + (long)min(j, li - 1) * a.sdim, a.sdim)) <= bound;
        const unsigned long long mask = __builtin_amdgcn_ballot_w64(in);
        const int pos = total + __popcll(mask & ((1ull << lane) - 1ull));
        if (in && pos < cap) out[pos] = j;
        total += __popcll(mask);
    }
    if (lane == 0) nbr_cnt[row] = total;
}

struct RagLists { const int* idx; const int* cnt; int cap; const int* rev_ptr; const int* rev_row; };
constexpr int LQ = 4;      // 64-column groups per wave of the list kernels

// forward (MODE 0) and d(scale) (MODE 1) on the lists: one wave per row, lane = value column; the kept candidates are walked in
// list order (ascending key), so every sum has a fixed order.  grid (rows / 4, n_head, colgroups)
template <int MODE>
__global__ __launch_bounds__(256) void ragged_list_rows_kernel(RagArgs a, RagLists L) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long rows_total = (long)a.batch * a.n_out;
    const long row = (long)blockIdx.x * 4 + wave;
    if (row >= rows_total) return;
    const int s = (int)(row / a.n_out), n = (int)(row - (long)s * a.n_out);
    const int h = blockIdx.y, cg = blockIdx.z;
    const int lo = clamp_len(a.len_out, s, a.n_out), li = clamp_len(a.len_in, s, a.n_in);
    const float c = head_c(a, h);
    int col[LQ]; bool cv[LQ];
#pragma unroll
    for (int q = 0; q < LQ; ++q) { col[q] = cg * 64 * LQ + q * 64 + lane; cv[q] = col[q] < a.dim; }
    float* rsp = a.rowstat + (((long)s * a.n_head + h) * a.n_out + n) * 4;
    if (MODE == 0) {
        if (row == 0 && cg == 0 && lane == 0 && a.scale_out) a.scale_out[h] = c;
        if (a.copy_inputs && h == 0)
#pragma unroll
            for (int q = 0; q < LQ; ++q)
                if (cv[q]) a.out[(long)s * a.out_bstride + (long)n * a.ld_out + col[q]] = a.values[(long)s * a.values_bstride + (long)n * a.ld_values + col[q]];
    }
    if (n >= lo) {
        if (MODE == 0) {
#pragma unroll
            for (int q = 0; q < LQ; ++q)
                if (cv[q]) a.out[(long)s * a.out_bstride + (long)n * a.ld_out + a.out_col0 + (long)h * a.dim + col[q]] = 0.0f;
            if (cg == 0 && lane == 0) *reinterpret_cast<float4*>(rsp) = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        }
        return;
    }
    float T, smin, inv = 0.0f, mbar = 0.0f;
    if (MODE == 0) {
        T = quantile_lerp(__fmul_rn(c, a.stats[row]), __fmul_rn(c, a.stats[rows_total + row]), a.rank_w[s]);
        smin = __fmul_rn(c, a.stats[2 * rows_total + row]);
    } else {
        const float4 rs = *reinterpret_cast<const float4*>(rsp);
        T = rs.x; smin = rs.y; inv = rs.z; mbar = rs.w;
    }
    const float4 xo = load_pt3(a.mesh_out + (long)s * a.mo_stride + (long)n * a.sdim, a.sdim);
    const float* pin = a.mesh_in + (long)s * a.mi_stride;
    const float* vals = a.values + (long)s * a.values_bstride;
    const int* list = L.idx + row * L.cap;
    const int cnt = L.cnt[row];
    const bool scan_all = cnt > L.cap;                    // overflowed list: all keys of the sample
    const int total = scan_all ? li : cnt;
    float acc[LQ] = {0.0f, 0.0f, 0.0f, 0.0f};
    float rsum = 0.0f, qsum = 0.0f;
    for (int base = 0; base < total; base += 64) {
        const int i = base + lane;
        const bool valid = i < total;
        const int j = valid ? (scan_all ? i : list[i]) : 0;
        const float m = dist3(xo, load_pt3(pin + (long)j * a.sdim, a.sdim));
        const float sv = __fmul_rn(m, c);
        const bool keep = valid && sv <= T;
        float p = keep ? __expf(smin - sv) : 0.0f;
        if (MODE == 0) { rsum += p; qsum += p * m; }
        else p = p * (m - mbar) * inv;
        unsigned long long mask = __builtin_amdgcn_ballot_w64(keep);
        while (mask) {
            const int src = __builtin_ctzll(mask);
            mask &= mask - 1ull;
            const int jj = __builtin_amdgcn_readlane(j, src);
            const float pv = lane_f(p, src);
            const float* vr = vals + (long)jj * a.ld_values;
#pragma unroll
            for (int q = 0; q < LQ; ++q) acc[q] += pv * (cv[q] ? vr[col[q]] : 0.0f);
        }
    }
    if (MODE == 1) {
        const float* go = a.d_out + (long)s * a.dout_bstride + (long)n * a.ld_dout + a.out_col0 + (long)h * a.dim;
        double part = 0.0;
#pragma unroll
        for (int q = 0; q < LQ; ++q) part += cv[q] ? (double)acc[q] * (double)go[col[q]] : 0.0;
        part = wave_sum_d(part);
        const int slot = (int)((blockIdx.x + 131u * cg + 977u * wave) & (PIT_DSCALE_SLOTS - 1));
        if (lane == 0) atomicAdd(a.dscale_acc + (long)h * PIT_DSCALE_SLOTS + slot, -part);
        return;
    }
    const float rs = wave_sum(rsum), qs = wave_sum(qsum);
    inv = rs > 0.0f ? 1.0f / rs : 0.0f;
#pragma unroll
    for (int q = 0; q < LQ; ++q)
        if (cv[q]) a.out[(long)s * a.out_bstride + (long)n * a.ld_out + a.out_col0 + (long)h * a.dim + col[q]] = acc[q] * inv;
    if (cg == 0 && lane == 0) *reinterpret_cast<float4*>(rsp) = make_float4(T, smin, inv, qs * inv);
}

// d(values) on the transposed lists: one wave per key.  The rows that list the key are taken in ASCENDING order (the transpose
// fills its ranges in whatever order its atomics land: the next row is found by a wave-wide minimum), then the rows whose list
// overflowed, ascending as well - a fixed order, no atomics.  grid (keys / 4, colgroups)
__global__ __launch_bounds__(256) void ragged_list_cols_kernel(RagArgs a, RagLists L) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long kid = (long)blockIdx.x * 4 + wave;
    if (kid >= (long)a.batch * a.n_in) return;
    const int s = (int)(kid / a.n_in), j = (int)(kid - (long)s * a.n_in), cg = blockIdx.y;
    const int lo = clamp_len(a.len_out, s, a.n_out), li = clamp_len(a.len_in, s, a.n_in);
    int col[LQ]; bool cv[LQ];
#pragma unroll
    for (int q = 0; q < LQ; ++q) { col[q] = cg * 64 * LQ + q * 64 + lane; cv[q] = col[q] < a.dim; }
    float* dv = a.d_values + (long)s * a.dvalues_bstride + (long)j * a.ld_dvalues;
    if (j >= li) {
#pragma unroll
        for (int q = 0; q < LQ; ++q) if (cv[q]) dv[col[q]] = 0.0f;
        return;
    }
    const float4 xi = load_pt3(a.mesh_in + (long)s * a.mi_stride + (long)j * a.sdim, a.sdim);
    const int beg = L.rev_ptr[(long)s * (a.n_in + 1) + j], end = L.rev_ptr[(long)s * (a.n_in + 1) + j + 1];
    const int* rrow = L.rev_row + (long)s * a.n_out * L.cap;
    const int* cnts = L.cnt + (long)s * a.n_out;
    float acc[LQ] = {0.0f, 0.0f, 0.0f, 0.0f};
    for (int h = 0; h < a.n_head; ++h) {
        const float c = head_c(a, h);
        const float* go = a.d_out + (long)s * a.dout_bstride + a.out_col0 + (long)h * a.dim;
        auto add_row = [&](int n) {
            const float4 rs = row_stat(a.rowstat, a.n_head, a.n_out, s, h, n);
            const float m = dist3(load_pt3(a.mesh_out + (long)s * a.mo_stride + (long)n * a.sdim, a.sdim), xi);
            const float sv = __fmul_rn(m, c);
            if (sv <= rs.x) {
                const float p = __expf(rs.y - sv) * rs.z;
                const float* gr = go + (long)n * a.ld_dout;
#pragma unroll
                for (int q = 0; q < LQ; ++q) acc[q] += p * (cv[q] ? gr[col[q]] : 0.0f);
            }
        };
        int last = -1;
        for (;;) {
            int nxt = 0x7fffffff;
            for (int base = beg; base < end; base += 64) {
                const int e = base + lane;
                const int r = e < end ? rrow[e] : -1;
                if (r > last) nxt = min(nxt, r);
            }
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) nxt = min(nxt, __shfl_xor(nxt, o));
            if (nxt == 0x7fffffff) break;
            add_row(nxt);
            last = nxt;
        }
        for (int base = 0; base < lo; base += 64) {
            const int n = base + lane;
            unsigned long long mask = __builtin_amdgcn_ballot_w64(n < lo && cnts[min(n, lo - 1)] > L.cap);
            while (mask) {
                const int src = __builtin_ctzll(mask);
                mask &= mask - 1ull;
                add_row(base + src);
            }
        }
    }
    const float* res = a.d_out + (long)s * a.dout_bstride + (long)j * a.ld_dout;
#pragma unroll
    for (int q = 0; q < LQ; ++q)
        if (cv[q]) dv[col[q]] = acc[q] + (a.add_residual ? res[col[q]] : 0.0f);
}

// ---- RelLpNorm over the first len[s] points of every sample (utils.py:86-98 on the truncated sample) -------------------
__device__ __forceinline__ float rag_pow_abs(float x, int p) {
    const float ax = fabsf(x);
    if (p == 1) return ax;
    if (p == 2) return ax * ax;
    return powf(ax, (float)p);
}
// one workgroup per (channel, sample): norms[(s, c)] = {||true - pred||_p, ||true||_p}
__global__ __launch_bounds__(256) void ragged_loss_norms_kernel(const float* __restrict__ tru, const float* __restrict__ pred,
                                                                const int* __restrict__ len, int npts, int nch, int p,
                                                                float* __restrict__ norms) {
    __shared__ double s_num[4], s_den[4];
    const int c = blockIdx.x, s = blockIdx.y;
    const int n = clamp_len(len, s, npts);
    const long base = (long)s * npts * nch + c;
    double num = 0.0, den = 0.0;
    for (int l = threadIdx.x; l < n; l += 256) {          // padded points are skipped, not multiplied by zero
        const float t = tru[base + (long)l * nch], q = pred[base + (long)l * nch];
        num += (double)rag_pow_abs(t - q, p);
        den += (double)rag_pow_abs(t, p);
    }
    num = wave_sum_d(num);
    den = wave_sum_d(den);
    if ((threadIdx.x & 63) == 0) { s_num[threadIdx.x >> 6] = num; s_den[threadIdx.x >> 6] = den; }
    __syncthreads();
    if (threadIdx.x == 0) {
        num = s_num[0] + s_num[1] + s_num[2] + s_num[3];
        den = s_den[0] + s_den[1] + s_den[2] + s_den[3];
        const double nn = (p == 1) ? num : (p == 2 ? sqrt(num) : pow(num, 1.0 / p));
        const double dn = (p == 1) ? den : (p == 2 ? sqrt(den) : pow(den, 1.0 / p));
        norms[((long)s * nch + c) * 2 + 0] = (float)nn;
        norms[((long)s * nch + c) * 2 + 1] = (float)dn;
    }
}
// loss = sum_s mean_c nn / dn, pairs in a fixed order
__global__ __launch_bounds__(64) void ragged_loss_sum_kernel(const float* __restrict__ norms, int pairs, int nch, float* __restrict__ loss) {
    double v = 0.0;
    for (int i = threadIdx.x; i < pairs; i += 64) v += (double)norms[2 * i] / (double)norms[2 * i + 1] / nch;
    v = wave_sum_d(v);
    if (threadIdx.x == 0) *loss = (float)v;
}
__global__ __launch_bounds__(256) void ragged_loss_bwd_kernel(const float* __restrict__ tru, const float* __restrict__ pred,
                                                              const int* __restrict__ len, int batch, int npts, int nch, int p,
                                                              const float* __restrict__ norms, const float* __restrict__ gloss,
                                                              float* __restrict__ d_pred) {
    const long total = (long)batch * npts * nch;
    const float g = gloss ? gloss[0] : 1.0f;
    for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long)gridDim.x * blockDim.x) {
        const int c = (int)(e % nch);
        const long bl = e / nch;
        const int l = (int)(bl % npts), s = (int)(bl / npts);
        float r = 0.0f;
        if (l < clamp_len(len, s, npts)) {
            const float d = pred[e] - tru[e];
            const float nn = norms[((long)s * nch + c) * 2 + 0], dn = norms[((long)s * nch + c) * 2 + 1];
            float dnorm;
            if (p == 1) dnorm = (d > 0.0f) ? 1.0f : (d < 0.0f ? -1.0f : 0.0f);
            else if (p == 2) dnorm = (nn > 0.0f) ? d / nn : 0.0f;
            else dnorm = (nn > 0.0f) ? copysignf(powf(fabsf(d) / nn, (float)(p - 1)), d) : 0.0f;
            r = g * dnorm / (dn * nch);
        }
        d_pred[e] = r;
    }
}

// ---- weight gradients of a pointwise MLP in a FIXED summation order ---------------------------------------------------
// C[m][n] = sum_r A[r][m] B[r][n] and c[m] = sum_r A[r][m]: the rows are cut into `slabs` equal slabs, a workgroup contracts
// one slab into a 64 x 64 tile of its own partial matrix (no atomics), and a second launch adds the partials slab by slab.
// pit_mlp_bwd_params adds its slabs with fp32 atomics, in whatever order they finish: the same inputs give gradients that
// differ in the last bits from run to run, which hides whether padding entered the arithmetic.
struct OrdArgs {
    const float* A; long lda; const float* B; long ldb;
    int rows, M, N, slabs, slab_rows;
    float* part;         // [slabs][M*N + M]
    float* C; float* c; int accumulate;
};
constexpr int OT = 64, OK_ = 16;

__global__ __launch_bounds__(256) void ordered_dw_kernel(OrdArgs g) {
    __shared__ __attribute__((aligned(16))) float s_a[OK_][OT], s_b[OK_][OT];
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    const int m0 = blockIdx.y * OT, n0 = blockIdx.x * OT, ks = blockIdx.z;
    const int rbeg = ks * g.slab_rows, rend = min(g.rows, rbeg + g.slab_rows);
    float acc[4][4], asum[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) { asum[i] = 0.0f;
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = 0.0f; }
    for (int r0 = rbeg; r0 < rend; r0 += OK_) {
#pragma unroll
        for (int u = 0; u < OK_ * OT / 256; ++u) {
            const int e = tid + 256 * u, rr = e >> 6, cc = e & 63, r = r0 + rr;
            s_a[rr][cc] = (r < rend && m0 + cc < g.M) ? g.A[(long)r * g.lda + m0 + cc] : 0.0f;
            s_b[rr][cc] = (r < rend && n0 + cc < g.N) ? g.B[(long)r * g.ldb + n0 + cc] : 0.0f;
        }
        __syncthreads();
#pragma unroll
        for (int rr = 0; rr < OK_; ++rr) {
            const float4 a = *reinterpret_cast<const float4*>(&s_a[rr][ty * 4]);
            const float4 b = *reinterpret_cast<const float4*>(&s_b[rr][tx * 4]);
            const float av[4] = {a.x, a.y, a.z, a.w}, bv[4] = {b.x, b.y, b.z, b.w};
#pragma unroll
            for (int i = 0; i < 4; ++i) { asum[i] += av[i];
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[i][j] += av[i] * bv[j]; }
        }
        __syncthreads();
    }
    float* part = g.part + (long)ks * ((long)g.M * g.N + g.M);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int m = m0 + ty * 4 + i;
        if (m >= g.M) continue;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int n = n0 + tx * 4 + j;
            if (n < g.N) part[(long)m * g.N + n] = acc[i][j];
        }
        if (blockIdx.x == 0 && tx == 0) part[(long)g.M * g.N + m] = asum[i];
    }
}
__global__ __launch_bounds__(256) void ordered_dw_finish_kernel(OrdArgs g) {
    const long mn = (long)g.M * g.N, total = mn + g.M;
    for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long)gridDim.x * blockDim.x) {
        float v = 0.0f;
        for (int ks = 0; ks < g.slabs; ++ks) v += g.part[(long)ks * total + e];
        float* dst = e < mn ? g.C + e : g.c + (e - mn);
        *dst = g.accumulate ? *dst + v : v;
    }
}

static int ordered_slabs(int rows) { return std::max(1, std::min(16, (rows + 255) / 256)); }

static int launch_ordered(const float* A, long lda, const float* B, long ldb, int rows, int M, int N, float* part, float* C, float* c,
                          int accumulate, hipStream_t s) {
    OrdArgs g;
    g.A = A; g.lda = lda; g.B = B; g.ldb = ldb; g.rows = rows; g.M = M; g.N = N;
    g.slabs = ordered_slabs(rows);
    g.slab_rows = (rows + g.slabs - 1) / g.slabs;
    g.part = part; g.C = C; g.c = c; g.accumulate = accumulate;
    hipLaunchKernelGGL(ordered_dw_kernel, dim3((unsigned)((N + OT - 1) / OT), (unsigned)((M + OT - 1) / OT), (unsigned)g.slabs), dim3(256), 0, s, g);
    PIT_CHECK_LAUNCH();
    const long total = (long)M * N + M;
    hipLaunchKernelGGL(ordered_dw_finish_kernel, dim3((unsigned)std::min<long>((total + 255) / 256, 2048L)), dim3(256), 0, s, g);
    PIT_CHECK_LAUNCH();
    return 0;
}

}  // namespace

extern "C" long pit_mlp_bwd_params_ordered_workspace(int rows, int n0, int n1, int n2) {
    if (rows <= 0 || n0 <= 0 || n1 <= 0 || n2 <= 0) return 0;
    const long a = (long)n1 * n0 + n1, b = (long)n2 * n1 + n2;
    return (long)ordered_slabs(rows) * std::max(a, b) * (long)sizeof(float);
}

extern "C" int pit_mlp_bwd_params_ordered(const float* x, long ldx, int rows, int n0, int n1, int n2, const float* h,
                                          int out_gelu, const float* d_y, long ld_dy,
                                          float* d_w1, float* d_b1, float* d_w2, float* d_b2,
                                          int accumulate, const float* scratch, float* workspace, void* stream) {
    if (!x || !h || !d_y || !d_w1 || !d_b1 || !d_w2 || !d_b2 || !scratch || !workspace) return PIT_ERR_NULL;
    if (rows <= 0 || n0 <= 0 || n1 <= 0 || n2 <= 0) return PIT_ERR_SIZE;
    hipStream_t s = (hipStream_t)stream;
    const float* dz1 = scratch;                                           // the layout of pit_mlp_bwd_data
    const float* dz2 = out_gelu ? scratch + (long)rows * n1 : d_y;
    const long ld_dz2 = out_gelu ? n2 : ld_dy;
    if (int rc = launch_ordered(dz2, ld_dz2, h, n1, rows, n2, n1, workspace, d_w2, d_b2, accumulate, s)) return rc;
    return launch_ordered(dz1, n1, x, ldx, rows, n1, n0, workspace, d_w1, d_b1, accumulate, s);
}

static int rag_check_sizes(int batch, int n_out, int n_in, int space_dim) {
    if (batch <= 0 || batch > 65535 || n_out <= 0 || n_in <= 0) return PIT_ERR_SIZE;
    if (space_dim < 1) return PIT_ERR_SIZE;
    if (space_dim > 3) return PIT_ERR_UNSUPPORTED;
    return 0;
}

// a sample stride in points: 0 (one mesh for the whole batch) or at least the mesh's width
static bool rag_stride_ok(long stride, int n) { return stride == 0 || stride >= n; }

// The entry points below in one form: sample strides in POINTS per mesh (0 = shared by the batch) and lengths that may be NULL
// (= full width).  The ABI 27 entries pass stride n and their (non-NULL) lengths: the arithmetic they always did.
static int plan_ragged(const float* mesh_out, const float* mesh_in, int mesh_batch, int n_out, int n_in,
                       int space_dim, long out_stride, long in_stride, const int* len_out, const int* len_in, float locality, int need_kth,
                       float* stats, float* rank_w, int cap, int* nbr_idx, int* nbr_cnt, void* stream) {
    if (!mesh_out || !mesh_in || !stats || !rank_w) return PIT_ERR_NULL;
    if (int rc = rag_check_sizes(mesh_batch, n_out, n_in, space_dim)) return rc;
    if (!rag_stride_ok(out_stride, n_out) || !rag_stride_ok(in_stride, n_in)) return PIT_ERR_SIZE;
    if (!(locality >= 0.0f && locality <= 1.0f)) return PIT_ERR_SIZE;
    RagSelectArgs a;
    a.mesh_out = mesh_out; a.mesh_in = mesh_in; a.len_out = len_out; a.len_in = len_in; a.stats = stats; a.rank_w = rank_w;
    a.mo_stride = out_stride * space_dim; a.mi_stride = in_stride * space_dim;
    a.batch = mesh_batch; a.n_out = n_out; a.n_in = n_in; a.sdim = space_dim; a.q = locality; a.need_kth = need_kth;
    hipLaunchKernelGGL(ragged_select_kernel, dim3((unsigned)((long)mesh_batch * n_out)), dim3(256), 0, (hipStream_t)stream, a);
    PIT_CHECK_LAUNCH();
    if (nbr_idx) {
        if (!nbr_cnt) return PIT_ERR_NULL;
        if (cap <= 0 || !need_kth) return PIT_ERR_SIZE;
        hipLaunchKernelGGL(ragged_neighbors_kernel, dim3((unsigned)(((long)mesh_batch * n_out + 3) / 4)), dim3(256), 0, (hipStream_t)stream,
                           a, cap, nbr_idx, nbr_cnt);
        PIT_CHECK_LAUNCH();
    }
    return 0;
}

static int posatt_ragged_fwd(const float* mesh_out, const float* mesh_in, int mesh_batch, int n_out, int n_in,
                                     int space_dim, long out_stride, long in_stride, const int* len_out, const int* len_in,
                                     const float* values, int dim, long ld_values, long values_bstride,
                                     const float* head, int n_head, int head_is_scale,
                                     const float* stats, const float* rank_w, int masked,
                                     float* out, long ld_out, long out_bstride, int out_col0, int copy_inputs,
                                     float* rowstat, float* scale_out,
                                     const int* nbr_idx, const int* nbr_cnt, int nbr_cap, int math_mode, void* stream) {
    if (!mesh_out || !mesh_in || !values || !head || !stats || !out || !rowstat) return PIT_ERR_NULL;
    if (masked && !rank_w) return PIT_ERR_NULL;
    if (int rc = rag_check_sizes(mesh_batch, n_out, n_in, space_dim)) return rc;
    if (!rag_stride_ok(out_stride, n_out) || !rag_stride_ok(in_stride, n_in)) return PIT_ERR_SIZE;
    if (dim <= 0 || n_head <= 0 || (copy_inputs && n_out != n_in)) return PIT_ERR_SIZE;
    if (math_mode != PIT_MATH_FP32) return PIT_ERR_UNSUPPORTED;
    RagArgs a = RagArgs();
    a.mesh_out = mesh_out; a.mesh_in = mesh_in; a.len_out = len_out; a.len_in = len_in;
    a.mo_stride = out_stride * space_dim; a.mi_stride = in_stride * space_dim;
    a.batch = mesh_batch; a.n_out = n_out; a.n_in = n_in; a.sdim = space_dim;
    a.rank_w = rank_w;
    layer_set_fwd(a, values, dim, ld_values, values_bstride, head, n_head, head_is_scale, stats, masked, out, ld_out, out_bstride, out_col0,
                  copy_inputs, rowstat, scale_out);
    a.colgroups = (dim + 255) / 256;
    if ((long)n_head * a.colgroups > 65535) return PIT_ERR_SIZE;
    if (nbr_idx && masked) {
        if (!nbr_cnt) return PIT_ERR_NULL;
        if (nbr_cap <= 0) return PIT_ERR_SIZE;
        const RagLists L = {nbr_idx, nbr_cnt, nbr_cap, nullptr, nullptr};
        const dim3 lgrid((unsigned)(((long)mesh_batch * n_out + 3) / 4), (unsigned)n_head, (unsigned)((dim + 64 * LQ - 1) / (64 * LQ)));
        hipLaunchKernelGGL(ragged_list_rows_kernel<0>, lgrid, dim3(256), 0, (hipStream_t)stream, a, L);
        PIT_CHECK_LAUNCH();
        return 0;
    }
    const dim3 grid((unsigned)((n_out + RT - 1) / RT), (unsigned)mesh_batch, (unsigned)(n_head * a.colgroups));
    hipLaunchKernelGGL(ragged_rows_kernel<0>, grid, dim3(256), 0, (hipStream_t)stream, a);
    PIT_CHECK_LAUNCH();
    return 0;
}

static int posatt_ragged_bwd(const float* mesh_out, const float* mesh_in, int mesh_batch, int n_out, int n_in,
                                     int space_dim, long out_stride, long in_stride, const int* len_out, const int* len_in,
                                     const float* values, int dim, long ld_values, long values_bstride,
                                     const float* head, int n_head, int head_is_scale, const float* scale,
                                     const float* rowstat, int masked,
                                     const float* d_out, long ld_dout, long dout_bstride, int out_col0,
                                     float* d_values, long ld_dvalues, long dvalues_bstride, int add_residual,
                                     float* d_head, int accumulate_head, double* workspace,
                                     const int* nbr_idx, const int* nbr_cnt, int nbr_cap, const int* rev_ptr, const int* rev_row,
                                     int math_mode, void* stream) {
    if (!mesh_out || !mesh_in || !values || !head || !rowstat || !d_out) return PIT_ERR_NULL;
    if (d_head && !workspace) return PIT_ERR_NULL;
    if (int rc = rag_check_sizes(mesh_batch, n_out, n_in, space_dim)) return rc;
    if (!rag_stride_ok(out_stride, n_out) || !rag_stride_ok(in_stride, n_in)) return PIT_ERR_SIZE;
    if (dim <= 0 || n_head <= 0 || (add_residual && n_out != n_in)) return PIT_ERR_SIZE;
    if (math_mode != PIT_MATH_FP32) return PIT_ERR_UNSUPPORTED;
    RagArgs a = RagArgs();
    a.mesh_out = mesh_out; a.mesh_in = mesh_in; a.len_out = len_out; a.len_in = len_in;
    a.mo_stride = out_stride * space_dim; a.mi_stride = in_stride * space_dim;
    a.batch = mesh_batch; a.n_out = n_out; a.n_in = n_in; a.sdim = space_dim;
    layer_set_bwd(a, values, dim, ld_values, values_bstride, head, n_head, head_is_scale, scale, rowstat, masked, d_out, ld_dout, dout_bstride,
                  out_col0, d_values, ld_dvalues, dvalues_bstride, add_residual, d_head, workspace);
    a.colgroups = (dim + 255) / 256;
    if ((long)n_head * a.colgroups > 65535) return PIT_ERR_SIZE;
    hipStream_t s = (hipStream_t)stream;
    const bool lists = nbr_idx && masked;
    if (lists && (!nbr_cnt || (rev_ptr && !rev_row))) return PIT_ERR_NULL;
    if (lists && nbr_cap <= 0) return PIT_ERR_SIZE;
    const RagLists L = {nbr_idx, nbr_cnt, nbr_cap, rev_ptr, rev_row};
    const unsigned lcg = (unsigned)((dim + 64 * LQ - 1) / (64 * LQ));
    if (d_values) {
        if (lists && rev_ptr) {                           // (lists without their transpose: the dense kernel, which needs none)
            hipLaunchKernelGGL(ragged_list_cols_kernel, dim3((unsigned)(((long)mesh_batch * n_in + 3) / 4), lcg), dim3(256), 0, s, a, L);
        } else {
            const dim3 grid((unsigned)((n_in + RT - 1) / RT), (unsigned)mesh_batch, (unsigned)a.colgroups);
            hipLaunchKernelGGL(ragged_cols_kernel, grid, dim3(256), 0, s, a);
        }
        PIT_CHECK_LAUNCH();
    }
    if (d_head) {
        if (lists) {
            hipLaunchKernelGGL(ragged_list_rows_kernel<1>, dim3((unsigned)(((long)mesh_batch * n_out + 3) / 4), (unsigned)n_head, lcg), dim3(256), 0, s, a, L);
        } else {
            const dim3 grid((unsigned)((n_out + RT - 1) / RT), (unsigned)mesh_batch, (unsigned)(n_head * a.colgroups));
            hipLaunchKernelGGL(ragged_rows_kernel<1>, grid, dim3(256), 0, s, a);
        }
        PIT_CHECK_LAUNCH();
    }
    return layer_finish_head(head, scale, d_head, workspace, n_head, accumulate_head, head_is_scale, stream);
}

extern "C" int pit_plan_ragged_fwd(const float* mesh_out, const float* mesh_in, int mesh_batch, int n_out, int n_in,
                                   int space_dim, const int* len_out, const int* len_in, float locality, int need_kth,
                                   float* stats, float* rank_w, int cap, int* nbr_idx, int* nbr_cnt, void* stream) {
    if (!len_out || !len_in) return PIT_ERR_NULL;
    return plan_ragged(mesh_out, mesh_in, mesh_batch, n_out, n_in, space_dim, n_out, n_in, len_out, len_in, locality, need_kth,
                       stats, rank_w, cap, nbr_idx, nbr_cnt, stream);
}

extern "C" int pit_plan_ragged_strided_fwd(const float* mesh_out, const float* mesh_in, int mesh_batch, int n_out, int n_in,
                                           int space_dim, long out_stride, long in_stride, const int* len_out, const int* len_in,
                                           float locality, int need_kth, float* stats, float* rank_w, int cap, int* nbr_idx,
                                           int* nbr_cnt, void* stream) {
    return plan_ragged(mesh_out, mesh_in, mesh_batch, n_out, n_in, space_dim, out_stride, in_stride, len_out, len_in, locality, need_kth,
                       stats, rank_w, cap, nbr_idx, nbr_cnt, stream);
}

extern "C" int pit_posatt_ragged_fwd(const float* mesh_out, const float* mesh_in, int mesh_batch, int n_out, int n_in,
                                     int space_dim, const int* len_out, const int* len_in,
                                     const float* values, int dim, long ld_values, long values_bstride,
                                     const float* head, int n_head, int head_is_scale,
                                     const float* stats, const float* rank_w, int masked,
                                     float* out, long ld_out, long out_bstride, int out_col0, int copy_inputs,
                                     float* rowstat, float* scale_out,
                                     const int* nbr_idx, const int* nbr_cnt, int nbr_cap, int math_mode, void* stream) {
    if (!len_out || !len_in) return PIT_ERR_NULL;
    return posatt_ragged_fwd(mesh_out, mesh_in, mesh_batch, n_out, n_in, space_dim, n_out, n_in, len_out, len_in, values, dim, ld_values,
                             values_bstride, head, n_head, head_is_scale, stats, rank_w, masked, out, ld_out, out_bstride, out_col0,
                             copy_inputs, rowstat, scale_out, nbr_idx, nbr_cnt, nbr_cap, math_mode, stream);
}

extern "C" int pit_posatt_ragged_strided_fwd(const float* mesh_out, const float* mesh_in, int mesh_batch, int n_out, int n_in,
                                             int space_dim, long out_stride, long in_stride, const int* len_out, const int* len_in,
                                             const float* values, int dim, long ld_values, long values_bstride,
                                             const float* head, int n_head, int head_is_scale,
                                             const float* stats, const float* rank_w, int masked,
                                             float* out, long ld_out, long out_bstride, int out_col0, int copy_inputs,
                                             float* rowstat, float* scale_out,
                                             const int* nbr_idx, const int* nbr_cnt, int nbr_cap, int math_mode, void* stream) {
    return posatt_ragged_fwd(mesh_out, mesh_in, mesh_batch, n_out, n_in, space_dim, out_stride, in_stride, len_out, len_in, values, dim,
                             ld_values, values_bstride, head, n_head, head_is_scale, stats, rank_w, masked, out, ld_out, out_bstride,
                             out_col0, copy_inputs, rowstat, scale_out, nbr_idx, nbr_cnt, nbr_cap, math_mode, stream);
}

extern "C" int pit_posatt_ragged_bwd(const float* mesh_out, const float* mesh_in, int mesh_batch, int n_out, int n_in,
                                     int space_dim, const int* len_out, const int* len_in,
                                     const float* values, int dim, long ld_values, long values_bstride,
                                     const float* head, int n_head, int head_is_scale, const float* scale,
                                     const float* rowstat, int masked,
                                     const float* d_out, long ld_dout, long dout_bstride, int out_col0,
                                     float* d_values, long ld_dvalues, long dvalues_bstride, int add_residual,
                                     float* d_head, int accumulate_head, double* workspace,
                                     const int* nbr_idx, const int* nbr_cnt, int nbr_cap, const int* rev_ptr, const int* rev_row,
                                     int math_mode, void* stream) {
    if (!len_out || !len_in) return PIT_ERR_NULL;
    return posatt_ragged_bwd(mesh_out, mesh_in, mesh_batch, n_out, n_in, space_dim, n_out, n_in, len_out, len_in, values, dim, ld_values,
                             values_bstride, head, n_head, head_is_scale, scale, rowstat, masked, d_out, ld_dout, dout_bstride, out_col0,
                             d_values, ld_dvalues, dvalues_bstride, add_residual, d_head, accumulate_head, workspace, nbr_idx, nbr_cnt,
                             nbr_cap, rev_ptr, rev_row, math_mode, stream);
}

extern "C" int pit_posatt_ragged_strided_bwd(const float* mesh_out, const float* mesh_in, int mesh_batch, int n_out, int n_in,
                                             int space_dim, long out_stride, long in_stride, const int* len_out, const int* len_in,
                                             const float* values, int dim, long ld_values, long values_bstride,
                                             const float* head, int n_head, int head_is_scale, const float* scale,
                                             const float* rowstat, int masked,
                                             const float* d_out, long ld_dout, long dout_bstride, int out_col0,
                                             float* d_values, long ld_dvalues, long dvalues_bstride, int add_residual,
                                             float* d_head, int accumulate_head, double* workspace,
                                             const int* nbr_idx, const int* nbr_cnt, int nbr_cap, const int* rev_ptr, const int* rev_row,
                                             int math_mode, void* stream) {
    return posatt_ragged_bwd(mesh_out, mesh_in, mesh_batch, n_out, n_in, space_dim, out_stride, in_stride, len_out, len_in, values, dim,
                             ld_values, values_bstride, head, n_head, head_is_scale, scale, rowstat, masked, d_out, ld_dout, dout_bstride,
                             out_col0, d_values, ld_dvalues, dvalues_bstride, add_residual, d_head, accumulate_head, workspace, nbr_idx,
                             nbr_cnt, nbr_cap, rev_ptr, rev_row, math_mode, stream);
}

extern "C" int pit_rel_lp_loss_ragged_fwd(const float* tru, const float* pred, const int* len, int batch, int npts, int nch, int p,
                                          float* norms, float* loss, void* stream) {
    if (!tru || !pred || !len || !norms || !loss) return PIT_ERR_NULL;
    if (batch <= 0 || batch > 65535 || npts <= 0 || nch <= 0 || p < 1) return PIT_ERR_SIZE;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(ragged_loss_norms_kernel, dim3((unsigned)nch, (unsigned)batch), dim3(256), 0, s, tru, pred, len, npts, nch, p, norms);
    PIT_CHECK_LAUNCH();
    hipLaunchKernelGGL(ragged_loss_sum_kernel, dim3(1), dim3(64), 0, s, norms, batch * nch, nch, loss);
    PIT_CHECK_LAUNCH();
    return 0;
}

extern "C" int pit_rel_lp_loss_ragged_bwd(const float* tru, const float* pred, const int* len, int batch, int npts, int nch, int p,
                                          const float* norms, const float* gloss, float* d_pred, void* stream) {
    if (!tru || !pred || !len || !norms || !d_pred) return PIT_ERR_NULL;
    if (batch <= 0 || npts <= 0 || nch <= 0 || p < 1) return PIT_ERR_SIZE;
    const long total = (long)batch * npts * nch;
    const unsigned blocks = (unsigned)std::min<long>((total + 255) / 256, 4096L);
    hipLaunchKernelGGL(ragged_loss_bwd_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, tru, pred, len, batch, npts, nch, p,
                       norms, gloss, d_pred);
    PIT_CHECK_LAUNCH();
    return 0;
}
