// Position attention on CALLER-SUPPLIED squared distances (any metric), fp32, for gfx950.
//
// The reference's extension point for another metric is overriding posatt.dist2att (pit.py:42-43,68-69): the layer itself is
// pit.py:48-57 applied to whatever matrix m the metric produced.  The kernels below take m - (n_out, n_in) shared by the batch
// or (batch, n_out, n_in), rows ld_m apart - instead of two meshes, and leave everything else as pit_posatt_fwd / _bwd have it:
//   S = fl(c m), kept iff S <= T = quantile_lerp(fl(c m_(k)), fl(c m_(k+1)), w), P = exp(S_min - S) / rowsum over the kept keys.
// Precondition: m finite and >= 0 (not checked: a check would synchronise).  Whatever m holds, no index is formed from its
// values, so nothing is addressed out of bounds.
//
//   selection   one workgroup per row: MSB-first bitwise search over the row's bit patterns (ragged_select_kernel); a row of up
//               to DM_SEL_LDS keys is staged in LDS once and searched there, a longer one is streamed from memory.
//   forward     a workgroup owns 32 rows x 256 value columns of one sample and head.  The keys are walked in tiles of 64: all
//               256 threads form the 32 x 64 weights of the tile into LDS (m read once, coalesced), then every wave contracts
//               them against its 64 columns with v_mfma_f32_32x32x2_f32 (A = weights from LDS, B = value rows from memory).
//   d(values)   the same tile machine transposed: a workgroup owns 32 keys, walks heads and rows, A = P^T, B = d_out rows.
//   d(scale)    d c = -sum_ij s_ij m_ij = -sum_i g_i . sum_j P_ij (m_ij - mbar_i) v_j: the forward's tile machine with those
//               weights (mbar_i = sum_j P_ij m_ij is in rowstat), the contracted rows dotted with d_out.
//   d(m)        a_i = sum_j P_ij gv_ij = g_i . out_i from the forward's result (a wave per row); then a workgroup owns a 32 x 128
//               tile of d_m, a wave forms the 32 x 32 tiles of gv = g . v on the matrix pipe (the channel axis contracted;
//               gv_tile of pit_layer.h) and loops over heads and - for a shared matrix - over the samples in ascending
//               order: d m_ij = -sum_h c_h P_ij (gv_ij - a_i).  No buffer of per-sample partials exists.
// Tiles whose weights are all zero (masked layers: most of them) skip their contraction - a wave- or workgroup-uniform branch.
// Every sum except d(scale)'s fp64 slots (the PIT_DSCALE_SLOTS convention of pit_posatt_bwd) has a fixed order; no atomics
// otherwise: the same input gives the same bits on every run.  Rows, keys and channels beyond a tensor read 0 through sized
// buffer descriptors (one per sample, built from workgroup-uniform values).
#include "pit_layer.h"

namespace {

constexpr int DM_SEL_LDS = 2048;   // keys of a row the selection keeps in LDS (longer rows are streamed)
constexpr int RT = 32;             // owner items (rows; keys for d(values)) per workgroup
constexpr int KT = 64;             // contracted items per tile

// ---- selection --------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void distmat_select_kernel(const float* __restrict__ m, long ld_m, long m_bstride, int n_out, int n_in,
                                                             int k, int need_kth, long rows, float* __restrict__ stats) {
    __shared__ uint32_t s_row[DM_SEL_LDS];
    __shared__ int s_cnt[4];
    __shared__ uint32_t s_min[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long row = blockIdx.x;
    const int s = (int)(row / n_out), i = (int)(row - (long)s * n_out);
    const uint32_t* src = reinterpret_cast<const uint32_t*>(m + (long)s * m_bstride + (long)i * ld_m);
    const bool in_lds = n_in <= DM_SEL_LDS;               // (a kernel argument: uniform)
    if (in_lds) {
        for (int j = threadIdx.x; j < n_in; j += 256) s_row[j] = src[j];
        __syncthreads();
    }
    auto key_at = [&](int j) -> uint32_t { return in_lds ? s_row[j] : src[j]; };
    auto block_count = [&](uint32_t cand, bool inclusive) -> int {
        int c = 0;
        for (int j = threadIdx.x; j < n_in; j += 256) {
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
        uint32_t mn = 0xFFFFFFFFu;
        for (int j = threadIdx.x; j < n_in; j += 256) {
            const uint32_t kk = key_at(j);
            if (!strictly_above || kk > bound) mn = min(mn, kk);
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) mn = min(mn, (uint32_t)__shfl_xor((int)mn, o));
        __syncthreads();
        if (lane == 0) s_min[wave] = mn;
        __syncthreads();
        return min(min(s_min[0], s_min[1]), min(s_min[2], s_min[3]));
    };
    const uint32_t kmin = block_min_above(0, false);
    uint32_t vk = kmin, vk1 = kmin;
    if (need_kth) {
        uint32_t prefix = 0;
        for (int bit = 30; bit >= 0; --bit) {             // MSB-first bitwise search (pit_select.hip, ragged_select_kernel)
            const uint32_t cand = prefix | (1u << bit);
            if (block_count(cand, false) <= k) prefix = cand;
        }
        vk = prefix;
        const int cnt_le = block_count(vk, true);
        const uint32_t next = block_min_above(vk, true);
        vk1 = (cnt_le >= k + 2 || k + 1 > n_in - 1) ? vk : next;
    }
    if (threadIdx.x == 0) {
        stats[row] = __uint_as_float(vk);
        stats[rows + row] = __uint_as_float(vk1);
        stats[2 * rows + row] = __uint_as_float(kmin);
    }
}

// ---- attention --------------------------------------------------------------------------------------------------------
struct DmatArgs : LayerIO {
    const float* m; long ld_m, m_bstride;        // m_bstride 0: one matrix shared by the batch
    int batch, n_out, n_in;
    float rank_w;
    float* a_ws;
    float* d_m;
    unsigned m_bytes;                            // of ONE sample's rows: the size of its buffer descriptor
};

// One tile's contraction for a wave: acc{0,1}[owner][col] += sum_t w[t][owner] * x[t0 + t][col] over the tile's KT items, for
// the wave's two 32-column tiles at cb and cb + 32 (columns of x from xcol0 on).  A: lane l holds w[2u + half][l & 31] (LDS),
// B: x[t0 + 2u + half][col] through the descriptor; items >= t_end and columns >= dim read 0.
__device__ __forceinline__ void contract_tile(const float (*w)[RT + 1], __amdgpu_buffer_rsrc_t rx, unsigned x_bytes, long ldx, int xcol0,
                                              int t0, int t_end, int cb, int dim, f32x16& acc0, f32x16& acc1) {
    const int lane = threadIdx.x & 63, half = lane >> 5, l31 = lane & 31;
    const int c0 = cb + l31, c1 = cb + 32 + l31;
    const bool ok0 = c0 < dim, ok1 = c1 < dim;
#pragma unroll 8
    for (int u = 0; u < KT / 2; ++u) {
        const int t = 2 * u + half, item = t0 + t;
        const bool tv = item < t_end;
        const unsigned base = (unsigned)(((long)item * ldx + xcol0) * 4);
        const float x0 = buf_load(rx, (tv && ok0) ? base + (unsigned)c0 * 4u : x_bytes);
        const float x1 = buf_load(rx, (tv && ok1) ? base + (unsigned)c1 * 4u : x_bytes);
        const float wv = w[t][l31];
        acc0 = mfma_32x32x2(wv, x0, acc0);
        acc1 = mfma_32x32x2(wv, x1, acc1);
    }
}

// MODE 0: forward.  MODE 1: d(scale) - the same tile machine with the weights P_ij (m_ij - mbar_i) from the saved rowstat; the
// contracted rows are dotted with d_out and meet in the fp64 slots.  grid (row tiles, batch, n_head * colgroups)
template <int MODE>
__global__ __launch_bounds__(256) void distmat_rows_kernel(DmatArgs a) {
    __shared__ float s_w[KT][RT + 1];
    __shared__ float4 s_rs[RT];          // {T, S_min, 1/rowsum, mbar} of the tile's rows
    __shared__ int s_any[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, half = lane >> 5, l31 = lane & 31;
    const int s = blockIdx.y, r0 = blockIdx.x * RT;
    const int h = blockIdx.z / a.colgroups, cg = blockIdx.z - h * a.colgroups;
    const int mb = a.m_bstride ? s : 0;
    const float c = head_c(a, h);
    const __amdgpu_buffer_rsrc_t rm = make_rsrc(a.m + (long)mb * a.m_bstride, a.m_bytes);
    const __amdgpu_buffer_rsrc_t rv = make_rsrc(a.values + (long)s * a.values_bstride, a.values_bytes);
    const int cb = cg * 256 + wave * 64;
    const int rows_here = min(RT, a.n_out - r0);
    const long rows_total = (long)(a.m_bstride ? a.batch : 1) * a.n_out;

    if (MODE == 0 && a.copy_inputs && h == 0) {           // torch.cat((inputs, conv), -1): the copied columns as they are
        const int col = cb + lane;                        // (eight rows' loads in flight, then their stores)
        const bool cok = col < a.dim;
        for (int rb = 0; rb < rows_here; rb += 8) {
            float v[8];
#pragma unroll
            for (int u = 0; u < 8; ++u)
                v[u] = buf_load(rv, (cok && rb + u < rows_here) ? (unsigned)(((long)(r0 + rb + u) * a.ld_values + col) * 4) : a.values_bytes);
#pragma unroll
            for (int u = 0; u < 8; ++u)
                if (cok && rb + u < rows_here) a.out[(long)s * a.out_bstride + (long)(r0 + rb + u) * a.ld_out + col] = v[u];
        }
    }
    if (MODE == 0 && s == 0 && blockIdx.x == 0 && cg == 0 && tid == 0 && a.scale_out) a.scale_out[h] = c;
    if (MODE == 1) {
        if (tid < RT) s_rs[tid] = row_stat(a.rowstat, a.n_head, a.n_out, mb, h, min(r0 + tid, a.n_out - 1));
    } else if (tid < RT) {
        const long row = (long)mb * a.n_out + min(r0 + tid, a.n_out - 1);
        float4 st;
        st.x = a.masked ? quantile_lerp(__fmul_rn(c, a.stats[row]), __fmul_rn(c, a.stats[rows_total + row]), a.rank_w) : __builtin_inff();
        st.y = __fmul_rn(c, a.stats[2 * rows_total + row]);
        st.z = 0.0f; st.w = 0.0f;
        s_rs[tid] = st;
    }
    __syncthreads();
    // weights: wave w forms rows 8w .. 8w + 7 of the tile, lane = key (m read in 256-byte pieces)
    float4 rs[8];
    float rsum[8], qsum[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) { rs[q] = s_rs[wave * 8 + q]; rsum[q] = 0.0f; qsum[q] = 0.0f; }
    f32x16 acc0, acc1;
#pragma unroll
    for (int r = 0; r < 16; ++r) { acc0[r] = 0.0f; acc1[r] = 0.0f; }
    const bool wave_cols = cb < a.dim;

    for (int j0 = 0; j0 < a.n_in; j0 += KT) {
        const int key = j0 + lane;
        const bool kv = key < a.n_in;
        bool any = false;
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const int rr = wave * 8 + q, row = r0 + rr;
            const bool valid = kv && row < a.n_out;
            const float mv = buf_load(rm, valid ? (unsigned)(((long)row * a.ld_m + key) * 4) : a.m_bytes);
            float p = weight_raw(mv, c, rs[q].x, rs[q].y, valid, a.masked);
            if (MODE == 0) { rsum[q] += p; qsum[q] += p * mv; }
            else p = p * rs[q].z * (mv - rs[q].w);
            any = any || (p != 0.0f);
            s_w[lane][rr] = p;
        }
        const unsigned long long bal = __builtin_amdgcn_ballot_w64(any);
        if (lane == 0) s_any[wave] = bal != 0ull;
        __syncthreads();
        if (wave_cols && (s_any[0] | s_any[1] | s_any[2] | s_any[3]))
            contract_tile(s_w, rv, a.values_bytes, a.ld_values, 0, j0, a.n_in, cb, a.dim, acc0, acc1);
        __syncthreads();
    }
    if (MODE == 1) {
        float ds = 0.0f;
        if (wave_cols) {
            const __amdgpu_buffer_rsrc_t rg = make_rsrc(a.d_out + (long)s * a.dout_bstride, a.dout_bytes);
            const int c0 = cb + l31, c1 = cb + 32 + l31;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int ri = acc_row(r, half);
                const bool rvalid = ri < rows_here;
                const unsigned base = (unsigned)(((long)(r0 + ri) * a.ld_dout + a.out_col0 + (long)h * a.dim) * 4);
                ds += acc0[r] * buf_load(rg, (rvalid && c0 < a.dim) ? base + (unsigned)c0 * 4u : a.dout_bytes);
                ds += acc1[r] * buf_load(rg, (rvalid && c1 < a.dim) ? base + (unsigned)c1 * 4u : a.dout_bytes);
            }
        }
        const double part = wave_sum_d((double)ds);
        const int slot = (int)((blockIdx.x + 131u * blockIdx.y + 977u * (cg * 4 + wave)) & (PIT_DSCALE_SLOTS - 1));
        if (lane == 0 && wave_cols) atomicAdd(a.dscale_acc + (long)h * PIT_DSCALE_SLOTS + slot, -part);
        return;
    }
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        const float rsm = wave_sum(rsum[q]), qs = wave_sum(qsum[q]);
        if (lane == 0) {
            const float inv = rsm > 0.0f ? 1.0f / rsm : 0.0f;
            float4 st = rs[q];
            st.z = inv; st.w = qs * inv;
            s_rs[wave * 8 + q] = st;
        }
    }
    __syncthreads();
    if (cg == 0 && tid < rows_here && (a.m_bstride || s == 0))
        *reinterpret_cast<float4*>(a.rowstat + (((long)mb * a.n_head + h) * a.n_out + r0 + tid) * 4) = s_rs[tid];
    if (wave_cols) {
        float* o = a.out + (long)s * a.out_bstride + (long)r0 * a.ld_out + a.out_col0 + (long)h * a.dim;
        const int c0 = cb + l31, c1 = cb + 32 + l31;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int ri = acc_row(r, half);
            if (ri < rows_here) {
                const float inv = s_rs[ri].z;
                if (c0 < a.dim) o[(long)ri * a.ld_out + c0] = acc0[r] * inv;
                if (c1 < a.dim) o[(long)ri * a.ld_out + c1] = acc1[r] * inv;
            }
        }
    }
}

// d(values): a workgroup owns 32 keys of one sample and 256 columns; d_values[s, j, :] = (residual) + sum_h sum_i P_h[i, j]
// d_out[s, i, head h], heads and rows in ascending order.  grid (key tiles, batch, colgroups)
__global__ __launch_bounds__(256) void distmat_dv_kernel(DmatArgs a) {
    __shared__ float s_w[KT][RT + 1];
    __shared__ int s_any[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, half = lane >> 5, l31 = lane & 31;
    const int s = blockIdx.y, k0 = blockIdx.x * RT, cg = blockIdx.z;
    const int mb = a.m_bstride ? s : 0;
    const __amdgpu_buffer_rsrc_t rm = make_rsrc(a.m + (long)mb * a.m_bstride, a.m_bytes);
    const __amdgpu_buffer_rsrc_t rg = make_rsrc(a.d_out + (long)s * a.dout_bstride, a.dout_bytes);
    const int cb = cg * 256 + wave * 64;
    const bool wave_cols = cb < a.dim;
    const int keys_here = min(RT, a.n_in - k0);
    const int key = k0 + l31, tr = tid >> 5;              // this thread's key and its rows tr, tr + 8, ... of a tile
    const bool kv = key < a.n_in;
    f32x16 acc0, acc1;
#pragma unroll
    for (int r = 0; r < 16; ++r) { acc0[r] = 0.0f; acc1[r] = 0.0f; }
    for (int h = 0; h < a.n_head; ++h) {
        const float c = head_c(a, h);
        for (int n0 = 0; n0 < a.n_out; n0 += KT) {
            bool any = false;
#pragma unroll
            for (int q = 0; q < KT / 8; ++q) {
                const int t = tr + 8 * q, row = n0 + t;
                const bool valid = kv && row < a.n_out;
                const float4 rs = row_stat(a.rowstat, a.n_head, a.n_out, mb, h, min(row, a.n_out - 1));
                const float mv = buf_load(rm, valid ? (unsigned)(((long)row * a.ld_m + key) * 4) : a.m_bytes);
                const float p = weight_raw(mv, c, rs.x, rs.y, valid, a.masked) * rs.z;
                any = any || (p != 0.0f);
                s_w[t][l31] = p;
            }
            const unsigned long long bal = __builtin_amdgcn_ballot_w64(any);
            if (lane == 0) s_any[wave] = bal != 0ull;
            __syncthreads();
            if (wave_cols && (s_any[0] | s_any[1] | s_any[2] | s_any[3]))
                contract_tile(s_w, rg, a.dout_bytes, a.ld_dout, a.out_col0 + h * a.dim, n0, a.n_out, cb, a.dim, acc0, acc1);
            __syncthreads();
        }
    }
    if (wave_cols) {
        float* dv = a.d_values + (long)s * a.dvalues_bstride + (long)k0 * a.ld_dvalues;
        const float* res = a.d_out + (long)s * a.dout_bstride + (long)k0 * a.ld_dout;      // self attention: n_out == n_in
        const int c0 = cb + l31, c1 = cb + 32 + l31;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int ri = acc_row(r, half);
            if (ri < keys_here) {
                if (c0 < a.dim) dv[(long)ri * a.ld_dvalues + c0] = acc0[r] + (a.add_residual ? res[(long)ri * a.ld_dout + c0] : 0.0f);
                if (c1 < a.dim) dv[(long)ri * a.ld_dvalues + c1] = acc1[r] + (a.add_residual ? res[(long)ri * a.ld_dout + c1] : 0.0f);
            }
        }
    }
}

// a_i = sum_j P_ij gv_ij = g_i . out_i (out_i = sum_j P_ij v_j is the forward's result): one wave per row and head.
// grid (ceil(n_out / 4), batch, n_head)
__global__ __launch_bounds__(256) void distmat_ai_kernel(DmatArgs a) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int row = blockIdx.x * 4 + wave, s = blockIdx.y, h = blockIdx.z;
    if (row >= a.n_out) return;                           // (wave-uniform; no barriers below)
    const float* o = a.out + (long)s * a.out_bstride + (long)row * a.ld_out + a.out_col0 + (long)h * a.dim;
    const float* g = a.d_out + (long)s * a.dout_bstride + (long)row * a.ld_dout + a.out_col0 + (long)h * a.dim;
    float part = 0.0f;
    for (int d = lane; d < a.dim; d += 64) part += o[d] * g[d];
    part = wave_sum(part);
    if (lane == 0) a.a_ws[((long)s * a.n_head + h) * a.n_out + row] = part;
}

// d(m): a workgroup owns rows i0 .. i0 + 31 x keys 128 bx .. + 127 of one matrix (wave w: 32 of the keys); heads outer, the
// samples that share the matrix inner and ascending.  grid (key tiles of 128, row tiles, matrices)
__global__ __launch_bounds__(256) void distmat_dm_kernel(DmatArgs a) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, half = lane >> 5, l31 = lane & 31;
    const int j0 = blockIdx.x * 128 + wave * 32, i0 = blockIdx.y * RT, mb = blockIdx.z;
    if (j0 >= a.n_in) return;                             // (wave-uniform; no barriers below)
    const int key = j0 + l31, grow = i0 + l31;            // grow: the row whose d_out this lane feeds to the gv tiles
    const bool kv = key < a.n_in, gvalid = grow < a.n_out;
    const unsigned vbase = kv ? (unsigned)(((long)key * a.ld_values) * 4) : 0u;
    const int s_beg = a.m_bstride ? mb : 0, s_end = a.m_bstride ? mb + 1 : a.batch;
    const __amdgpu_buffer_rsrc_t rm = make_rsrc(a.m + (long)mb * a.m_bstride, a.m_bytes);
    float acc[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.0f;
    for (int h = 0; h < a.n_head; ++h) {
        const float c = head_c(a, h);
        float p[16];
        bool any = false;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int row = i0 + acc_row(r, half);
            const bool valid = kv && row < a.n_out;
            const float4 rs = row_stat(a.rowstat, a.n_head, a.n_out, mb, h, min(row, a.n_out - 1));
            const float mv = buf_load(rm, valid ? (unsigned)(((long)row * a.ld_m + key) * 4) : a.m_bytes);
            p[r] = -c * (weight_raw(mv, c, rs.x, rs.y, valid, a.masked) * rs.z);
            any = any || (p[r] != 0.0f);
        }
        if (__builtin_amdgcn_ballot_w64(any) == 0ull) continue;      // (wave-uniform)
        for (int s = s_beg; s < s_end; ++s) {
            const __amdgpu_buffer_rsrc_t rv = make_rsrc(a.values + (long)s * a.values_bstride, a.values_bytes);
            const __amdgpu_buffer_rsrc_t rg = make_rsrc(a.d_out + (long)s * a.dout_bstride, a.dout_bytes);
            const unsigned gbase = gvalid ? (unsigned)(((long)grow * a.ld_dout + a.out_col0 + (long)h * a.dim) * 4) : 0u;
            const f32x16 gv = gv_tile(rg, rv, gbase, gvalid, vbase, kv, a.dim, a.dout_bytes, a.values_bytes);
            const float* ai = a.a_ws + ((long)s * a.n_head + h) * a.n_out;
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[r] += p[r] * (gv[r] - ai[min(i0 + acc_row(r, half), a.n_out - 1)]);
        }
    }
    if (kv) {
        float* dm = a.d_m + ((long)mb * a.n_out) * a.n_in + key;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int row = i0 + acc_row(r, half);
            if (row < a.n_out) dm[(long)row * a.n_in] = acc[r];
        }
    }
}

// the matrix operands, then the layer's (pit_layer.h); fills the per-sample descriptor sizes
int dmat_check(DmatArgs& a, int need_dout) {
    if (a.batch <= 0 || a.n_out <= 0 || a.n_in <= 0) return PIT_ERR_SIZE;
    if (a.batch > 65535) return PIT_ERR_UNSUPPORTED;
    if (a.ld_m < a.n_in) return PIT_ERR_SIZE;
    const unsigned long long mbytes = rows_bytes(a.n_out, a.ld_m, a.n_in);
    if (a.m_bstride != 0 && (a.m_bstride < 0 || (unsigned long long)a.m_bstride * 4ull < mbytes)) return PIT_ERR_SIZE;
    if (mbytes > PIT_MAX_BUFFER_BYTES) return PIT_ERR_UNSUPPORTED;
    a.m_bytes = (unsigned)mbytes;
    if (int rc = layer_check_values(a, a.n_in)) return rc;
    if ((long)a.n_head * a.colgroups > 65535) return PIT_ERR_UNSUPPORTED;
    return need_dout ? layer_check_dout(a, a.n_out) : 0;
}

}  // namespace

extern "C" int pit_distmat_select_fwd(const float* m, long ld_m, long m_bstride, int mesh_batch, int n_out, int n_in,
                                      int rank_k, int need_kth, float* stats, void* stream) {
    if (!m || !stats) return PIT_ERR_NULL;
    if (mesh_batch <= 0 || n_out <= 0 || n_in <= 0 || ld_m < n_in || m_bstride < 0) return PIT_ERR_SIZE;
    if (mesh_batch > 1 && m_bstride < (long)(n_out - 1) * ld_m + n_in) return PIT_ERR_SIZE;
    if (need_kth && (rank_k < 0 || rank_k > n_in - 1)) return PIT_ERR_SIZE;
    const long rows = (long)mesh_batch * n_out;
    if (rows > 0x7fffffffL) return PIT_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(distmat_select_kernel, dim3((unsigned)rows), dim3(256), 0, (hipStream_t)stream, m, ld_m,
                       mesh_batch > 1 ? m_bstride : 0L, n_out, n_in, rank_k, need_kth, rows, stats);
    PIT_CHECK_LAUNCH();
    return 0;
}

extern "C" int pit_distmat_fwd(const float* m, long ld_m, long m_bstride, int n_out, int n_in,
                               const float* values, int batch, int dim, long ld_values, long values_bstride,
                               const float* head, int n_head, int head_is_scale,
                               const float* stats, float rank_w, int masked,
                               float* out, long ld_out, long out_bstride, int out_col0, int copy_inputs,
                               float* rowstat, float* scale_out, int math_mode, void* stream) {
    if (!m || !values || !head || !stats || !out || !rowstat) return PIT_ERR_NULL;
    if (math_mode != PIT_MATH_FP32) return PIT_ERR_UNSUPPORTED;
    DmatArgs a = DmatArgs();
    a.m = m; a.ld_m = ld_m; a.m_bstride = m_bstride; a.batch = batch; a.n_out = n_out; a.n_in = n_in; a.rank_w = rank_w;
    layer_set_fwd(a, values, dim, ld_values, values_bstride, head, n_head, head_is_scale, stats, masked, out, ld_out, out_bstride, out_col0,
                  copy_inputs, rowstat, scale_out);
    if (int rc = dmat_check(a, 0)) return rc;
    if (out_col0 < 0 || ld_out < out_col0 + (long)n_head * dim || out_bstride < 0 || (copy_inputs && (n_out != n_in || out_col0 < dim)))
        return PIT_ERR_SIZE;
    const dim3 grid((unsigned)((n_out + RT - 1) / RT), (unsigned)batch, (unsigned)(n_head * a.colgroups));
    hipLaunchKernelGGL(distmat_rows_kernel<0>, grid, dim3(256), 0, (hipStream_t)stream, a);
    PIT_CHECK_LAUNCH();
    return 0;
}

extern "C" long pit_distmat_bwd_workspace(int batch, int n_out, int n_head) {
    if (batch <= 0 || n_out <= 0 || n_head <= 0) return 0;
    return (long)batch * n_head * n_out * (long)sizeof(float);
}

extern "C" int pit_distmat_bwd(const float* m, long ld_m, long m_bstride, int n_out, int n_in,
                               const float* values, int batch, int dim, long ld_values, long values_bstride,
                               const float* head, int n_head, int head_is_scale, const float* scale,
                               const float* rowstat, int masked,
                               const float* d_out, long ld_dout, long dout_bstride, int out_col0,
                               float* d_values, long ld_dvalues, long dvalues_bstride, int add_residual,
                               float* d_head, int accumulate_head, double* workspace,
                               float* d_m, const float* out, long ld_out, long out_bstride, float* a_workspace,
                               int math_mode, void* stream) {
    if (!m || !values || !head || !rowstat || !d_out) return PIT_ERR_NULL;
    if ((d_head && !workspace) || (d_m && (!a_workspace || !out))) return PIT_ERR_NULL;
    if (math_mode != PIT_MATH_FP32) return PIT_ERR_UNSUPPORTED;
    DmatArgs a = DmatArgs();
    a.m = m; a.ld_m = ld_m; a.m_bstride = m_bstride; a.batch = batch; a.n_out = n_out; a.n_in = n_in;
    layer_set_bwd(a, values, dim, ld_values, values_bstride, head, n_head, head_is_scale, scale, rowstat, masked, d_out, ld_dout, dout_bstride,
                  out_col0, d_values, ld_dvalues, dvalues_bstride, add_residual, d_head, workspace);
    if (int rc = dmat_check(a, 1)) return rc;
    if (n_head > 65535 || (add_residual && (n_out != n_in || out_col0 < dim))) return PIT_ERR_SIZE;
    if (d_values && (ld_dvalues < dim || dvalues_bstride < 0)) return PIT_ERR_SIZE;
    a.a_ws = d_m ? a_workspace : nullptr;
    a.d_m = d_m;
    hipStream_t st = (hipStream_t)stream;
    if (d_values) {
        const dim3 grid((unsigned)((n_in + RT - 1) / RT), (unsigned)batch, (unsigned)a.colgroups);
        hipLaunchKernelGGL(distmat_dv_kernel, grid, dim3(256), 0, st, a);
        PIT_CHECK_LAUNCH();
    }
    if (d_head) {
        const dim3 grid((unsigned)((n_out + RT - 1) / RT), (unsigned)batch, (unsigned)(n_head * a.colgroups));
        hipLaunchKernelGGL(distmat_rows_kernel<1>, grid, dim3(256), 0, st, a);
        PIT_CHECK_LAUNCH();
    }
    if (d_m) {
        const unsigned row_tiles = (unsigned)((n_out + RT - 1) / RT);
        if (row_tiles > 65535u || ld_out < out_col0 + (long)n_head * dim || out_bstride < 0) return PIT_ERR_SIZE;
        a.out = const_cast<float*>(out); a.ld_out = ld_out; a.out_bstride = out_bstride;
        hipLaunchKernelGGL(distmat_ai_kernel, dim3((unsigned)((n_out + 3) / 4), (unsigned)batch, (unsigned)n_head), dim3(256), 0, st, a);
        PIT_CHECK_LAUNCH();
        const dim3 grid((unsigned)((n_in + 127) / 128), row_tiles, (unsigned)(m_bstride ? batch : 1));
        hipLaunchKernelGGL(distmat_dm_kernel, grid, dim3(256), 0, st, a);
        PIT_CHECK_LAUNCH();
    }
    return layer_finish_head(head, scale, d_head, workspace, n_head, accumulate_head, head_is_scale, stream);
}
