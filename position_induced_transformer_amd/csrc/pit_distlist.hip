// Position attention on CANDIDATE LISTS of caller-supplied squared distances (any metric, any n_in), fp32, for gfx950.
//
// pit_distmat.hip takes the layer's squared distances as a dense (n_out, n_in) matrix.  The kernels below take, per row, a list of
// `cap` slots (key, squared distance) - what a kNN, radius or truncated-Dijkstra search returns - and apply pit.py:48-57 to the
// dense matrix that holds the listed values and something large enough to be masked everywhere else:
//   S = fl(c sqd), kept iff valid and S <= T = quantile_lerp(fl(c m_(k)), fl(c m_(k+1)), w), P = exp(S_min - S) / rowsum,
// rank (k, w) from n_in, order statistics from the valid listed values.  A slot whose key is outside [0, n_in) is padding: the
// key is compared, never dereferenced, and whatever its sqd holds (NaN included) is replaced by 0 before any arithmetic.
//
//   selection   one wave per row, the row's bit patterns in registers (NPL per lane), MSB-first bitwise search by ballots.
//   forward     one wave per (sample, row); weights are formed 64 slots at a time (lane = slot) for NH heads, the kept slots are
//               broadcast by readlane in list order, four at a time, and the value row of a slot is gathered ONCE for all heads
//               (lane = value column: 256 columns per wave, further columns in further column groups).
//   d(values)   by key over the caller's transposed index (rev_ptr / rev_pos: the listing slots of a key, ascending): one wave
//               per (sample, key), no atomics.  A key listed by more than PIT_DISTLIST_CHUNK slots is summed in chunks by
//               separate waves (distlist_dv_kernel<true>) into a workspace; its wave then adds the partial rows in chunk order.
//   d(scale), d(sqd)   by row, one wave per row of a list set: gv = g . v by wave reductions,
//               d c = -sum P (sqd - mbar) gv (fp64 slots, the PIT_DSCALE_SLOTS convention), d sqd = -sum_h c_h P (gv - a), a = g . out;
//               for shared lists the samples are summed in ascending order inside the wave.
// Rows of values, d_out and out are read through sized buffer descriptors (one per sample, wave-uniform): an offset beyond the
// tensor reads 0, which is also how the tail of a group of four slots is fed.  VEC: 16-byte pieces (lane holds 4 consecutive
// columns), otherwise 4-byte pieces (lane holds columns lane, lane + 64, ...).
//
// RAGGED BATCHES (the *_ragged_* entries; RAG = true instances of the same kernels, the RAG = false instances are the code they
// were): sample s has lo = len_out[s] rows and li = len_in[s] keys, read on the device and clamped into [1, width]; per-sample
// lists only.  A slot is valid iff its key lies in [0, li); the rank (k_s, w_s) of the sample comes from li (sample_rank,
// pit_layer.h) - the selection writes w_s, the forward reads it.  A row >= lo writes zero statistics, zero head columns, zero
// rowstat and zero d_sqd and reads neither its list nor d_out; a key >= li gets a zero d_values row and its value row is never read.
// d(values) runs over the SAME transposed index as ever, built from the keys alone against the padded n_in; the lengths filter
// where the slots are read: an entry whose row is >= lo weighs 0 (its d_out row is not loaded).  Order of that sum: a key's
// entries ascend in row * cap + slot, so the entries of rows >= lo stand BEHIND those of the real rows; the real entries
// therefore fill the same places of the same 64-entry groups and PIT_DISTLIST_CHUNK-entry chunks as in a run of the trimmed cloud
// alone, and the skipped ones add +0 after them: for a key whose range - padded rows' entries included - fits one chunk the sum
// is the cloud-alone sum bit for bit.  A hub key's chunks are summed by separate waves and added in chunk order; chunks that
// hold skipped entries only add zeros.  The tests hold a hub key to a tolerance only, not to bits.
#include "pit_layer.h"

namespace {

constexpr int LQ = 4;                      // columns per lane and column group (a wave covers 64 * LQ = 256 columns)
constexpr int CHUNK = PIT_DISTLIST_CHUNK;  // listing slots of a key summed by one wave

struct ListArgs : LayerIO {
    const int* idx; const float* sqd; long ld, bstride; int cap;     // bstride 0: one list set shared by the batch
    int batch, n_out, n_in;
    float rank_w;
    const int* len_out; const int* len_in; const float* rank_w_s;    // ragged instances only: NULL length = full width; w per sample
    float* d_sqd;
    const int* rev_ptr; const int* rev_pos; const int* chunk_ptr; const int* chunk_key; float* dv_ws;
    int chunk_slots;
    unsigned out_bytes;                                              // of ONE sample's rows: the size of out's buffer descriptor
};

__device__ __forceinline__ bool key_ok(int j, int n_in) { return (unsigned)j < (unsigned)n_in; }

// column u of a lane in column group cg
template <bool VEC>
__device__ __forceinline__ int col_of(int cg, int lane, int u) { return cg * 64 * LQ + (VEC ? lane * LQ + u : u * 64 + lane); }

// the lane's LQ columns of the row that starts at byte `row_off` of the descriptor; columns >= dim and rows with row_ok = false read 0
template <bool VEC>
__device__ __forceinline__ void load_cols(__amdgpu_buffer_rsrc_t r, unsigned oob, bool row_ok, unsigned row_off, int cg, int lane, int dim,
                                          float (&v)[LQ]) {
    if (VEC) {
        const int c0 = col_of<true>(cg, lane, 0);                     // (dim % 4 == 0: a piece is inside the row or outside it)
        buf_load4(r, (row_ok && c0 < dim) ? row_off + (unsigned)c0 * 4u : oob, v);
    } else {
#pragma unroll
        for (int u = 0; u < LQ; ++u) {
            const int c = col_of<false>(cg, lane, u);
            v[u] = buf_load(r, (row_ok && c < dim) ? row_off + (unsigned)c * 4u : oob);
        }
    }
}
template <bool VEC>
__device__ __forceinline__ void store_cols(float* row, int cg, int lane, int dim, const float (&v)[LQ]) {
    if (VEC) {
        const int c0 = col_of<true>(cg, lane, 0);
        if (c0 < dim) *reinterpret_cast<float4*>(row + c0) = make_float4(v[0], v[1], v[2], v[3]);
    } else {
#pragma unroll
        for (int u = 0; u < LQ; ++u) {
            const int c = col_of<false>(cg, lane, u);
            if (c < dim) row[c] = v[u];
        }
    }
}

// ---- selection --------------------------------------------------------------------------------------------------------
// Padding holds the pattern 0xFFFFFFFF, above every candidate of the search (valid values are finite and >= 0).
// RAG: k is formed here from the sample's key count and q = fl32(locality); w goes to rank_w[s]; a row >= len_out[s] gets 0, 0, 0
template <int NPL, bool RAG>
__global__ __launch_bounds__(256) void distlist_select_kernel(const int* __restrict__ idx, const float* __restrict__ sqd, long ld, long bstride,
                                                              int cap, int n_out, int n_in, int k, int need_kth, long rows,
                                                              float* __restrict__ stats, const int* __restrict__ len_out,
                                                              const int* __restrict__ len_in, float q, float* __restrict__ rank_w) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long row = (long)blockIdx.x * 4 + wave;
    if (row >= rows) return;                              // (wave-uniform; no barriers below)
    const int s = (int)(row / n_out), i = (int)(row - (long)s * n_out);
    const long base = (long)s * bstride + (long)i * ld;
    if constexpr (RAG) {
        n_in = clamp_len(len_in, s, n_in);                // the keys of THIS sample: the rest of the kernel is the dense one
        float w;
        k = min(sample_rank(q, n_in, w), cap - 1);
        if (i == 0 && lane == 0) rank_w[s] = w;
        if (i >= clamp_len(len_out, s, n_out)) {          // padded row: defined statistics, nothing is read
            if (lane == 0) { stats[row] = 0.0f; stats[rows + row] = 0.0f; stats[2 * rows + row] = 0.0f; }
            return;
        }
    }
    uint32_t key[NPL];
    uint32_t kmin = 0xFFFFFFFFu;
#pragma unroll
    for (int u = 0; u < NPL; ++u) {
        const int t = u * 64 + lane;
        const bool in = t < cap;
        const long at = base + (in ? t : 0);
        const bool valid = in && key_ok(idx[at], n_in);
        key[u] = valid ? __float_as_uint(sqd[at]) : 0xFFFFFFFFu;
        kmin = min(kmin, key[u]);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) kmin = min(kmin, (uint32_t)__shfl_xor((int)kmin, o));
    uint32_t vk = kmin, vk1 = kmin;
    if (need_kth && kmin != 0xFFFFFFFFu) {
        uint32_t prefix = 0;
        for (int bit = 30; bit >= 0; --bit) {             // MSB-first bitwise search (distmat_select_kernel)
            const uint32_t cand = prefix | (1u << bit);
            int c = 0;
#pragma unroll
            for (int u = 0; u < NPL; ++u) c += __popcll(__builtin_amdgcn_ballot_w64(key[u] < cand));
            if (c <= k) prefix = cand;
        }
        vk = prefix;
        int cnt_le = 0;
        uint32_t next = 0xFFFFFFFFu;
#pragma unroll
        for (int u = 0; u < NPL; ++u) {
            cnt_le += __popcll(__builtin_amdgcn_ballot_w64(key[u] <= vk));
            if (key[u] > vk) next = min(next, key[u]);
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) next = min(next, (uint32_t)__shfl_xor((int)next, o));
        vk1 = (cnt_le >= k + 2 || next == 0xFFFFFFFFu) ? vk : next;      // (no valid value above: the rank is clipped)
    }
    if (kmin == 0xFFFFFFFFu) vk = vk1 = kmin = 0u;        // a row without a valid slot
    if (lane == 0) {
        stats[row] = __uint_as_float(vk);
        stats[rows + row] = __uint_as_float(vk1);
        stats[2 * rows + row] = __uint_as_float(kmin);
    }
}

// ---- the weights of 64 slots --------------------------------------------------------------------------------------------
// lane = slot t0 + lane of the row at `base`: its key (0 for padding and beyond the list), its distance (0 there) and validity
__device__ __forceinline__ bool load_slot(const ListArgs& a, int n_in, long base, int t0, int lane, int& j, float& m) {
    const int t = t0 + lane;
    const bool in = t < a.cap;
    const long at = base + (in ? t : 0);
    const int jj = a.idx[at];
    const bool valid = in && key_ok(jj, n_in);
    const float mm = a.sqd[at];
    j = valid ? jj : 0;
    m = valid ? mm : 0.0f;
    return valid;
}

// ---- forward --------------------------------------------------------------------------------------------------------------
// grid (rows / 4, head groups of NH, colgroups)
template <int NH, bool VEC, bool RAG>
__global__ __launch_bounds__(256) void distlist_fwd_kernel(ListArgs a) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long rows_all = (long)a.batch * a.n_out;
    const long wrow = (long)blockIdx.x * 4 + wave;
    if (wrow >= rows_all) return;                         // (wave-uniform; no barriers below)
    const int s = (int)(wrow / a.n_out), n = (int)(wrow - (long)s * a.n_out);
    const int h0 = blockIdx.y * NH, cg = blockIdx.z;
    const int mb = a.bstride ? s : 0;
    const long rows_total = (long)(a.bstride ? a.batch : 1) * a.n_out;
    const long srow = (long)mb * a.n_out + n;
    const long base = (long)mb * a.bstride + (long)n * a.ld;
    const __amdgpu_buffer_rsrc_t rv = make_rsrc(a.values + (long)s * a.values_bstride, a.values_bytes);
    float* orow = a.out + (long)s * a.out_bstride + (long)n * a.ld_out;

    if (a.copy_inputs && h0 == 0) {                       // torch.cat((inputs, conv), -1): the copied columns as they are
        float v[LQ];
        load_cols<VEC>(rv, a.values_bytes, true, (unsigned)((long)n * a.ld_values * 4), cg, lane, a.dim, v);
        store_cols<VEC>(orow, cg, lane, a.dim, v);
    }
    int li = a.n_in;
    float rank_w = a.rank_w;
    if constexpr (RAG) {
        li = clamp_len(a.len_in, s, a.n_in);
        rank_w = a.rank_w_s[mb];
        if (n >= clamp_len(a.len_out, s, a.n_out)) {      // padded row (wave-uniform): zeros, its list is not read
            const float z[LQ] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
            for (int q = 0; q < NH; ++q) {
                if (h0 + q >= a.n_head) continue;
                store_cols<VEC>(orow + a.out_col0 + (long)(h0 + q) * a.dim, cg, lane, a.dim, z);
                if (cg == 0 && lane == 0)
                    *reinterpret_cast<float4*>(a.rowstat + (((long)mb * a.n_head + h0 + q) * a.n_out + n) * 4) = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            }
            return;
        }
    }
    float c[NH], T[NH], smin[NH], rsum[NH], qsum[NH], acc[NH][LQ];
    bool hv[NH];
#pragma unroll
    for (int q = 0; q < NH; ++q) {
        hv[q] = h0 + q < a.n_head;
        c[q] = head_c(a, hv[q] ? h0 + q : 0);
        T[q] = a.masked ? quantile_lerp(__fmul_rn(c[q], a.stats[srow]), __fmul_rn(c[q], a.stats[rows_total + srow]), rank_w) : __builtin_inff();
        smin[q] = __fmul_rn(c[q], a.stats[2 * rows_total + srow]);
        rsum[q] = 0.0f; qsum[q] = 0.0f;
#pragma unroll
        for (int u = 0; u < LQ; ++u) acc[q][u] = 0.0f;
        if (wrow == 0 && cg == 0 && lane == 0 && hv[q] && a.scale_out) a.scale_out[h0 + q] = c[q];
    }
    for (int t0 = 0; t0 < a.cap; t0 += 64) {
        int j; float m;
        const bool valid = load_slot(a, li, base, t0, lane, j, m);
        float p[NH];
        bool any = false;
#pragma unroll
        for (int q = 0; q < NH; ++q) {
            p[q] = weight_raw(m, c[q], T[q], smin[q], valid && hv[q], a.masked);
            rsum[q] += p[q]; qsum[q] += p[q] * m;
            any = any || p[q] != 0.0f;
        }
        unsigned long long mask = __builtin_amdgcn_ballot_w64(any);
        while (mask) {                                    // four kept slots per turn: their gathers are in flight together
            float v[4][LQ], pw[4][NH];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const bool on = mask != 0ull;
                const int src = on ? __builtin_ctzll(mask) : 0;
                mask &= mask - 1ull;                      // (0 stays 0)
                const int jj = __builtin_amdgcn_readlane(j, src);
#pragma unroll
                for (int q = 0; q < NH; ++q) pw[e][q] = on ? lane_f(p[q], src) : 0.0f;
                load_cols<VEC>(rv, a.values_bytes, on, (unsigned)((long)jj * a.ld_values * 4), cg, lane, a.dim, v[e]);
            }
#pragma unroll
            for (int e = 0; e < 4; ++e)
#pragma unroll
                for (int q = 0; q < NH; ++q)
#pragma unroll
                    for (int u = 0; u < LQ; ++u) acc[q][u] += pw[e][q] * v[e][u];
        }
    }
#pragma unroll
    for (int q = 0; q < NH; ++q) {
        if (!hv[q]) continue;                             // (wave-uniform)
        const float rs = wave_sum(rsum[q]), qs = wave_sum(qsum[q]);
        const float inv = rs > 0.0f ? 1.0f / rs : 0.0f;
        float o[LQ];
#pragma unroll
        for (int u = 0; u < LQ; ++u) o[u] = acc[q][u] * inv;
        store_cols<VEC>(orow + a.out_col0 + (long)(h0 + q) * a.dim, cg, lane, a.dim, o);
        if (cg == 0 && lane == 0 && (a.bstride || s == 0))
            *reinterpret_cast<float4*>(a.rowstat + (((long)mb * a.n_head + h0 + q) * a.n_out + n) * 4) =
                rs > 0.0f ? make_float4(T[q], smin[q], inv, qs * inv) : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    }
}

// ---- d(values) --------------------------------------------------------------------------------------------------------------
// acc += sum over the entries e0 .. e1 - 1 of rev_pos (list set mb), ascending, and over the heads, of P g: 64 entries at a time
// (lane = entry), per head the entries with a weight are broadcast in order, four at a time.
// RAG: `li` keys count and the entries of rows >= `lo` weigh 0 (the dense instances pass n_in and do not look at `lo`).
template <bool VEC, bool RAG>
__device__ __forceinline__ void dv_range(const ListArgs& a, int mb, int li, int lo, __amdgpu_buffer_rsrc_t rg, const int* rev_pos, int e0, int e1,
                                         int cg, int lane, float (&acc)[LQ]) {
    const long slots = (long)a.n_out * a.cap;
    for (int eb = e0; eb < e1; eb += 64) {
        const int e = eb + lane;
        const bool ev = e < e1;
        long pos = ev ? rev_pos[e] : 0;
        pos = pos < 0 ? 0 : (pos > slots - 1 ? slots - 1 : pos);
        const int row = (int)(pos / a.cap), slot = (int)(pos - (long)row * a.cap);
        const long at = (long)mb * a.bstride + (long)row * a.ld + slot;
        const bool valid = ev && key_ok(a.idx[at], li) && (!RAG || row < lo);
        const float mm = a.sqd[at];
        const float m = valid ? mm : 0.0f;
        for (int h = 0; h < a.n_head; ++h) {
            const float c = head_c(a, h);
            const float4 rs = row_stat(a.rowstat, a.n_head, a.n_out, mb, h, row);
            const float p = weight_raw(m, c, rs.x, rs.y, valid, a.masked) * rs.z;
            unsigned long long mask = __builtin_amdgcn_ballot_w64(p != 0.0f);
            const unsigned hoff = (unsigned)((a.out_col0 + (long)h * a.dim) * 4);
            while (mask) {
                float g[4][LQ], pw[4];
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const bool on = mask != 0ull;
                    const int src = on ? __builtin_ctzll(mask) : 0;
                    mask &= mask - 1ull;
                    const int rr = __builtin_amdgcn_readlane(row, src);
                    pw[q] = on ? lane_f(p, src) : 0.0f;
                    load_cols<VEC>(rg, a.dout_bytes, on, (unsigned)((long)rr * a.ld_dout * 4) + hoff, cg, lane, a.dim, g[q]);
                }
#pragma unroll
                for (int q = 0; q < 4; ++q)
#pragma unroll
                    for (int u = 0; u < LQ; ++u) acc[u] += pw[q] * g[q][u];
            }
        }
    }
}

// HUB = false: one wave per (sample, key): a range of up to CHUNK entries is summed here, a longer one from its partial rows in
//              chunk order; + the residual; writes d_values.  grid (keys / 4, batch, colgroups)
// HUB = true:  one wave per (sample, chunk slot): the slot's CHUNK entries of its key into the workspace.
//              grid (chunk slots / 4, batch, colgroups)
template <bool HUB, bool VEC, bool RAG>
__global__ __launch_bounds__(256) void distlist_dv_kernel(ListArgs a) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int item = blockIdx.x * 4 + wave, s = blockIdx.y, cg = blockIdx.z;
    if (item >= (HUB ? a.chunk_slots : a.n_in)) return;   // (wave-uniform; no barriers below)
    const int mb = a.bstride ? s : 0;
    const int entries = (int)((long)a.n_out * a.cap);
    const int* rev_ptr = a.rev_ptr + (long)mb * (a.n_in + 1);
    const int* rev_pos = a.rev_pos + (long)mb * entries;
    const int* chunk_ptr = a.chunk_ptr + (long)mb * (a.n_in + 1);
    const __amdgpu_buffer_rsrc_t rg = make_rsrc(a.d_out + (long)s * a.dout_bstride, a.dout_bytes);
    const long wcols = (long)a.colgroups * 64 * LQ;       // floats of a partial row
    float acc[LQ] = {0.0f, 0.0f, 0.0f, 0.0f};
    int key = item;
    if (HUB) {
        key = a.chunk_key[(long)mb * a.chunk_slots + item];
        if (!key_ok(key, a.n_in)) return;                 // a free slot
    }
    int li = a.n_in, lo = a.n_out;
    if constexpr (RAG) {
        li = clamp_len(a.len_in, s, a.n_in);
        lo = clamp_len(a.len_out, s, a.n_out);
        if (key >= li) {                                  // a padding key (wave-uniform): a zero row; its chunks are never read
            if (!HUB) store_cols<VEC>(a.d_values + (long)s * a.dvalues_bstride + (long)key * a.ld_dvalues, cg, lane, a.dim, acc);
            return;
        }
    }
    const int r0 = min(max(rev_ptr[key], 0), entries), r1 = min(max(rev_ptr[key + 1], r0), entries);
    if (HUB) {
        const int ch = item - chunk_ptr[key];
        const int e0 = (ch >= 0 && ch < (r1 - r0 + CHUNK - 1) / CHUNK) ? r0 + ch * CHUNK : r1;
        dv_range<VEC, RAG>(a, mb, li, lo, rg, rev_pos, e0, min(e0 + CHUNK, r1), cg, lane, acc);
        float* w = a.dv_ws + ((long)s * a.chunk_slots + item) * wcols + (long)cg * 64 * LQ;
#pragma unroll
        for (int u = 0; u < LQ; ++u) w[VEC ? lane * LQ + u : u * 64 + lane] = acc[u];
        return;
    }
    if (r1 - r0 <= CHUNK) {
        dv_range<VEC, RAG>(a, mb, li, lo, rg, rev_pos, r0, r1, cg, lane, acc);
    } else {
        const int c0 = min(max(chunk_ptr[key], 0), a.chunk_slots), c1 = min(max(chunk_ptr[key + 1], c0), a.chunk_slots);
        for (int ch = c0; ch < c1; ++ch) {
            const float* w = a.dv_ws + ((long)s * a.chunk_slots + ch) * wcols + (long)cg * 64 * LQ;
#pragma unroll
            for (int u = 0; u < LQ; ++u) acc[u] += w[VEC ? lane * LQ + u : u * 64 + lane];
        }
    }
    if (a.add_residual && (!RAG || key < lo)) {           // self attention: n_out == n_in (ragged: the d_out of a padded row is never read)
        float r[LQ];
        load_cols<VEC>(rg, a.dout_bytes, true, (unsigned)((long)key * a.ld_dout * 4), cg, lane, a.dim, r);
#pragma unroll
        for (int u = 0; u < LQ; ++u) acc[u] += r[u];
    }
    store_cols<VEC>(a.d_values + (long)s * a.dvalues_bstride + (long)key * a.ld_dvalues, cg, lane, a.dim, acc);
}

// ---- d(scale) and d(sqd) ------------------------------------------------------------------------------------------------------
// One wave per row of a list set; 64 slots at a time (lane = slot), inside them the samples that use the list set, ascending, then the
// heads in groups of NH.  The value row of a kept slot is gathered once per head group.  grid (list rows / 4)
template <int NH, bool VEC, bool RAG>
__global__ __launch_bounds__(256) void distlist_rows_bwd_kernel(ListArgs a) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long rows_total = (long)(a.bstride ? a.batch : 1) * a.n_out;
    const long srow = (long)blockIdx.x * 4 + wave;
    if (srow >= rows_total) return;                       // (wave-uniform; no barriers below)
    const int mb = (int)(srow / a.n_out), n = (int)(srow - (long)mb * a.n_out);
    const int s_beg = a.bstride ? mb : 0, s_end = a.bstride ? mb + 1 : a.batch;
    const long base = (long)mb * a.bstride + (long)n * a.ld;
    const bool need_a = a.d_sqd != nullptr;
    int li = a.n_in;
    if constexpr (RAG) {                                  // (per-sample lists: mb is the sample)
        li = clamp_len(a.len_in, s_beg, a.n_in);
        if (n >= clamp_len(a.len_out, s_beg, a.n_out)) {  // padded row (wave-uniform): no d(scale), a zero d_sqd row
            if (a.d_sqd)
                for (int t = lane; t < a.cap; t += 64) a.d_sqd[srow * a.cap + t] = 0.0f;
            return;
        }
    }
    for (int t0 = 0; t0 < a.cap; t0 += 64) {
        int j; float m;
        const bool valid = load_slot(a, li, base, t0, lane, j, m);
        float dsq = 0.0f;
        for (int s = s_beg; s < s_end; ++s) {
            const __amdgpu_buffer_rsrc_t rv = make_rsrc(a.values + (long)s * a.values_bstride, a.values_bytes);
            const __amdgpu_buffer_rsrc_t rg = make_rsrc(a.d_out + (long)s * a.dout_bstride, a.dout_bytes);
            const __amdgpu_buffer_rsrc_t ro = make_rsrc(a.out + (long)(need_a ? s : 0) * a.out_bstride, need_a ? a.out_bytes : 0u);
            for (int h0 = 0; h0 < a.n_head; h0 += NH) {
                float c[NH], p[NH], mbar[NH], ai[NH], gvl[NH], g0[NH][LQ];
                unsigned goff[NH];
                bool any = false;
#pragma unroll
                for (int q = 0; q < NH; ++q) {
                    const bool hv = h0 + q < a.n_head;
                    const int h = hv ? h0 + q : 0;
                    c[q] = head_c(a, h);
                    const float4 rs = row_stat(a.rowstat, a.n_head, a.n_out, mb, h, n);
                    p[q] = weight_raw(m, c[q], rs.x, rs.y, valid && hv, a.masked) * rs.z;
                    mbar[q] = rs.w;
                    any = any || p[q] != 0.0f;
                    goff[q] = (unsigned)(((long)n * a.ld_dout + a.out_col0 + (long)h * a.dim) * 4);
                    load_cols<VEC>(rg, a.dout_bytes, hv, goff[q], 0, lane, a.dim, g0[q]);      // g_i, column group 0
                    gvl[q] = 0.0f;
                    float part = 0.0f;
                    if (need_a)                              // a_i = g_i . out_i
                        for (int cg = 0; cg < a.colgroups; ++cg) {
                            float o[LQ], g[LQ];
                            load_cols<VEC>(ro, a.out_bytes, hv, (unsigned)(((long)n * a.ld_out + a.out_col0 + (long)h * a.dim) * 4), cg, lane, a.dim, o);
                            if (cg == 0) {
#pragma unroll
                                for (int u = 0; u < LQ; ++u) g[u] = g0[q][u];
                            } else load_cols<VEC>(rg, a.dout_bytes, hv, goff[q], cg, lane, a.dim, g);
#pragma unroll
                            for (int u = 0; u < LQ; ++u) part += o[u] * g[u];
                        }
                    ai[q] = need_a ? wave_sum(part) : 0.0f;
                }
                unsigned long long mask = __builtin_amdgcn_ballot_w64(any);
                while (mask) {                            // gv of the kept slots, four at a time
                    float part[4][NH];
                    int src[4];
                    bool on[4];
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        on[e] = mask != 0ull;
                        src[e] = on[e] ? __builtin_ctzll(mask) : 0;
                        mask &= mask - 1ull;
#pragma unroll
                        for (int q = 0; q < NH; ++q) part[e][q] = 0.0f;
                    }
                    for (int cg = 0; cg < a.colgroups; ++cg) {
                        float v[4][LQ];
#pragma unroll
                        for (int e = 0; e < 4; ++e) {
                            const int jj = __builtin_amdgcn_readlane(j, src[e]);
                            load_cols<VEC>(rv, a.values_bytes, on[e], (unsigned)((long)jj * a.ld_values * 4), cg, lane, a.dim, v[e]);
                        }
#pragma unroll
                        for (int q = 0; q < NH; ++q) {
                            float g[LQ];
                            if (cg == 0) {
#pragma unroll
                                for (int u = 0; u < LQ; ++u) g[u] = g0[q][u];
                            } else load_cols<VEC>(rg, a.dout_bytes, h0 + q < a.n_head, goff[q], cg, lane, a.dim, g);
#pragma unroll
                            for (int e = 0; e < 4; ++e)
#pragma unroll
                                for (int u = 0; u < LQ; ++u) part[e][q] += g[u] * v[e][u];
                        }
                    }
#pragma unroll
                    for (int e = 0; e < 4; ++e)
#pragma unroll
                        for (int q = 0; q < NH; ++q) {
                            const float gv = wave_sum(part[e][q]);
                            if (on[e] && lane == src[e]) gvl[q] = gv;
                        }
                }
#pragma unroll
                for (int q = 0; q < NH; ++q) {
                    if (h0 + q >= a.n_head) continue;     // (wave-uniform)
                    dsq += -c[q] * (p[q] * (gvl[q] - ai[q]));
                    if (a.dscale_acc) {                   // d c = -sum P (sqd - mbar) gv
                        const double part = wave_sum_d((double)(p[q] * (m - mbar[q])) * (double)gvl[q]);
                        const int slot = (int)((blockIdx.x + 131u * (unsigned)s + 977u * (unsigned)(wave + 4 * (t0 >> 6))) & (PIT_DSCALE_SLOTS - 1));
                        if (lane == 0) atomicAdd(a.dscale_acc + (long)(h0 + q) * PIT_DSCALE_SLOTS + slot, -part);
                    }
                }
            }
        }
        if (a.d_sqd && t0 + lane < a.cap) a.d_sqd[srow * a.cap + t0 + lane] = dsq;
    }
}

bool aligned4(const void* p, long a = 0, long b = 0, long c = 0, long d = 0) {
    return (reinterpret_cast<uintptr_t>(p) & 15u) == 0 && ((a | b | c | d) & 3L) == 0;
}

// the list operands, then the layer's (pit_layer.h); fills the per-sample descriptor sizes
int list_check(ListArgs& a, int need_dout) {
    if (a.batch <= 0 || a.n_out <= 0 || a.n_in <= 0 || a.cap <= 0) return PIT_ERR_SIZE;
    if (a.batch > 65535) return PIT_ERR_UNSUPPORTED;
    if (a.ld < a.cap || a.bstride < 0 || (a.bstride != 0 && a.bstride < (long)(a.n_out - 1) * a.ld + a.cap)) return PIT_ERR_SIZE;
    if ((long)a.n_out * a.cap > 0x7fffffffL || (long)a.batch * a.n_out > 0x7fffffffL) return PIT_ERR_UNSUPPORTED;
    if (int rc = layer_check_values(a, a.n_in)) return rc;
    if (a.n_head > 65535 || a.colgroups > 65535) return PIT_ERR_UNSUPPORTED;
    return need_dout ? layer_check_dout(a, std::max(a.n_out, a.add_residual ? a.n_in : 0)) : 0;
}

// what the ragged entries add to the dense ones' operands (rag = false: the dense entry, the rest is unused)
struct RagLens { bool rag; const int* len_out; const int* len_in; };

template <int NPL>
void launch_select(const int* idx, const float* sqd, long ld, long bstride, int cap, int n_out, int n_in, int k, int need_kth, long rows,
                   float* stats, const RagLens& r, float q, float* rank_w, hipStream_t st) {
    const dim3 grid((unsigned)((rows + 3) / 4));
    if (r.rag)
        hipLaunchKernelGGL((distlist_select_kernel<NPL, true>), grid, dim3(256), 0, st, idx, sqd, ld, bstride, cap, n_out, n_in, k, need_kth, rows,
                           stats, r.len_out, r.len_in, q, rank_w);
    else
        hipLaunchKernelGGL((distlist_select_kernel<NPL, false>), grid, dim3(256), 0, st, idx, sqd, ld, bstride, cap, n_out, n_in, k, need_kth, rows,
                           stats, nullptr, nullptr, 0.0f, nullptr);
}

// rag: rank_k is the rank of the padded width (the largest a sample can have) - what the width of the lists is checked against
int list_select(const int* idx, const float* sqd, long ld, long bstride, int cap, int mesh_batch, int n_out, int n_in, int rank_k, int need_kth,
                float* stats, const RagLens& r, float q, float* rank_w, void* stream) {
    if (!idx || !sqd || !stats || (r.rag && !rank_w)) return PIT_ERR_NULL;
    if (mesh_batch <= 0 || n_out <= 0 || n_in <= 0 || cap <= 0 || ld < cap || bstride < 0) return PIT_ERR_SIZE;
    if (mesh_batch > 1 && bstride < (long)(n_out - 1) * ld + cap) return PIT_ERR_SIZE;
    if (need_kth && (rank_k < 0 || rank_k > cap - 1)) return PIT_ERR_SIZE;
    if (cap > PIT_DISTLIST_MAX_CAP) return PIT_ERR_UNSUPPORTED;
    const long rows = (long)mesh_batch * n_out;
    if (rows > 0x7fffffffL) return PIT_ERR_UNSUPPORTED;
    const long bs = mesh_batch > 1 ? bstride : 0L;
    hipStream_t st = (hipStream_t)stream;
    const int npl = (cap + 63) / 64;
    if (npl <= 1) launch_select<1>(idx, sqd, ld, bs, cap, n_out, n_in, rank_k, need_kth, rows, stats, r, q, rank_w, st);
    else if (npl <= 2) launch_select<2>(idx, sqd, ld, bs, cap, n_out, n_in, rank_k, need_kth, rows, stats, r, q, rank_w, st);
    else if (npl <= 4) launch_select<4>(idx, sqd, ld, bs, cap, n_out, n_in, rank_k, need_kth, rows, stats, r, q, rank_w, st);
    else if (npl <= 8) launch_select<8>(idx, sqd, ld, bs, cap, n_out, n_in, rank_k, need_kth, rows, stats, r, q, rank_w, st);
    else if (npl <= 16) launch_select<16>(idx, sqd, ld, bs, cap, n_out, n_in, rank_k, need_kth, rows, stats, r, q, rank_w, st);
    else launch_select<32>(idx, sqd, ld, bs, cap, n_out, n_in, rank_k, need_kth, rows, stats, r, q, rank_w, st);
    PIT_CHECK_LAUNCH();
    return 0;
}

// ragged batches run on per-sample lists only (a batch of one has one list set whatever its stride says)
bool rag_lists_ok(long bstride, int batch) { return bstride != 0 || batch == 1; }

int list_fwd(const int* idx, const float* sqd, long ld, long bstride, int cap, int n_out, int n_in,
             const float* values, int batch, int dim, long ld_values, long values_bstride,
             const float* head, int n_head, int head_is_scale,
             const float* stats, float rank_w, const float* rank_w_s, const RagLens& r, int masked,
             float* out, long ld_out, long out_bstride, int out_col0, int copy_inputs,
             float* rowstat, float* scale_out, int math_mode, void* stream) {
    if (!idx || !sqd || !values || !head || !stats || !out || !rowstat || (r.rag && !rank_w_s)) return PIT_ERR_NULL;
    if (math_mode != PIT_MATH_FP32) return PIT_ERR_UNSUPPORTED;
    if (r.rag && !rag_lists_ok(bstride, batch)) return PIT_ERR_SIZE;
    ListArgs a = ListArgs();
    a.idx = idx; a.sqd = sqd; a.ld = ld; a.bstride = bstride; a.cap = cap; a.batch = batch; a.n_out = n_out; a.n_in = n_in;
    a.rank_w = rank_w;
    a.len_out = r.len_out; a.len_in = r.len_in; a.rank_w_s = rank_w_s;
    layer_set_fwd(a, values, dim, ld_values, values_bstride, head, n_head, head_is_scale, stats, masked, out, ld_out, out_bstride, out_col0,
                  copy_inputs, rowstat, scale_out);
    if (int rc = list_check(a, 0)) return rc;
    if (out_col0 < 0 || ld_out < out_col0 + (long)n_head * dim || out_bstride < 0 || (copy_inputs && (n_out != n_in || out_col0 < dim)))
        return PIT_ERR_SIZE;
    if (rows_bytes(n_out, ld_out, out_col0 + (long)n_head * dim) > PIT_MAX_BUFFER_BYTES) return PIT_ERR_UNSUPPORTED;
    const bool vec = dim % 4 == 0 && aligned4(values, ld_values, values_bstride) && aligned4(out, ld_out, out_bstride, out_col0);
    const int nh = n_head == 1 ? 1 : n_head == 2 ? 2 : 4;
    const dim3 grid((unsigned)(((long)batch * n_out + 3) / 4), (unsigned)((n_head + nh - 1) / nh), (unsigned)a.colgroups);
    hipStream_t st = (hipStream_t)stream;
#define PIT_LIST_FWD2(NH_, RAG_) do { if (vec) hipLaunchKernelGGL((distlist_fwd_kernel<NH_, true, RAG_>), grid, dim3(256), 0, st, a); \
                                      else hipLaunchKernelGGL((distlist_fwd_kernel<NH_, false, RAG_>), grid, dim3(256), 0, st, a); } while (0)
#define PIT_LIST_FWD(NH_) do { if (r.rag) PIT_LIST_FWD2(NH_, true); else PIT_LIST_FWD2(NH_, false); } while (0)
    if (nh == 1) PIT_LIST_FWD(1); else if (nh == 2) PIT_LIST_FWD(2); else PIT_LIST_FWD(4);
#undef PIT_LIST_FWD
#undef PIT_LIST_FWD2
    PIT_CHECK_LAUNCH();
    return 0;
}

}  // namespace

extern "C" int pit_distlist_select_fwd(const int* idx, const float* sqd, long ld, long bstride, int cap, int mesh_batch, int n_out, int n_in,
                                       int rank_k, int need_kth, float* stats, void* stream) {
    return list_select(idx, sqd, ld, bstride, cap, mesh_batch, n_out, n_in, rank_k, need_kth, stats, RagLens{false, nullptr, nullptr}, 0.0f,
                       nullptr, stream);
}

extern "C" int pit_distlist_select_ragged_fwd(const int* idx, const float* sqd, long ld, long bstride, int cap, int mesh_batch, int n_out,
                                              int n_in, float locality, int need_kth, const int* len_out, const int* len_in, float* stats,
                                              float* rank_w, void* stream) {
    if (!(locality >= 0.0f && locality <= 1.0f)) return PIT_ERR_SIZE;
    // the rank of the padded width bounds every sample's (ops.quantile_rank's arithmetic, here on the host)
    const int k_max = n_in > 0 ? (int)floorf(locality * (float)(n_in - 1)) : 0;
    return list_select(idx, sqd, ld, bstride, cap, mesh_batch, n_out, n_in, k_max, need_kth, stats, RagLens{true, len_out, len_in}, locality,
                       rank_w, stream);
}

extern "C" int pit_distlist_fwd(const int* idx, const float* sqd, long ld, long bstride, int cap, int n_out, int n_in,
                                const float* values, int batch, int dim, long ld_values, long values_bstride,
                                const float* head, int n_head, int head_is_scale,
                                const float* stats, float rank_w, int masked,
                                float* out, long ld_out, long out_bstride, int out_col0, int copy_inputs,
                                float* rowstat, float* scale_out, int math_mode, void* stream) {
    return list_fwd(idx, sqd, ld, bstride, cap, n_out, n_in, values, batch, dim, ld_values, values_bstride, head, n_head, head_is_scale, stats,
                    rank_w, nullptr, RagLens{false, nullptr, nullptr}, masked, out, ld_out, out_bstride, out_col0, copy_inputs, rowstat,
                    scale_out, math_mode, stream);
}

extern "C" int pit_distlist_ragged_fwd(const int* idx, const float* sqd, long ld, long bstride, int cap, int n_out, int n_in,
                                       const float* values, int batch, int dim, long ld_values, long values_bstride,
                                       const float* head, int n_head, int head_is_scale,
                                       const float* stats, const float* rank_w, int masked,
                                       const int* len_out, const int* len_in,
                                       float* out, long ld_out, long out_bstride, int out_col0, int copy_inputs,
                                       float* rowstat, float* scale_out, int math_mode, void* stream) {
    return list_fwd(idx, sqd, ld, bstride, cap, n_out, n_in, values, batch, dim, ld_values, values_bstride, head, n_head, head_is_scale, stats,
                    0.0f, rank_w, RagLens{true, len_out, len_in}, masked, out, ld_out, out_bstride, out_col0, copy_inputs, rowstat, scale_out,
                    math_mode, stream);
}

extern "C" long pit_distlist_bwd_workspace(int batch, int n_out, int cap, int dim) {
    if (batch <= 0 || n_out <= 0 || cap <= 0 || dim <= 0) return 0;
    const long colgroups = (dim + 64 * LQ - 1) / (64 * LQ);
    return (long)batch * PIT_DISTLIST_CHUNK_SLOTS(n_out, cap) * colgroups * 64 * LQ * (long)sizeof(float);
}

namespace {

int list_bwd(const int* idx, const float* sqd, long ld, long bstride, int cap, int n_out, int n_in,
             const float* values, int batch, int dim, long ld_values, long values_bstride,
             const float* head, int n_head, int head_is_scale, const float* scale,
             const float* rowstat, int masked, const RagLens& r,
             const float* d_out, long ld_dout, long dout_bstride, int out_col0,
             float* d_values, long ld_dvalues, long dvalues_bstride, int add_residual,
             float* d_head, int accumulate_head, double* workspace,
             float* d_sqd, const float* out, long ld_out, long out_bstride,
             const int* rev_ptr, const int* rev_pos, const int* chunk_ptr, const int* chunk_key, float* dv_workspace,
             int math_mode, void* stream) {
    if (!idx || !sqd || !values || !head || !rowstat || !d_out) return PIT_ERR_NULL;
    if ((d_head && !workspace) || (d_sqd && !out)) return PIT_ERR_NULL;
    if (d_values && (!rev_ptr || !rev_pos || !chunk_ptr || !chunk_key || !dv_workspace)) return PIT_ERR_NULL;
    if (math_mode != PIT_MATH_FP32) return PIT_ERR_UNSUPPORTED;
    if (r.rag && !rag_lists_ok(bstride, batch)) return PIT_ERR_SIZE;
    ListArgs a = ListArgs();
    a.idx = idx; a.sqd = sqd; a.ld = ld; a.bstride = bstride; a.cap = cap; a.batch = batch; a.n_out = n_out; a.n_in = n_in;
    a.len_out = r.len_out; a.len_in = r.len_in;
    layer_set_bwd(a, values, dim, ld_values, values_bstride, head, n_head, head_is_scale, scale, rowstat, masked, d_out, ld_dout, dout_bstride,
                  out_col0, d_values, ld_dvalues, dvalues_bstride, add_residual, d_head, workspace);
    if (add_residual && (n_out != n_in || out_col0 < dim)) return PIT_ERR_SIZE;
    if (int rc = list_check(a, 1)) return rc;
    if (d_values && (ld_dvalues < dim || dvalues_bstride < 0)) return PIT_ERR_SIZE;
    a.d_sqd = d_sqd;
    a.rev_ptr = rev_ptr; a.rev_pos = rev_pos; a.chunk_ptr = chunk_ptr; a.chunk_key = chunk_key; a.dv_ws = dv_workspace;
    const long slots = PIT_DISTLIST_CHUNK_SLOTS(n_out, cap);
    a.chunk_slots = (int)slots;
    bool vec = dim % 4 == 0 && aligned4(values, ld_values, values_bstride) && aligned4(d_out, ld_dout, dout_bstride, out_col0);
    if (d_values) vec = vec && aligned4(d_values, ld_dvalues, dvalues_bstride);
    if (d_sqd) {
        if (ld_out < out_col0 + (long)n_head * dim || out_bstride < 0) return PIT_ERR_SIZE;
        const unsigned long long ob = rows_bytes(n_out, ld_out, out_col0 + (long)n_head * dim);
        if (ob > PIT_MAX_BUFFER_BYTES) return PIT_ERR_UNSUPPORTED;
        a.out = const_cast<float*>(out); a.ld_out = ld_out; a.out_bstride = out_bstride; a.out_bytes = (unsigned)ob;
        vec = vec && aligned4(out, ld_out, out_bstride);
    }
    hipStream_t st = (hipStream_t)stream;
    if (d_values) {
        const dim3 hub((unsigned)((slots + 3) / 4), (unsigned)batch, (unsigned)a.colgroups);
        const dim3 grid((unsigned)((n_in + 3) / 4), (unsigned)batch, (unsigned)a.colgroups);
#define PIT_LIST_DV(VEC_, RAG_) do { hipLaunchKernelGGL((distlist_dv_kernel<true, VEC_, RAG_>), hub, dim3(256), 0, st, a); \
                                     hipLaunchKernelGGL((distlist_dv_kernel<false, VEC_, RAG_>), grid, dim3(256), 0, st, a); } while (0)
        if (r.rag) { if (vec) PIT_LIST_DV(true, true); else PIT_LIST_DV(false, true); }
        else       { if (vec) PIT_LIST_DV(true, false); else PIT_LIST_DV(false, false); }
#undef PIT_LIST_DV
        PIT_CHECK_LAUNCH();
    }
    if (d_head || d_sqd) {
        const long rows = (long)(bstride ? batch : 1) * n_out;
        const dim3 grid((unsigned)((rows + 3) / 4));
        const int nh = n_head == 1 ? 1 : n_head == 2 ? 2 : 4;
#define PIT_LIST_ROWS2(NH_, RAG_) do { if (vec) hipLaunchKernelGGL((distlist_rows_bwd_kernel<NH_, true, RAG_>), grid, dim3(256), 0, st, a); \
                                       else hipLaunchKernelGGL((distlist_rows_bwd_kernel<NH_, false, RAG_>), grid, dim3(256), 0, st, a); } while (0)
#define PIT_LIST_ROWS(NH_) do { if (r.rag) PIT_LIST_ROWS2(NH_, true); else PIT_LIST_ROWS2(NH_, false); } while (0)
        if (nh == 1) PIT_LIST_ROWS(1); else if (nh == 2) PIT_LIST_ROWS(2); else PIT_LIST_ROWS(4);
#undef PIT_LIST_ROWS
#undef PIT_LIST_ROWS2
        PIT_CHECK_LAUNCH();
    }
    return layer_finish_head(head, scale, d_head, workspace, n_head, accumulate_head, head_is_scale, stream);
}

}  // namespace

extern "C" int pit_distlist_bwd(const int* idx, const float* sqd, long ld, long bstride, int cap, int n_out, int n_in,
                                const float* values, int batch, int dim, long ld_values, long values_bstride,
                                const float* head, int n_head, int head_is_scale, const float* scale,
                                const float* rowstat, int masked,
                                const float* d_out, long ld_dout, long dout_bstride, int out_col0,
                                float* d_values, long ld_dvalues, long dvalues_bstride, int add_residual,
                                float* d_head, int accumulate_head, double* workspace,
                                float* d_sqd, const float* out, long ld_out, long out_bstride,
                                const int* rev_ptr, const int* rev_pos, const int* chunk_ptr, const int* chunk_key, float* dv_workspace,
                                int math_mode, void* stream) {
    return list_bwd(idx, sqd, ld, bstride, cap, n_out, n_in, values, batch, dim, ld_values, values_bstride, head, n_head, head_is_scale, scale,
                    rowstat, masked, RagLens{false, nullptr, nullptr}, d_out, ld_dout, dout_bstride, out_col0, d_values, ld_dvalues,
                    dvalues_bstride, add_residual, d_head, accumulate_head, workspace, d_sqd, out, ld_out, out_bstride, rev_ptr, rev_pos,
                    chunk_ptr, chunk_key, dv_workspace, math_mode, stream);
}

extern "C" int pit_distlist_ragged_bwd(const int* idx, const float* sqd, long ld, long bstride, int cap, int n_out, int n_in,
                                       const float* values, int batch, int dim, long ld_values, long values_bstride,
                                       const float* head, int n_head, int head_is_scale, const float* scale,
                                       const float* rowstat, int masked,
                                       const int* len_out, const int* len_in,
                                       const float* d_out, long ld_dout, long dout_bstride, int out_col0,
                                       float* d_values, long ld_dvalues, long dvalues_bstride, int add_residual,
                                       float* d_head, int accumulate_head, double* workspace,
                                       float* d_sqd, const float* out, long ld_out, long out_bstride,
                                       const int* rev_ptr, const int* rev_pos, const int* chunk_ptr, const int* chunk_key,
                                       float* dv_workspace, int math_mode, void* stream) {
    return list_bwd(idx, sqd, ld, bstride, cap, n_out, n_in, values, batch, dim, ld_values, values_bstride, head, n_head, head_is_scale, scale,
                    rowstat, masked, RagLens{true, len_out, len_in}, d_out, ld_dout, dout_bstride, out_col0, d_values, ld_dvalues,
                    dvalues_bstride, add_residual, d_head, accumulate_head, workspace, d_sqd, out, ld_out, out_bstride, rev_ptr, rev_pos,
                    chunk_ptr, chunk_key, dv_workspace, math_mode, stream);
}
