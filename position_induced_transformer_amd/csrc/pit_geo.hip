// The k nearest keys of every row under the path length of a graph (include/pit_hip.h, pit_geo_knn): the neighbour lists of the
// any-metric layers where the metric is a geodesic - a truncated single-source shortest-path search per row.
//
// One wavefront per row, one wavefront per workgroup; everything a row knows lives in LDS (sized at the launch from `reach`):
//   s_vert[e], s_len[e]   the DISCOVERED vertices in the order of their discovery, e < count <= reach: the vertex (its
//                         complement once it is settled) and the bits of its tentative length (lengths >= 0 order as unsigned
//                         integers; -0.0 is stored as +0.0);
//   s_hash[]              open addressing, a power of two >= 2 * reach slots of 16 bits: e + 1 of the vertex hashed there, 0 = empty.
// A step: the least (length, vertex) among the unsettled entries by a lane-strided scan and a wave reduction; the completion
// test; the vertex is settled; its adjacency row is read a lane per edge, an edge to a discovered vertex lowers that vertex's
// length by an LDS atomic min, edges to new vertices are appended by lane 0 one by one (which looks the vertex up again: an
// earlier edge of the same row may have brought it).  An append that would make the discovered set larger than `reach` ends the
// row as truncated.  At the end the settled key vertices are compacted to the front of the two arrays, sorted by
// (length, vertex) - a vertex discovered at a settled length may have a lower index than one settled before it - and cut at k.
// Every loop is bounded by reach, n_edge or k; no global atomics, nothing shared between workgroups.
#include "pit_common.h"

namespace {

constexpr unsigned GEO_INF = 0x7f800000u;
static_assert(PIT_GEO_MAX_REACH <= 65535, "s_hash holds e + 1 in 16 bits");
static_assert(PIT_GEO_MAX_K <= PIT_GEO_MAX_REACH, "a list is cut from the settled set");

__device__ __forceinline__ unsigned geo_bits(float d) {
    const unsigned b = __float_as_uint(d);
    return b == 0x80000000u ? 0u : b;
}

__device__ __forceinline__ unsigned geo_hash(int v, int hbits) { return ((unsigned)v * 2654435761u) >> (32 - hbits); }

// the entry of vertex v, or -1 with `slot` = the empty slot its probe sequence ends at
__device__ __forceinline__ int geo_find(const int* s_vert, const unsigned short* s_hash, int hbits, int v, unsigned& slot) {
    const unsigned mask = (1u << hbits) - 1u;
    unsigned s = geo_hash(v, hbits);
    for (unsigned p = 0; p <= mask; ++p) {               // (the table is at most half full: an empty slot ends every probe)
        const int e = (int)s_hash[s] - 1;
        if (e < 0) break;
        const int u = s_vert[e];
        if (u == v || u == ~v) return e;
        s = (s + 1u) & mask;
    }
    slot = s;
    return -1;
}

__global__ __launch_bounds__(PIT_WAVE) void geo_knn_kernel(const int* __restrict__ adj, const float* __restrict__ w, long adj_bstride,
                                                           int n_vert, int n_edge, const int* __restrict__ sources, long src_bstride,
                                                           int n_rows, const int* __restrict__ key_of, long key_bstride,
                                                           const int* __restrict__ len_v, int k, int reach, int cap, int hbits,
                                                           int* __restrict__ idx, float* __restrict__ dist, float* __restrict__ next,
                                                           int* __restrict__ status) {
    extern __shared__ unsigned geo_lds[];
    int* s_vert = (int*)geo_lds;                          // cap = the power of two >= reach entries each
    unsigned* s_len = geo_lds + cap;
    unsigned short* s_hash = (unsigned short*)(geo_lds + 2 * cap);
    const int lane = (int)threadIdx.x;
    const long row = blockIdx.x;                          // sample * n_rows + i
    const long sample = row / n_rows, i = row - sample * n_rows;
    const int vs = len_v ? max(1, min(len_v[sample], n_vert)) : n_vert;
    const int src = sources ? sources[sample * src_bstride + i] : (int)i;
    int* idx_row = idx + row * k;
    float* dist_row = dist + row * k;
    if (src < 0 || src >= vs) {                           // a padded row
        for (int t = lane; t < k; t += PIT_WAVE) { idx_row[t] = -1; dist_row[t] = 0.0f; }
        if (lane == 0) { next[row] = __builtin_inff(); status[row] = 0; }
        return;
    }
    const int* adj_s = adj + sample * adj_bstride;
    const float* w_s = w + sample * adj_bstride;
    const int* key_s = key_of ? key_of + sample * key_bstride : nullptr;

    for (int t = lane; t < (1 << hbits); t += PIT_WAVE) s_hash[t] = 0;
    __syncthreads();
    if (lane == 0) { s_vert[0] = src; s_len[0] = 0u; s_hash[geo_hash(src, hbits)] = 1; }
    int count = 1, n_cand = 0;
    unsigned kth = 0u, front = GEO_INF;                   // the k-th candidate's length; the frontier's least length at the end
    bool truncated = false;

    for (int step = 0; step <= reach; ++step) {           // (count <= reach vertices are settled, then the frontier is empty)
        __syncthreads();
        // ---- the least (length, vertex) of the frontier
        unsigned long long best = ~0ull;
        int best_e = -1;
        for (int e = lane; e < count; e += PIT_WAVE) {
            const int u = s_vert[e];
            const unsigned long long word = ((unsigned long long)s_len[e] << 32) | (unsigned)u;
            if (u >= 0 && word < best) { best = word; best_e = e; }
        }
        unsigned long long m = best;
#pragma unroll
        for (int o = PIT_WAVE / 2; o > 0; o >>= 1) {
            const unsigned long long other = __shfl_xor(m, o);
            m = other < m ? other : m;
        }
        if (m == ~0ull) break;                            // the frontier is empty
        const unsigned lbits = (unsigned)(m >> 32);
        if (n_cand >= k && lbits > kth) { front = lbits; break; }
        const unsigned long long holds = __ballot(best == m);     // (the words of a row are distinct: one lane)
        const int e_min = __shfl(best_e, __ffsll((long long)holds) - 1);
        const int v = (int)(unsigned)m;
        // ---- settle it
        if (lane == 0) s_vert[e_min] = ~v;
        const int kv = key_s ? key_s[v] : v;
        if (kv >= 0) {
            ++n_cand;
            if (n_cand == k) kth = lbits;
        }
        // ---- relax its edges
        const float d_v = __uint_as_float(lbits);
        const long edge0 = (long)v * n_edge;
        for (int t0 = 0; t0 < n_edge && !truncated; t0 += PIT_WAVE) {
            __syncthreads();
            const int t = t0 + lane;
            int a = -1;
            unsigned nl = 0u;
            bool on = t < n_edge;
            if (on) {
                a = adj_s[edge0 + t];
                on = a >= 0 && a < vs;
                if (on) nl = geo_bits(__fadd_rn(d_v, w_s[edge0 + t]));
            }
            bool fresh = false;
            if (on) {
                unsigned slot;
                const int f = geo_find(s_vert, s_hash, hbits, a, slot);
                if (f < 0) fresh = true;
                else if (s_vert[f] >= 0) atomicMin(&s_len[f], nl);
            }
            __syncthreads();
            unsigned long long pend = __ballot(fresh);
            while (pend) {                                // at most reach appends over the whole row
                const int l = __ffsll((long long)pend) - 1;
                pend &= pend - 1ull;
                const int av = __shfl(a, l);
                const unsigned nv = (unsigned)__shfl((int)nl, l);
                int res = 0;
                if (lane == 0) {
                    unsigned slot;
                    const int f = geo_find(s_vert, s_hash, hbits, av, slot);
                    if (f >= 0) {
                        if (s_vert[f] >= 0 && nv < s_len[f]) s_len[f] = nv;
                    } else if (count < reach) {
                        s_vert[count] = av;
                        s_len[count] = nv;
                        s_hash[slot] = (unsigned short)(count + 1);
                        res = 1;
                    } else {
                        res = 2;
                    }
                }
                res = __shfl(res, 0);
                if (res == 1) ++count;
                if (res == 2) { truncated = true; break; }
            }
        }
        if (truncated) break;
    }
    __syncthreads();

    // ---- the settled key vertices to the front (an entry moves to a position at or before its own)
    int n_list = 0;
    for (int e0 = 0; e0 < count; e0 += PIT_WAVE) {
        const int e = e0 + lane;
        bool c = false;
        int v = 0;
        unsigned l = 0u;
        if (e < count) {
            const int u = s_vert[e];
            if (u < 0) {
                v = ~u;
                c = (key_s ? key_s[v] : v) >= 0;
                l = s_len[e];
            }
        }
        const unsigned long long mask = __ballot(c);
        const int pos = n_list + __popcll(mask & ((1ull << lane) - 1ull));
        __syncthreads();
        if (c) { s_vert[pos] = v; s_len[pos] = l; }
        n_list += __popcll(mask);
        __syncthreads();
    }
    // ---- ascending by (length, vertex)
    if (n_list > 1) {
        const int padded = 1 << (32 - __clz(n_list - 1));            // <= cap
        for (int t = n_list + lane; t < padded; t += PIT_WAVE) { s_vert[t] = -1; s_len[t] = 0xffffffffu; }
        for (int size = 2; size <= padded; size <<= 1)
            for (int stride = size >> 1; stride > 0; stride >>= 1) {
                __syncthreads();
                for (int t = lane; t < padded / 2; t += PIT_WAVE) {
                    const int lo = 2 * t - (t & (stride - 1)), hi = lo + stride;
                    const int va = s_vert[lo], vb = s_vert[hi];
                    const unsigned la = s_len[lo], lb = s_len[hi];
                    const unsigned long long wa = ((unsigned long long)la << 32) | (unsigned)va;
                    const unsigned long long wb = ((unsigned long long)lb << 32) | (unsigned)vb;
                    if ((wa > wb) == ((lo & size) == 0)) { s_vert[lo] = vb; s_len[lo] = lb; s_vert[hi] = va; s_len[hi] = la; }
                }
            }
        __syncthreads();
    }
    for (int t = lane; t < k; t += PIT_WAVE) {
        if (t < n_list) {
            const int v = min(max(s_vert[t], 0), vs - 1);             // (a vertex of the row: inside [0, vs) already)
            idx_row[t] = key_s ? key_s[v] : v;
            dist_row[t] = __uint_as_float(s_len[t]);
        } else {
            idx_row[t] = -1;
            dist_row[t] = 0.0f;
        }
    }
    if (lane == 0) {
        unsigned nb = front;
        if (n_list > k) nb = min(nb, s_len[k]);
        next[row] = truncated ? __builtin_inff() : __uint_as_float(nb);
        status[row] = truncated ? 1 : 0;
    }
}

}  // namespace

extern "C" int pit_geo_knn(const int* adj, const float* w, long adj_bstride, int batch, int n_vert, int n_edge, const int* sources,
                           long src_bstride, int n_rows, const int* key_of, long key_bstride, const int* len_v, int k, int reach,
                           int* idx, float* dist, float* next, int* status, void* stream) {
    if (!adj || !w || !idx || !dist || !next || !status) return PIT_ERR_NULL;
    if (batch < 1 || n_vert < 1 || n_edge < 1 || n_rows < 1 || k < 1 || reach < k) return PIT_ERR_SIZE;
    if ((long)n_vert * n_edge > 0x7fffffffL) return PIT_ERR_SIZE;
    if (adj_bstride != 0 && adj_bstride < (long)n_vert * n_edge) return PIT_ERR_SIZE;
    if (sources ? (src_bstride != 0 && src_bstride < n_rows) : (n_rows != n_vert || src_bstride != 0)) return PIT_ERR_SIZE;
    if (key_of ? (key_bstride != 0 && key_bstride < n_vert) : key_bstride != 0) return PIT_ERR_SIZE;
    if ((long)batch * n_rows * k > 0x7fffffffL) return PIT_ERR_SIZE;
    if (k > PIT_GEO_MAX_K || reach > PIT_GEO_MAX_REACH) return PIT_ERR_UNSUPPORTED;
    int cap = 64, hbits = 7;                              // entries: the power of two >= reach; slots: 2 * cap
    while (cap < reach) { cap <<= 1; ++hbits; }
    const size_t lds = (size_t)cap * 8 + ((size_t)2 << hbits);
    const unsigned rows = (unsigned)((long)batch * n_rows);
    hipLaunchKernelGGL(geo_knn_kernel, dim3(rows), dim3(PIT_WAVE), lds, (hipStream_t)stream, adj, w, adj_bstride, n_vert, n_edge,
                       sources, src_bstride, n_rows, key_of, key_bstride, len_v, k, reach, cap, hbits, idx, dist, next, status);
    PIT_CHECK_LAUNCH();
    return 0;
}
