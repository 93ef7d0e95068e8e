// The k nearest keys of every row, ascending (include/pit_hip.h, pit_knn_box / pit_knn_rows): the neighbour lists of the metric
// layers without torch.topk and - for a box metric - without the N x J matrix.
//
// One workgroup of 256 threads per row; two loaders over ONE selection core.  A key's distance is mapped to its bit pattern
// (distances >= 0 order as unsigned integers; -0.0 is stored as +0.0) and joined with its index into the 64-bit word
// (distance bits << 32 | j): the words of a row are distinct and their unsigned order is the order of the header - the distance, then
// the key index - whatever the distances hold, so every emitted index lies in [0, J) and no index comes twice.
//   1. the k-th smallest word by an MSB-first radix search, 8 bits a pass over a 256-bin histogram in LDS (integer LDS counters: no
//      rounding, no global atomics): four passes give the k-th distance T.  When the row's whole tie shell at T fits into the list -
//      every row but those cut inside a shell - the cut is (T, any index) and the search ends; otherwise it goes on over the bits of
//      the index among the keys at T, which gives the lowest indices of the shell.
//   2. one collecting pass: a key with word <= cut takes a slot of the LDS list (any slot: the words are sorted next), the others
//      fold their distance into a minimum - the distance of pair k + 1, `next`.
//   3. a bitonic sort of the k words in LDS, and the stores.
// The two forms differ in where a pass finds the distances: a row of up to PIT_KNN_REG_MAX_KEYS keys computes (or loads) them once
// into 4 registers per thread (form 1); a longer row recomputes them in every pass, four independent keys per thread in flight
// (form 2), because no memory holds a row (the matrix never exists).  Counters of one wave that hit the same bin - the first pass
// sees the exponent bits, which are nearly equal for a whole row - are added once per wave for the two most frequent leaders.
//
// pit_knn_box_ragged (RAG = true instances of the box kernel): sample s searches its first L = len_in[s] keys - the selection core
// takes the key count and k at run time, so the row runs it with (L, min(k, L)) and then fills the slots it did not reach with
// key -1 / distance 0; a row >= len_out[s] is filled whole and reads nothing.  The form is the host's choice from the padded n_in.
#include "pit_common.h"

namespace {

constexpr int KNN_THREADS = 256;
constexpr int KNN_WAVES = KNN_THREADS / PIT_WAVE;
constexpr int KNN_PPT = PIT_KNN_REG_MAX_KEYS / KNN_THREADS;        // keys per thread, in registers (form 1) or in flight (form 2)
static_assert(KNN_PPT * KNN_THREADS == PIT_KNN_REG_MAX_KEYS, "the register form holds a whole number of keys per thread");
static_assert(PIT_KNN_MAX_K == 2048, "the LDS list below holds 2048 words");

struct knn_periods { float p[PIT_MAX_SPACE_DIM]; };                 // <= 0: the axis does not wrap

__device__ __forceinline__ unsigned knn_bits(float d) {
    const unsigned b = __float_as_uint(d);
    return b == 0x80000000u ? 0u : b;
}

// distances from coordinates: |x - y|, the wrap, the squares summed in ascending order of the coordinate, every operation rounded
template <int SDIM, bool WRAP>
struct box_loader {
    const float* keys;                  // this sample's (J, SDIM) mesh
    float x[SDIM];
    knn_periods per;
    __device__ __forceinline__ unsigned operator()(unsigned j) const {
        const float* y = keys + (long)j * SDIM;
        float d = 0.0f;
#pragma unroll
        for (int a = 0; a < SDIM; ++a) {
            float t = fabsf(__fsub_rn(x[a], y[a]));
            if (WRAP) t = per.p[a] > 0.0f ? fminf(t, __fsub_rn(per.p[a], t)) : t;
            const float q = __fmul_rn(t, t);
            d = a == 0 ? q : __fadd_rn(d, q);
        }
        return knn_bits(d);
    }
};

// distances the caller formed: one row of a matrix
struct rows_loader {
    const float* row;
    __device__ __forceinline__ unsigned operator()(unsigned j) const { return knn_bits(row[j]); }
};

// one histogram update of a wave: lanes with `on` count `digit`; the bins of the first two leaders are added once per wave
__device__ __forceinline__ void knn_count(unsigned* hist, bool on, unsigned digit) {
    unsigned long long act = __ballot(on);
    const int lane = threadIdx.x & (PIT_WAVE - 1);
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        if (!act) break;
        const int leader = __ffsll((long long)act) - 1;
        const unsigned dl = (unsigned)__shfl((int)digit, leader);
        const unsigned long long same = __ballot(on && digit == dl) & act;
        if (lane == leader) atomicAdd(&hist[dl], (unsigned)__popcll(same));
        act &= ~same;
    }
    if ((act >> lane) & 1ull) atomicAdd(&hist[digit], 1u);
}

template <class Loader, bool CACHED>
__device__ __forceinline__ void knn_row(const Loader& ld, unsigned J, int k, int* __restrict__ idx_out,
                                        float* __restrict__ dist_out, float* __restrict__ next_out) {
    __shared__ unsigned long long s_list[PIT_KNN_MAX_K];
    __shared__ unsigned s_hist[256];
    __shared__ unsigned s_wtot[KNN_WAVES];
    __shared__ unsigned s_sel[3];
    __shared__ unsigned s_cnt;
    __shared__ unsigned s_min[KNN_WAVES];
    const unsigned tid = threadIdx.x, lane = tid & (PIT_WAVE - 1), wave = tid / PIT_WAVE;

    unsigned cache[KNN_PPT];
    if constexpr (CACHED) {
#pragma unroll
        for (int s = 0; s < KNN_PPT; ++s) cache[s] = ld(min(s * KNN_THREADS + tid, J - 1u));
    }
    // f(distance bits, j, j < J) for every key of the row, by every thread of the workgroup in step (f may vote)
    auto for_keys = [&](auto&& f) {
        if constexpr (CACHED) {
#pragma unroll
            for (int s = 0; s < KNN_PPT; ++s) {
                const unsigned j = s * KNN_THREADS + tid;
                f(cache[s], j, j < J);
            }
        } else {
            for (unsigned base = 0; base < J; base += KNN_THREADS * KNN_PPT) {
                unsigned b[KNN_PPT];
#pragma unroll
                for (int s = 0; s < KNN_PPT; ++s) b[s] = ld(min(base + s * KNN_THREADS + tid, J - 1u));
#pragma unroll
                for (int s = 0; s < KNN_PPT; ++s) {
                    const unsigned j = base + s * KNN_THREADS + tid;
                    f(b[s], j, j < J);
                }
            }
        }
    };

    // ---- 1. the k-th smallest word
    int index_bits = 0;
    while (index_bits < 32 && ((J - 1u) >> index_bits)) ++index_bits;
    const int index_passes = (index_bits + 7) / 8;
    unsigned long long prefix = 0ull, cut = 0ull;
    unsigned rank = (unsigned)k - 1u;                    // 0-based, among the words that share `prefix`
    for (int pass = 0; pass < 8; ++pass) {
        const int shift = 56 - 8 * pass;
        if (pass >= 4 && pass < 8 - index_passes) continue;          // index bits that are zero for every key
        s_hist[tid] = 0u;
        __syncthreads();
        for_keys([&](unsigned bits, unsigned j, bool valid) {
            const unsigned long long w = ((unsigned long long)bits << 32) | j;
            const bool on = valid && (pass == 0 || (w >> (shift + 8)) == (prefix >> (shift + 8)));
            knn_count(s_hist, on, (unsigned)(w >> shift) & 255u);
        });
        __syncthreads();
        // the bin that holds `rank`: an exclusive scan of the 256 counts, one per thread
        const unsigned h = s_hist[tid];
        unsigned incl = h;
#pragma unroll
        for (int o = 1; o < PIT_WAVE; o <<= 1) {
            const unsigned up = (unsigned)__shfl_up((int)incl, o);
            incl += lane >= (unsigned)o ? up : 0u;
        }
        if (lane == PIT_WAVE - 1) s_wtot[wave] = incl;
        __syncthreads();
        unsigned excl = incl - h;
        for (unsigned w = 0; w < wave; ++w) excl += s_wtot[w];
        if (h > 0u && excl <= rank && rank - excl < h) { s_sel[0] = tid; s_sel[1] = excl; s_sel[2] = h; }
        __syncthreads();
        prefix |= (unsigned long long)s_sel[0] << shift;
        rank -= s_sel[1];
        cut = prefix;
        if (pass == 3 && rank + 1u == s_sel[2]) {        // the whole shell at T is taken: no search among its indices
            cut = prefix | 0xffffffffull;
            break;
        }
    }

    // ---- 2. the words up to the cut, and the least distance beyond it
    const int padded = k <= 1 ? 1 : 1 << (32 - __clz(k - 1));           // the power of two the sort runs on
    for (int t = k + (int)tid; t < padded; t += KNN_THREADS) s_list[t] = ~0ull;
    if (tid == 0) s_cnt = 0u;
    __syncthreads();
    unsigned beyond = 0xffffffffu;
    for_keys([&](unsigned bits, unsigned j, bool valid) {
        const unsigned long long w = ((unsigned long long)bits << 32) | j;
        if (valid && w <= cut) {
            const unsigned slot = atomicAdd(&s_cnt, 1u);
            if (slot < (unsigned)k) s_list[slot] = w;
        } else if (valid) {
            beyond = min(beyond, bits);
        }
    });
#pragma unroll
    for (int o = PIT_WAVE / 2; o > 0; o >>= 1) beyond = min(beyond, (unsigned)__shfl_xor((int)beyond, o));
    if (lane == 0) s_min[wave] = beyond;

    // ---- 3. ascending
    for (int size = 2; size <= padded; size <<= 1)
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            __syncthreads();
            for (int t = (int)tid; t < padded / 2; t += KNN_THREADS) {
                const int lo = 2 * t - (t & (stride - 1)), hi = lo + stride;
                const unsigned long long a = s_list[lo], b = s_list[hi];
                if ((a > b) == ((lo & size) == 0)) { s_list[lo] = b; s_list[hi] = a; }
            }
        }
    __syncthreads();
    for (int t = (int)tid; t < k; t += KNN_THREADS) {
        const unsigned long long w = s_list[t];
        idx_out[t] = (int)min((unsigned)w, J - 1u);                  // (a word of the row: below J already)
        dist_out[t] = __uint_as_float((unsigned)(w >> 32));
    }
    if (tid == 0) {
        unsigned m = s_min[0];
#pragma unroll
        for (int w = 1; w < KNN_WAVES; ++w) m = min(m, s_min[w]);
        *next_out = (unsigned)k == J ? __builtin_inff() : __uint_as_float(m);
    }
}

template <int SDIM, bool WRAP, bool CACHED, bool RAG>
__global__ __launch_bounds__(KNN_THREADS) void knn_box_kernel(const float* __restrict__ mesh_out, const float* __restrict__ mesh_in,
                                                              int n_out, int n_in, long out_stride, long in_stride,
                                                              knn_periods per, int k, int* __restrict__ idx,
                                                              float* __restrict__ dist, float* __restrict__ next,
                                                              const int* __restrict__ len_out, const int* __restrict__ len_in) {
    const long row = blockIdx.x;                         // sample * n_out + i
    const long sample = row / n_out, i = row - sample * n_out;
    int k_row = k;                                       // the pairs this row emits (ragged: min(k, the sample's keys))
    if constexpr (RAG) {                                 // lengths clamped into [1, width]; NULL: the full width
        const int lo = len_out ? max(1, min(len_out[sample], n_out)) : n_out;
        const int li = len_in ? max(1, min(len_in[sample], n_in)) : n_in;
        const int kk = min(k, li);
        // the slots the search does not reach: all of a padded row's, those beyond the sample's keys otherwise (block-uniform)
        for (int t = (i >= lo ? 0 : kk) + (int)threadIdx.x; t < k; t += KNN_THREADS) {
            idx[row * k + t] = -1;
            dist[row * k + t] = 0.0f;
        }
        if (i >= lo) {
            if (threadIdx.x == 0) next[row] = __builtin_inff();
            return;
        }
        n_in = li;                                       // (the selection writes +inf to `next` when it took every key)
        k_row = kk;
    }
    box_loader<SDIM, WRAP> ld;
    ld.keys = mesh_in + sample * in_stride * SDIM;
    const float* x = mesh_out + (sample * out_stride + i) * SDIM;
#pragma unroll
    for (int a = 0; a < SDIM; ++a) ld.x[a] = x[a];
    ld.per = per;
    knn_row<box_loader<SDIM, WRAP>, CACHED>(ld, (unsigned)n_in, k_row, idx + row * k, dist + row * k, next + row);
}

template <bool CACHED>
__global__ __launch_bounds__(KNN_THREADS) void knn_rows_kernel(const float* __restrict__ m, long ld_m, long m_bstride, int n_out,
                                                               int n_in, int k, int* __restrict__ idx, float* __restrict__ dist,
                                                               float* __restrict__ next) {
    const long row = blockIdx.x;
    const long sample = row / n_out, i = row - sample * n_out;
    rows_loader ld;
    ld.row = m + sample * m_bstride + i * ld_m;
    knn_row<rows_loader, CACHED>(ld, (unsigned)n_in, k, idx + row * k, dist + row * k, next + row);
}

template <int SDIM, bool RAG>
void knn_box_launch(bool wrap, bool cached, unsigned rows, hipStream_t st, const float* mesh_out, const float* mesh_in, int n_out,
                    int n_in, long out_stride, long in_stride, const knn_periods& per, int k, int* idx, float* dist, float* next,
                    const int* len_out, const int* len_in) {
#define PIT_KNN_BOX(W_, C_) hipLaunchKernelGGL((knn_box_kernel<SDIM, W_, C_, RAG>), dim3(rows), dim3(KNN_THREADS), 0, st, mesh_out, \
                                               mesh_in, n_out, n_in, out_stride, in_stride, per, k, idx, dist, next, len_out, len_in)
    if (wrap) { if (cached) PIT_KNN_BOX(true, true); else PIT_KNN_BOX(true, false); }
    else      { if (cached) PIT_KNN_BOX(false, true); else PIT_KNN_BOX(false, false); }
#undef PIT_KNN_BOX
}

int g_last_form = 0;                                     // include/pit_hip.h, pit_knn_last_form

// the refusals the two entries share, in the header's order; `sizes_ok`: what only the caller can check
int knn_refuse(bool pointers_ok, bool sizes_ok, int batch, int n_out, int n_in, int k) {
    if (!pointers_ok) return PIT_ERR_NULL;
    if (batch < 1 || n_out < 1 || n_in < 1 || !sizes_ok || k < 1 || k > n_in) return PIT_ERR_SIZE;
    if ((long)batch * n_out * k > 0x7fffffffL) return PIT_ERR_SIZE;
    if (k > PIT_KNN_MAX_K) return PIT_ERR_UNSUPPORTED;
    return 0;
}

template <bool RAG>
int knn_box_entry(const float* mesh_out, const float* mesh_in, int batch, int n_out, int n_in, int space_dim, long out_stride,
                  long in_stride, const float* periods, int k, const int* len_out, const int* len_in, int* idx, float* dist,
                  float* next, void* stream) {
    const bool sizes_ok = space_dim >= 1 && space_dim <= PIT_MAX_SPACE_DIM && (out_stride == 0 || out_stride >= n_out) &&
                          (in_stride == 0 || in_stride >= n_in);
    const int rc = knn_refuse(mesh_out && mesh_in && idx && dist && next, sizes_ok, batch, n_out, n_in, k);
    if (rc) return rc;
    knn_periods per;
    bool wrap = false;
    for (int a = 0; a < PIT_MAX_SPACE_DIM; ++a) {
        per.p[a] = (periods && a < space_dim && periods[a] > 0.0f) ? periods[a] : 0.0f;
        wrap = wrap || per.p[a] > 0.0f;
    }
    const bool cached = n_in <= PIT_KNN_REG_MAX_KEYS;
    const unsigned rows = (unsigned)((long)batch * n_out);
    hipStream_t st = (hipStream_t)stream;
#define PIT_KNN_SDIM(S_) case S_: knn_box_launch<S_, RAG>(wrap, cached, rows, st, mesh_out, mesh_in, n_out, n_in, out_stride, in_stride, \
                                                          per, k, idx, dist, next, len_out, len_in); break
    switch (space_dim) {
        PIT_KNN_SDIM(1); PIT_KNN_SDIM(2); PIT_KNN_SDIM(3); PIT_KNN_SDIM(4);
        PIT_KNN_SDIM(5); PIT_KNN_SDIM(6); PIT_KNN_SDIM(7); PIT_KNN_SDIM(8);
    }
#undef PIT_KNN_SDIM
    PIT_CHECK_LAUNCH();
    g_last_form = cached ? 1 : 2;
    return 0;
}

}  // namespace

extern "C" int pit_knn_box(const float* mesh_out, const float* mesh_in, int batch, int n_out, int n_in, int space_dim,
                           long out_stride, long in_stride, const float* periods, int k, int* idx, float* dist, float* next,
                           void* stream) {
    return knn_box_entry<false>(mesh_out, mesh_in, batch, n_out, n_in, space_dim, out_stride, in_stride, periods, k, nullptr, nullptr,
                                idx, dist, next, stream);
}

extern "C" int pit_knn_box_ragged(const float* mesh_out, const float* mesh_in, int batch, int n_out, int n_in, int space_dim,
                                  long out_stride, long in_stride, const float* periods, int k, const int* len_out,
                                  const int* len_in, int* idx, float* dist, float* next, void* stream) {
    return knn_box_entry<true>(mesh_out, mesh_in, batch, n_out, n_in, space_dim, out_stride, in_stride, periods, k, len_out, len_in,
                               idx, dist, next, stream);
}

extern "C" int pit_knn_rows(const float* m, long ld_m, long m_bstride, int batch, int n_out, int n_in, int k, int* idx,
                            float* dist, float* next, void* stream) {
    const bool sizes_ok = ld_m >= n_in && (m_bstride == 0 || (n_out >= 1 && m_bstride >= (long)(n_out - 1) * ld_m + n_in));
    const int rc = knn_refuse(m && idx && dist && next, sizes_ok, batch, n_out, n_in, k);
    if (rc) return rc;
    const bool cached = n_in <= PIT_KNN_REG_MAX_KEYS;
    const unsigned rows = (unsigned)((long)batch * n_out);
    if (cached)
        hipLaunchKernelGGL(knn_rows_kernel<true>, dim3(rows), dim3(KNN_THREADS), 0, (hipStream_t)stream, m, ld_m, m_bstride, n_out,
                           n_in, k, idx, dist, next);
    else
        hipLaunchKernelGGL(knn_rows_kernel<false>, dim3(rows), dim3(KNN_THREADS), 0, (hipStream_t)stream, m, ld_m, m_bstride, n_out,
                           n_in, k, idx, dist, next);
    PIT_CHECK_LAUNCH();
    g_last_form = cached ? 1 : 2;
    return 0;
}

extern "C" int pit_knn_last_form(void) { return g_last_form; }
