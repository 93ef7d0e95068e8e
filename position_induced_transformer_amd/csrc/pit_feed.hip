// Device-resident data feed (include/pit_hip.h, pit_batch_feed): one launch at the head of a captured step picks the step's
// samples - a keyed permutation of the epoch, the identity or a caller's order; this rank's shard of it - and gathers their rows
// from the dataset in device memory into the step's static buffers: the shuffle, the collate and the copies of
// train_darcy.py:98,124-126 without the host.  The cursor lives on the device; the workgroup of the last arrival ticket moves it
// (adam_step_kernel's rule: every workgroup reads the cursor first), so a replayed graph walks through the epochs by itself.
//
// A pure copy.  grid = (pieces, batch): every field's row is cut into equal pieces, one workgroup per (slot, field, piece) -
// 256 threads and pieces of at least 2048 words while the launch moves no more than FEED_SMALL_WORDS (launch latency is the
// cost: one round trip of eight dwords per thread), 1024 threads and pieces of at least 8192 words beyond; either way no more
// pieces per slot than keep the grid near FEED_FILL workgroups, one per CU: every workgroup ends with a returning atomic on
// ONE address (the ticket), and a thousand of those cost more than the copy (measured: DESIGN section 19).  A piece whose
// source and destination are congruent mod 16 moves as 16-byte units with a dword head and tail, any other piece as dwords.
// All accesses go through raw buffer resources that span exactly the bytes of their run: a lane beyond the end reads 0 and
// its store is dropped by the range check, so a tile is a block of loads followed by a block of stores with no predicate
// anywhere (a predicated global load costs a round trip of its own).
#include "pit_common.h"

namespace {

constexpr int FEED_T_SMALL = 256, FEED_T_LARGE = 1024;  // threads per workgroup
constexpr long FEED_MIN_WORDS = 8;      // a piece keeps at least this many words PER THREAD
constexpr long FEED_FILL = 256;         // workgroups that occupy the chip (one per CU); no further split beyond
constexpr long FEED_SMALL_WORDS = FEED_FILL * FEED_T_SMALL * FEED_MIN_WORDS;      // 2 MiB: the small form up to here

struct FeedFields {                     // the descriptors, by value in the kernel arguments
    const char* src[PIT_FEED_MAX_FIELDS];
    char* dst[PIT_FEED_MAX_FIELDS];
    long words[PIT_FEED_MAX_FIELDS];    // row_bytes / 4
    long piece[PIT_FEED_MAX_FIELDS];    // words per workgroup
    int first_part[PIT_FEED_MAX_FIELDS];        // blockIdx.x of the field's first piece
    int n;
};

__device__ __forceinline__ uint32_t fmix(uint32_t h) {
    h ^= h >> 16; h *= 0x85EBCA6Bu; h ^= h >> 13; h *= 0xC2B2AE35u; h ^= h >> 16;
    return h;
}

// the keyed permutation of [0, n) (four Feistel rounds on an even number of bits, cycle walking: the domain is < 4n)
__device__ __forceinline__ uint32_t feistel(uint32_t n, long long seed, uint32_t epoch, uint32_t g) {
    int bits = 32 - __builtin_clz((n - 1u) | 1u);
    if (n <= 1u) bits = 0;
    bits = max(2, bits);
    bits += bits & 1;
    const int half = bits / 2;
    const uint32_t mask = (1u << half) - 1u;
    const uint32_t lo = (uint32_t)((unsigned long long)seed & 0xffffffffull), hi = (uint32_t)((unsigned long long)seed >> 32);
    uint32_t key[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) key[j] = fmix(lo ^ fmix(hi + 0x9E3779B9u * (epoch + 1u) + (uint32_t)j));
    uint32_t x = g;
    do {
        uint32_t L = x >> half, R = x & mask;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const uint32_t t = L ^ (fmix(R + key[j]) & mask);
            L = R;
            R = t;
        }
        x = (L << half) | R;
    } while (x >= n);
    return x;
}

constexpr int FEED_DEEP_W = 8;          // dword loads in flight per thread
constexpr int FEED_DEEP_V = 4;          // 16-byte loads in flight per thread (64 KiB per 1024-thread workgroup)

// n <= PIT_FEED_MAX_ROW_BYTES / 4 words from s to d (both 4-byte aligned), by the whole workgroup
template <int FEED_T>
__device__ __forceinline__ void copy_run(const char* s, char* d, unsigned n, int tid) {
    if ((((uintptr_t)s ^ (uintptr_t)d) & 15u) == 0 && n >= 8u) {
        const unsigned head = min(n, (unsigned)(((16u - ((uintptr_t)s & 15u)) & 15u) >> 2));     // dwords before the 16-byte units
        const unsigned body = (n - head) >> 2, tail = n - head - 4u * body;
        const __amdgpu_buffer_rsrc_t sh = make_rsrc(s, head * 4u), dh = make_rsrc(d, head * 4u);
        const __amdgpu_buffer_rsrc_t sb = make_rsrc(s + head * 4u, body * 16u), db = make_rsrc(d + head * 4u, body * 16u);
        const unsigned done = (head + 4u * body) * 4u;
        const __amdgpu_buffer_rsrc_t st = make_rsrc(s + done, tail * 4u), dt = make_rsrc(d + done, tail * 4u);
        const int hv = __builtin_amdgcn_raw_buffer_load_b32(sh, tid * 4, 0, 0);
        const int tv = __builtin_amdgcn_raw_buffer_load_b32(st, tid * 4, 0, 0);
        bool first = true;
        for (unsigned i0 = 0; i0 < body; i0 += FEED_DEEP_V * FEED_T) {
            i32x4 v[FEED_DEEP_V];
#pragma unroll
            for (int u = 0; u < FEED_DEEP_V; ++u) v[u] = __builtin_amdgcn_raw_buffer_load_b128(sb, (int)((i0 + u * FEED_T + tid) * 16u), 0, 0);
            if (first) {                                               // (head and tail travel with the first tile)
                __builtin_amdgcn_raw_buffer_store_b32(hv, dh, tid * 4, 0, 0);
                __builtin_amdgcn_raw_buffer_store_b32(tv, dt, tid * 4, 0, 0);
                first = false;
            }
#pragma unroll
            for (int u = 0; u < FEED_DEEP_V; ++u) __builtin_amdgcn_raw_buffer_store_b128(v[u], db, (int)((i0 + u * FEED_T + tid) * 16u), 0, 0);
        }
    } else {
        const __amdgpu_buffer_rsrc_t sr = make_rsrc(s, n * 4u), dr = make_rsrc(d, n * 4u);
        for (unsigned i0 = 0; i0 < n; i0 += FEED_DEEP_W * FEED_T) {
            int v[FEED_DEEP_W];
#pragma unroll
            for (int u = 0; u < FEED_DEEP_W; ++u) v[u] = __builtin_amdgcn_raw_buffer_load_b32(sr, (int)((i0 + u * FEED_T + tid) * 4u), 0, 0);
#pragma unroll
            for (int u = 0; u < FEED_DEEP_W; ++u) __builtin_amdgcn_raw_buffer_store_b32(v[u], dr, (int)((i0 + u * FEED_T + tid) * 4u), 0, 0);
        }
    }
}

template <int FEED_T>
__global__ __launch_bounds__(FEED_T) void batch_feed_kernel(FeedFields fields, uint32_t n_samples,
                                                            int batch, long long rank, long long world, long long steps,
                                                            int shuffle, const int* __restrict__ order, long long seed,
                                                            long long* state, int* __restrict__ indices,
                                                            int* __restrict__ n_valid) {
    const int tid = threadIdx.x;
    const int s = blockIdx.y, part = blockIdx.x;
    // the cursor: read by EVERY workgroup before its ticket, rewritten by the last arriver alone
    const long long cursor = __hip_atomic_load(state, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const unsigned long long c = cursor > 0 ? (unsigned long long)cursor : 0ull;
    const unsigned long long epoch = c / (unsigned long long)steps, i = c % (unsigned long long)steps;
    const long long first = ((long long)i * world + rank) * batch;     // global position of slot 0
    const uint32_t pos = (uint32_t)((unsigned long long)(first + s) % n_samples);
    uint32_t idx;
    if (order) {
        const int v = order[pos];
        idx = (uint32_t)min(max(v, 0), (int)(n_samples - 1u));
    } else if (!shuffle) {
        idx = pos;
    } else {
        idx = feistel(n_samples, seed, (uint32_t)(epoch & 0xffffffffull), pos);
    }
    if (part == 0 && tid == 0) {
        if (indices) indices[s] = (int)idx;
        if (n_valid && s == 0) {
            const long long left = (long long)n_samples - first;
            *n_valid = (int)min(max(left, 0ll), (long long)batch);
        }
    }
    idx = (uint32_t)__builtin_amdgcn_readfirstlane((int)idx);                         // (the same in every lane: the buffer resources stay scalar)
    // this workgroup's piece: words [a, b) of field f's row
    int f = 0;
    while (f + 1 < fields.n && part >= fields.first_part[f + 1]) ++f;
    const long words = fields.words[f];
    const long a = min(words, (long)(part - fields.first_part[f]) * fields.piece[f]), b = min(words, a + fields.piece[f]);
    const char* src = fields.src[f] + ((long)idx * words + a) * 4;
    char* dst = fields.dst[f] + ((long)s * words + a) * 4;
    copy_run<FEED_T>(src, dst, (unsigned)(b - a), tid);               // (a row is at most PIT_FEED_MAX_ROW_BYTES: 32-bit byte offsets)
    __syncthreads();
    if (tid == 0) {
        // No fence: the cursor's value has been consumed (every address above derives from it), so its load was performed
        // before this ticket; the copied rows become visible at the end of the launch like any kernel's stores.
        unsigned long long* ticket = reinterpret_cast<unsigned long long*>(state + 1);
        if (atomicAdd(ticket, 1ull) == (unsigned long long)gridDim.x * gridDim.y - 1ull) {
            __hip_atomic_store(state, (long long)(c + 1ull), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            atomicExch(ticket, 0ull);
        }
    }
}

// ---- pit_batch_feed_points: the same launch, delivering a random subset of each cloud's points ---------------------------------------
// A point field's destination row - m_g points of `pw` words - is cut into pieces of words like any row; a piece touches the
// points [a / pw, (b - 1) / pw].  The workgroup forms the source point of each of them ONCE, FEED_PTS_CHUNK at a time, in LDS
// (one cycle walk per point, not per word), then moves the chunk's words with consecutive lanes on consecutive DESTINATION
// words: stores are coalesced, loads are segments of one point's pw words.  A destination point beyond M = min(m_g, L) has
// the entry -1 and its words load from an offset beyond every resource: the range check returns zero words, which is what
// those points are defined to hold.  The source resource spans exactly the sample's L points of the field.
constexpr int FEED_PTS_CHUNK = 2048;            // points whose indices a workgroup holds at a time (8 KiB of LDS)
constexpr unsigned FEED_OFF_NONE = 0x80000000u; // a byte offset beyond every resource (a field is at most 1 GiB per sample)

struct FeedPointFields {
    FeedFields f;
    int kind[PIT_FEED_MAX_FIELDS];              // PIT_FEED_WHOLE_ROW, PIT_FEED_POINTS_G0, PIT_FEED_POINTS_G1
    int pw[PIT_FEED_MAX_FIELDS];                // words per point (point fields)
    int n_pts[2], m_pts[2];                     // n_g, m_g
    int writer[2];                              // the field of group g whose workgroups write len_dst_g and points_g (-1: none)
    const int* len_src[2];
    int* len_dst[2];
    int* points[2];
};

// the keyed permutation with the four round keys formed by the caller (feistel() above, same arithmetic)
__device__ __forceinline__ uint32_t feistel_keyed(uint32_t n, int half, uint32_t mask, const uint32_t (&key)[4], uint32_t g) {
    uint32_t x = g;
    // Terminates: one pass of the rounds is a permutation of [0, 2^bits) and g < n lies on one of its cycles; following that
    // cycle from g re-enters [0, n) - at g itself at the latest - so a value below n comes after at most 2^bits - n + 1 passes
    // (the domain is < 4n, or 4 for n <= 2).
    do {
        uint32_t L = x >> half, R = x & mask;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const uint32_t t = L ^ (fmix(R + key[j]) & mask);
            L = R;
            R = t;
        }
        x = (L << half) | R;
    } while (x >= n);
    return x;
}

template <int FEED_T>
__global__ __launch_bounds__(FEED_T) void batch_feed_points_kernel(FeedPointFields pf, uint32_t n_samples,
                                                                   int batch, long long rank, long long world, long long steps,
                                                                   int shuffle, const int* __restrict__ order, long long seed,
                                                                   long long* state, int* __restrict__ indices,
                                                                   int* __restrict__ n_valid) {
    __shared__ int pts[FEED_PTS_CHUNK];
    const int tid = threadIdx.x;
    const int s = blockIdx.y, part = blockIdx.x;
    // the cursor: read by EVERY workgroup before its ticket, rewritten by the last arriver alone (batch_feed_kernel's rule)
    const long long cursor = __hip_atomic_load(state, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const unsigned long long c = cursor > 0 ? (unsigned long long)cursor : 0ull;
    const unsigned long long epoch = c / (unsigned long long)steps, i = c % (unsigned long long)steps;
    const long long first = ((long long)i * world + rank) * batch;     // global position of slot 0
    const uint32_t pos = (uint32_t)((unsigned long long)(first + s) % n_samples);
    const uint32_t e32 = (uint32_t)(epoch & 0xffffffffull);
    uint32_t idx;
    if (order) {
        const int v = order[pos];
        idx = (uint32_t)min(max(v, 0), (int)(n_samples - 1u));
    } else if (!shuffle) {
        idx = pos;
    } else {
        idx = feistel(n_samples, seed, e32, pos);
    }
    if (part == 0 && tid == 0) {
        if (indices) indices[s] = (int)idx;
        if (n_valid && s == 0) {
            const long long left = (long long)n_samples - first;
            *n_valid = (int)min(max(left, 0ll), (long long)batch);
        }
    }
    idx = (uint32_t)__builtin_amdgcn_readfirstlane((int)idx);          // (the same in every lane: the buffer resources stay scalar)
    int f = 0;
    while (f + 1 < pf.f.n && part >= pf.f.first_part[f + 1]) ++f;
    const long words = pf.f.words[f];                                  // of the DESTINATION row
    const long a = min(words, (long)(part - pf.f.first_part[f]) * pf.f.piece[f]), b = min(words, a + pf.f.piece[f]);
    const int kind = pf.kind[f];
    if (kind == PIT_FEED_WHOLE_ROW) {
        const char* src = pf.f.src[f] + ((long)idx * words + a) * 4;
        char* dst = pf.f.dst[f] + ((long)s * words + a) * 4;
        copy_run<FEED_T>(src, dst, (unsigned)(b - a), tid);
    } else {
        const int g = kind - PIT_FEED_POINTS_G0;
        const uint32_t n_g = (uint32_t)pf.n_pts[g], m_g = (uint32_t)pf.m_pts[g], pw = (uint32_t)pf.pw[f];
        uint32_t L = n_g;
        if (pf.len_src[g]) L = (uint32_t)min(max(pf.len_src[g][idx], 1), (int)n_g);
        L = (uint32_t)__builtin_amdgcn_readfirstlane((int)L);
        const uint32_t M = min(m_g, L);
        // the group's key and its four round keys (feistel()'s schedule with key in the place of seed)
        const unsigned long long key64 = (unsigned long long)seed ^
            (((unsigned long long)idx + 1ull) * 0x9E3779B97F4A7C15ull + (unsigned long long)g * 0xD1B54A32D192ED03ull);
        const uint32_t lo = (uint32_t)(key64 & 0xffffffffull), hi = (uint32_t)(key64 >> 32);
        uint32_t key[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) key[j] = fmix(lo ^ fmix(hi + 0x9E3779B9u * (e32 + 1u) + (uint32_t)j));
        int bits = 32 - __builtin_clz((L - 1u) | 1u);
        if (L <= 1u) bits = 0;
        bits = max(2, bits);
        bits += bits & 1;
        const int half = bits / 2;
        const uint32_t mask = (1u << half) - 1u;
        const bool writer = pf.writer[g] == f;
        if (writer && a == 0 && tid == 0 && pf.len_dst[g]) pf.len_dst[g][s] = (int)M;
        int* table = writer && pf.points[g] ? pf.points[g] + (long)s * m_g : nullptr;
        // the sample's L points of this field, and nothing behind them
        const __amdgpu_buffer_rsrc_t sr = make_rsrc(pf.f.src[f] + (long)idx * n_g * pw * 4, L * pw * 4u);
        char* drow = pf.f.dst[f] + (long)s * words * 4;
        const uint32_t ua = (uint32_t)a, ub = (uint32_t)b;            // (a destination row is below 2^28 words)
        const uint32_t p_end = ub > ua ? (ub - 1u) / pw + 1u : 0u;
        for (uint32_t pc = ua / pw; pc < p_end; pc += FEED_PTS_CHUNK) {
            const uint32_t np = min((uint32_t)FEED_PTS_CHUNK, p_end - pc);
            for (uint32_t t = tid; t < np; t += FEED_T) {
                const uint32_t k = pc + t;
                const int v = k < M ? (int)feistel_keyed(L, half, mask, key, k) : -1;
                pts[t] = v;
                if (table && k * pw >= ua) table[k] = v;              // (the piece that holds the point's first word)
            }
            __syncthreads();
            const uint32_t wa = max(ua, pc * pw), wb = min(ub, (pc + np) * pw), nw = wb - wa;
            const __amdgpu_buffer_rsrc_t dr = make_rsrc(drow + (long)wa * 4, nw * 4u);
            for (uint32_t j0 = 0; j0 < nw; j0 += FEED_DEEP_W * FEED_T) {
                int v[FEED_DEEP_W];
#pragma unroll
                for (int u = 0; u < FEED_DEEP_W; ++u) {
                    const uint32_t j = j0 + u * FEED_T + tid;
                    unsigned off = FEED_OFF_NONE;
                    if (j < nw) {
                        const uint32_t w = wa + j, p = w / pw;
                        const int q = pts[p - pc];
                        if (q >= 0) off = ((uint32_t)q * pw + (w - p * pw)) * 4u;
                    }
                    v[u] = __builtin_amdgcn_raw_buffer_load_b32(sr, (int)off, 0, 0);
                }
#pragma unroll
                for (int u = 0; u < FEED_DEEP_W; ++u)
                    __builtin_amdgcn_raw_buffer_store_b32(v[u], dr, (int)((j0 + u * FEED_T + tid) * 4u), 0, 0);
            }
            __syncthreads();
        }
    }
    __syncthreads();
    if (tid == 0) {
        // (no fence: see batch_feed_kernel)
        unsigned long long* ticket = reinterpret_cast<unsigned long long*>(state + 1);
        if (atomicAdd(ticket, 1ull) == (unsigned long long)gridDim.x * gridDim.y - 1ull) {
            __hip_atomic_store(state, (long long)(c + 1ull), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            atomicExch(ticket, 0ull);
        }
    }
}

}  // namespace

extern "C" int pit_batch_feed_points(const void* const* src, void* const* dst, const long* bytes, const int* kind, int n_fields,
                                     int n0, int m0, int n1, int m1, const int* len_src0, const int* len_src1, int* len_dst0,
                                     int* len_dst1, int* points0, int* points1, long n_samples, int batch, int rank, int world,
                                     int drop_last, int shuffle, const int* order, long long seed, long long* state,
                                     int* indices, int* n_valid, void* stream) {
    if (!src || !dst || !bytes || !kind || !state) return PIT_ERR_NULL;
    if (n_fields < 1 || n_fields > PIT_FEED_MAX_FIELDS) return PIT_ERR_SIZE;
    for (int f = 0; f < n_fields; ++f)
        if (!src[f] || !dst[f]) return PIT_ERR_NULL;
    if (n_samples <= 0 || batch <= 0 || batch > 65535 || world <= 0 || rank < 0 || rank >= world) return PIT_ERR_SIZE;
    if ((drop_last & ~1) || (shuffle & ~1)) return PIT_ERR_SIZE;
    FeedPointFields pf = {};
    const int n_pts[2] = {n0, n1}, m_pts[2] = {m0, m1};
    const int* const len_src[2] = {len_src0, len_src1};
    int* const len_dst[2] = {len_dst0, len_dst1};
    int* const points[2] = {points0, points1};
    pf.writer[0] = pf.writer[1] = -1;
    for (int f = 0; f < n_fields; ++f) {
        if (kind[f] < PIT_FEED_WHOLE_ROW || kind[f] > PIT_FEED_POINTS_G1) return PIT_ERR_SIZE;
        if (bytes[f] <= 0 || (bytes[f] & 3)) return PIT_ERR_SIZE;
        if (((uintptr_t)src[f] | (uintptr_t)dst[f]) & 3u) return PIT_ERR_SIZE;            // moved as aligned words
        if (kind[f] != PIT_FEED_WHOLE_ROW) {
            const int g = kind[f] - PIT_FEED_POINTS_G0;
            if (n_pts[g] < 1) return PIT_ERR_SIZE;                     // a point field whose group has no widths
            if (pf.writer[g] < 0) pf.writer[g] = f;
        }
    }
    for (int g = 0; g < 2; ++g) {
        if (pf.writer[g] >= 0 && (m_pts[g] < 1 || m_pts[g] > n_pts[g])) return PIT_ERR_SIZE;
        if (((uintptr_t)len_src[g] | (uintptr_t)len_dst[g] | (uintptr_t)points[g]) & 3u) return PIT_ERR_SIZE;
        if (pf.writer[g] < 0 && (len_src[g] || len_dst[g] || points[g])) return PIT_ERR_SIZE;     // nothing would write them
        pf.n_pts[g] = n_pts[g];
        pf.m_pts[g] = m_pts[g];
        pf.len_src[g] = len_src[g];
        pf.len_dst[g] = len_dst[g];
        pf.points[g] = points[g];
    }
    const long per_step = (long)batch * world;
    if (drop_last && n_samples < per_step) return PIT_ERR_SIZE;        // no full step
    if (n_samples > 0x7fffffffL) return PIT_ERR_UNSUPPORTED;
    long total_words = 0;
    for (int f = 0; f < n_fields; ++f) {
        const bool whole = kind[f] == PIT_FEED_WHOLE_ROW;
        const int g = whole ? 0 : kind[f] - PIT_FEED_POINTS_G0;
        // a sample's field is one buffer resource (bytes[f] < 2^62 here, n_g < 2^31: the quotient form cannot overflow)
        if (bytes[f] > PIT_FEED_MAX_ROW_BYTES / (whole ? 1 : n_pts[g])) return PIT_ERR_UNSUPPORTED;
        pf.f.src[f] = static_cast<const char*>(src[f]);
        pf.f.dst[f] = static_cast<char*>(dst[f]);
        pf.kind[f] = kind[f];
        pf.pw[f] = whole ? 0 : (int)(bytes[f] / 4);
        pf.f.words[f] = whole ? bytes[f] / 4 : (bytes[f] / 4) * m_pts[g];
        total_words += pf.f.words[f];
    }
    pf.f.n = n_fields;
    const long steps = drop_last ? n_samples / per_step : (n_samples + per_step - 1) / per_step;
    // pit_batch_feed's cut, on the words of the DESTINATION rows
    const bool small = total_words * batch <= FEED_SMALL_WORDS;
    const int threads = small ? FEED_T_SMALL : FEED_T_LARGE;
    const long slot_parts = std::max(1L, FEED_FILL / batch);
    long target = std::max(FEED_MIN_WORDS * threads, (total_words + slot_parts - 1) / slot_parts);
    target = (target + 3) & ~3L;
    long parts = 0;
    for (int f = 0; f < n_fields; ++f) {
        pf.f.first_part[f] = (int)parts;
        pf.f.piece[f] = target;
        parts += (pf.f.words[f] + target - 1) / target;
    }
    const dim3 grid((unsigned)parts, (unsigned)batch);
    if (small)
        hipLaunchKernelGGL(batch_feed_points_kernel<FEED_T_SMALL>, grid, dim3(FEED_T_SMALL), 0, (hipStream_t)stream, pf,
                           (uint32_t)n_samples, batch, (long long)rank, (long long)world, (long long)steps, shuffle, order, seed,
                           state, indices, n_valid);
    else
        hipLaunchKernelGGL(batch_feed_points_kernel<FEED_T_LARGE>, grid, dim3(FEED_T_LARGE), 0, (hipStream_t)stream, pf,
                           (uint32_t)n_samples, batch, (long long)rank, (long long)world, (long long)steps, shuffle, order, seed,
                           state, indices, n_valid);
    PIT_CHECK_LAUNCH();
    return 0;
}

extern "C" int pit_batch_feed(const void* const* src, void* const* dst, const long* row_bytes, int n_fields, long n_samples,
                              int batch, int rank, int world, int drop_last, int shuffle, const int* order, long long seed,
                              long long* state, int* indices, int* n_valid, void* stream) {
    if (!src || !dst || !row_bytes || !state) return PIT_ERR_NULL;
    if (n_fields < 1 || n_fields > PIT_FEED_MAX_FIELDS) return PIT_ERR_SIZE;
    for (int f = 0; f < n_fields; ++f)
        if (!src[f] || !dst[f]) return PIT_ERR_NULL;
    if (n_samples <= 0 || batch <= 0 || batch > 65535 || world <= 0 || rank < 0 || rank >= world) return PIT_ERR_SIZE;
    if ((drop_last & ~1) || (shuffle & ~1)) return PIT_ERR_SIZE;
    FeedFields fields = {};
    long total_words = 0;
    for (int f = 0; f < n_fields; ++f) {
        if (row_bytes[f] <= 0 || (row_bytes[f] & 3)) return PIT_ERR_SIZE;
        if (((uintptr_t)src[f] | (uintptr_t)dst[f]) & 3u) return PIT_ERR_SIZE;            // rows are moved as aligned words
        fields.src[f] = static_cast<const char*>(src[f]);
        fields.dst[f] = static_cast<char*>(dst[f]);
        fields.words[f] = row_bytes[f] / 4;
        total_words += fields.words[f];
    }
    fields.n = n_fields;
    const long per_step = (long)batch * world;
    if (drop_last && n_samples < per_step) return PIT_ERR_SIZE;        // no full step
    if (n_samples > 0x7fffffffL) return PIT_ERR_UNSUPPORTED;
    for (int f = 0; f < n_fields; ++f)
        if (row_bytes[f] > PIT_FEED_MAX_ROW_BYTES) return PIT_ERR_UNSUPPORTED;     // a piece is one buffer resource
    const long steps = drop_last ? n_samples / per_step : (n_samples + per_step - 1) / per_step;
    // the piece every field is cut by: FEED_MIN_WORDS per thread, larger once a slot's pieces times the batch would exceed FEED_FILL
    const bool small = total_words * batch <= FEED_SMALL_WORDS;
    const int threads = small ? FEED_T_SMALL : FEED_T_LARGE;
    const long slot_parts = std::max(1L, FEED_FILL / batch);
    long target = std::max(FEED_MIN_WORDS * threads, (total_words + slot_parts - 1) / slot_parts);
    target = (target + 3) & ~3L;                                       // (whole 16-byte units: a cut adds no heads or tails of its own)
    long parts = 0;
    for (int f = 0; f < n_fields; ++f) {
        fields.first_part[f] = (int)parts;
        fields.piece[f] = target;
        parts += (fields.words[f] + target - 1) / target;              // (at most slot_parts + n_fields in all)
    }
    const dim3 grid((unsigned)parts, (unsigned)batch);
    if (small)
        hipLaunchKernelGGL(batch_feed_kernel<FEED_T_SMALL>, grid, dim3(FEED_T_SMALL), 0, (hipStream_t)stream, fields, (uint32_t)n_samples,
                           batch, (long long)rank, (long long)world, (long long)steps, shuffle, order, seed, state, indices, n_valid);
    else
        hipLaunchKernelGGL(batch_feed_kernel<FEED_T_LARGE>, grid, dim3(FEED_T_LARGE), 0, (hipStream_t)stream, fields, (uint32_t)n_samples,
                           batch, (long long)rank, (long long)world, (long long)steps, shuffle, order, seed, state, indices, n_valid);
    PIT_CHECK_LAUNCH();
    return 0;
}
