// Farthest-point sampling of clouds of any size (include/pit_hip.h, pit_fps_large): the semantics of pit_fps (pit_fps.hip), bit for
// bit, with the points in memory instead of one workgroup's registers.  A cloud is cut into slices of slice_points points, one
// workgroup each, and ONE kernel serves every pick: m launches of grid (slices, batch) per sampling, the hand-off between two
// picks being the kernel boundary (an ordinary dependent launch).  Launch t:
//   the current point: every WAVE of every workgroup of sample s reads the candidates (distance bits, ~index) that launch t - 1
//   wrote for the sample's slices - 8 bytes each, lane l the candidates l, l + 64, ... - and reduces them itself with two maxima
//   on DPP lanes: the largest distance bits, then the largest ~index among equals (the lowest index).  All waves of a sample
//   compute the same winner, so nothing is communicated inside a launch, and this step has no LDS and no barrier;
//   the workgroup of slice 0 stores the pick; launch 0 also writes the slots beyond the picks and the count;
//   every workgroup folds the distance to the current point into the running distances of its slice (the workspace; launch 0
//   starts them at +inf and reads nothing), and writes the slice's candidate into the set of parity t & 1 - launch t reads the
//   set of parity (t - 1) & 1, so no launch reads what it writes.
// No atomics, no spin-waits, no grid barrier, no tickets: visibility between picks comes from the kernel boundary alone, and the
// same input gives the same bits.  The arithmetic of a distance, the unsigned order of distance bits and the tie rule are
// pit_fps.hip's, restated here (that unit is not touched, so its instances keep their registers).
#include "pit_common.h"

namespace {

constexpr int FPSL_THREADS = 256;
constexpr int FPSL_WAVES = FPSL_THREADS / PIT_WAVE;
constexpr int FPSL_CHUNK = 4;                            // points per thread whose loads are in flight together

template <int CTRL, int ROW_MASK>
__device__ __forceinline__ unsigned dpp_max_u32(unsigned v) {
    // (lanes outside ROW_MASK and sources outside the wave read 0: the identity of an unsigned maximum)
    return max(v, (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, ROW_MASK, 0xf, true));
}
// the maximum over the wave, in every lane
__device__ __forceinline__ unsigned wave_max_u32(unsigned v) {
    v = dpp_max_u32<0xB1, 0xf>(v);                       // quad_perm(1,0,3,2)
    v = dpp_max_u32<0x4E, 0xf>(v);                       // quad_perm(2,3,0,1)
    v = dpp_max_u32<0x124, 0xf>(v);                      // row_ror:4
    v = dpp_max_u32<0x128, 0xf>(v);                      // row_ror:8
    v = dpp_max_u32<0x142, 0xa>(v);                      // row_bcast:15 -> rows 1 and 3
    v = dpp_max_u32<0x143, 0xc>(v);                      // row_bcast:31 -> rows 2 and 3
    return (unsigned)__builtin_amdgcn_readlane((int)v, 63);
}
// a candidate is (~index, distance bits): the larger distance wins, then the larger ~index - the lowest index.  ~index is never
// 0 (indices stay below 2^22), so a lane that holds no candidate offers (0, 0) and loses to every real one.
__device__ __forceinline__ uint2 wave_best(uint2 key) {
    const unsigned d = wave_max_u32(key.y);
    const unsigned i = wave_max_u32(key.y == d ? key.x : 0u);
    return make_uint2(i, d);
}
__device__ __forceinline__ bool key_less(uint2 a, uint2 b) { return a.y < b.y || (a.y == b.y && a.x < b.x); }

// MAXD coordinates per point, +0 beyond space_dim: (0 - 0)^2 = +0 leaves the bits of a sum >= 0 as they are
template <int MAXD> struct fps_pt { float c[MAXD]; };

template <int MAXD>
__device__ __forceinline__ float fps_dist(const fps_pt<MAXD>& p, const fps_pt<MAXD>& q) {
    float e = __fsub_rn(p.c[0], q.c[0]);
    float d = __fmul_rn(e, e);
#pragma unroll
    for (int k = 1; k < MAXD; ++k) {
        e = __fsub_rn(p.c[k], q.c[k]);
        d = __fadd_rn(d, __fmul_rn(e, e));
    }
    return d;
}

template <int MAXD>
__device__ __forceinline__ fps_pt<MAXD> load_pt(__amdgpu_buffer_rsrc_t rs, unsigned i, int sdim) {
    fps_pt<MAXD> p;
#pragma unroll
    for (int c = 0; c < MAXD; ++c) p.c[c] = c < sdim ? buf_load(rs, (i * (unsigned)sdim + (unsigned)c) * 4u) : 0.0f;   // (beyond the range: 0)
    return p;
}

// cand: two sets of batch * slices candidates; dist: batch * n running distances (bits).  Neither needs initial contents: launch 0
// writes every distance it or a later launch reads, and launch t reads only candidates that launch t - 1 wrote.
template <int MAXD>
__global__ __launch_bounds__(FPSL_THREADS) void fps_large_kernel(const float* __restrict__ mesh, int n, int sdim, long mesh_bstride,
                                                                 const int* __restrict__ lengths, const int* __restrict__ start,
                                                                 int start_all, int m, int t, int slice_points, int* __restrict__ idx,
                                                                 float* __restrict__ out_mesh, int* __restrict__ out_len, uint2* cand,
                                                                 unsigned* __restrict__ dist) {
    __shared__ uint2 s_key[FPSL_WAVES];
    const int tid = threadIdx.x, lane = tid & (PIT_WAVE - 1), wave = tid / PIT_WAVE;
    const int slice = blockIdx.x, slices = gridDim.x, s = blockIdx.y, batch = gridDim.y;
    const int first = slice * slice_points;              // (< n <= 2^22)
    unsigned* dist_s = dist + (long)s * n;
    constexpr unsigned INF = 0x7f800000u;

    // A launch is a chain of dependent memory round trips (length -> candidates -> current point -> distances), so everything
    // whose address is known goes out before the first wait: the running distances of the slice's first FPSL_CHUNK points per
    // thread, which depend on nothing (inside the workspace whatever L is; a value at or beyond L is dropped below) ...
    unsigned old[FPSL_CHUNK];
#pragma unroll
    for (int k = 0; k < FPSL_CHUNK; ++k) {
        const int i = first + k * FPSL_THREADS + tid;
        old[k] = (t > 0 && i < n && k * FPSL_THREADS < slice_points) ? dist_s[i] : INF;
    }
    // ... and the candidates of the previous launch (a wave folds more than 64 slices as it reads them)
    uint2 key = make_uint2(0u, 0u);
    if (t > 0) {
        const uint2* prev = cand + ((long)((t - 1) & 1) * batch + s) * slices;
        for (int j = lane; j < slices; j += PIT_WAVE) {
            const uint2 c = prev[j];
            key = key_less(key, c) ? c : key;
        }
    }
    const int L = min(max(lengths ? lengths[s] : n, 1), n);
    const int picks = min(m, L);
    if (t >= picks) return;                              // (uniform over the workgroup; launch 0 always runs: picks >= 1)
    const float* cloud = mesh + (long)s * mesh_bstride;
    const __amdgpu_buffer_rsrc_t rs = make_rsrc(cloud, (unsigned)L * (unsigned)sdim * 4u);
    const int last = min(first + slice_points, L);
    fps_pt<MAXD> p[FPSL_CHUNK];                          // (a point at or beyond L reads zeros and is not used)
#pragma unroll
    for (int k = 0; k < FPSL_CHUNK; ++k)
        if (k * FPSL_THREADS < slice_points) p[k] = load_pt<MAXD>(rs, (unsigned)(first + k * FPSL_THREADS + tid), sdim);

    // the current point
    int cur;
    if (t == 0) {
        cur = min(max(start ? start[s] : start_all, 0), L - 1);
    } else {
        key = wave_best(key);
        cur = (int)min(~key.x, (unsigned)(L - 1));       // (a real point always wins; clamped whatever the coordinates hold)
    }
    const fps_pt<MAXD> pc = load_pt<MAXD>(rs, (unsigned)cur, sdim);

    // the pick; launch 0: the slots beyond the picks, and the count
    if (slice == 0) {
        int* idx_s = idx + (long)s * m;
        float* out_s = out_mesh + (long)s * m * sdim;
        if (tid == 0) {
            idx_s[t] = cur;
#pragma unroll
            for (int c = 0; c < MAXD; ++c)
                if (c < sdim) out_s[(long)t * sdim + c] = pc.c[c];
        }
        if (t == 0) {
            for (int u = picks + tid; u < m; u += FPSL_THREADS) idx_s[u] = -1;
            for (long u = (long)picks * sdim + tid; u < (long)m * sdim; u += FPSL_THREADS) out_s[u] = 0.0f;
            if (out_len && tid == 0) out_len[s] = picks;
        }
    }
    if (t + 1 >= picks) return;

    // this slice's running distances, and this thread's candidate: its points have ascending indices, so a strict comparison
    // keeps the lowest index of a tie.  Points at and beyond L have distance 0 and are not stored: behind every real point in
    // index order they can never win (a thread without a real point offers its first index with distance 0).
    unsigned best_d = 0u, best_i = (unsigned)(first + tid);
    for (int base = first;;) {
#pragma unroll
        for (int k = 0; k < FPSL_CHUNK; ++k) {
            const int i = base + k * FPSL_THREADS + tid;
            if (i < last) {
                const unsigned b = min(old[k], __float_as_uint(fps_dist<MAXD>(p[k], pc)));
                dist_s[i] = b;
                const bool take = b > best_d;
                best_d = take ? b : best_d;
                best_i = take ? (unsigned)i : best_i;
            }
        }
        base += FPSL_CHUNK * FPSL_THREADS;
        if (base >= last) break;                         // (uniform over the workgroup)
        // a slice of more than FPSL_CHUNK points per thread: the next chunk, all its loads before the first use
#pragma unroll
        for (int k = 0; k < FPSL_CHUNK; ++k) {
            const int i = base + k * FPSL_THREADS + tid;
            old[k] = (t > 0 && i < last) ? dist_s[i] : INF;
            p[k] = load_pt<MAXD>(rs, (unsigned)i, sdim);
        }
    }
    const uint2 mine = make_uint2(~best_i, best_d);
    const uint2 wbest = wave_best(mine);
    if (mine.x == wbest.x && mine.y == wbest.y) s_key[wave] = wbest;      // (indices are unique: exactly one lane)
    __syncthreads();
    if (tid == 0) {
        uint2 key = s_key[0];
#pragma unroll
        for (int w = 1; w < FPSL_WAVES; ++w) {
            const uint2 c = s_key[w];
            key = key_less(key, c) ? c : key;
        }
        cand[((long)(t & 1) * batch + s) * slices + slice] = key;
    }
}

// the library's slice: 1024 points (4 per thread) up to 262144 points, beyond that the multiple of 256 that gives 256 slices
int default_slice(int n) {
    const int per = ((n + 255) / 256 + 255) / 256 * 256;
    return per > 1024 ? per : 1024;
}

bool slice_ok(int slice_points) { return slice_points == 0 || (slice_points >= 256 && slice_points <= 65536 && slice_points % 256 == 0); }

}  // namespace

extern "C" long pit_fps_large_workspace(int batch, int n, int slice_points) {
    if (batch < 1 || batch > 65535 || n < 1 || n > PIT_FPS_LARGE_MAX_POINTS || !slice_ok(slice_points)) return 0;
    const int sp = slice_points ? slice_points : default_slice(n);
    const long slices = (n + sp - 1) / sp;
    return 2l * batch * slices * (long)sizeof(uint2) + (long)batch * n * (long)sizeof(unsigned);
}

extern "C" int pit_fps_large(const float* mesh, int batch, int n, int space_dim, long mesh_bstride, const int* lengths,
                             const int* start, int start_all, int m, int* idx, float* out_mesh, int* out_len, int slice_points,
                             void* workspace, void* stream) {
    if (!mesh || !idx || !out_mesh || !workspace) return PIT_ERR_NULL;
    if (batch < 1 || batch > 65535 || n < 1 || m < 1 || m > n) return PIT_ERR_SIZE;
    if (space_dim < 1 || space_dim > PIT_MAX_SPACE_DIM) return PIT_ERR_SIZE;
    if (mesh_bstride < (long)n * space_dim) return PIT_ERR_SIZE;
    if (!slice_ok(slice_points)) return PIT_ERR_SIZE;
    if (n > PIT_FPS_LARGE_MAX_POINTS || m > PIT_FPS_LARGE_MAX_SAMPLES) return PIT_ERR_UNSUPPORTED;
    const int sp = slice_points ? slice_points : default_slice(n);
    const int slices = (n + sp - 1) / sp;
    uint2* cand = (uint2*)workspace;
    unsigned* dist = (unsigned*)(cand + 2l * batch * slices);
    const dim3 grid((unsigned)slices, (unsigned)batch);
    hipStream_t st = (hipStream_t)stream;
    for (int t = 0; t < m; ++t) {
        if (space_dim <= 3)
            hipLaunchKernelGGL(fps_large_kernel<3>, grid, dim3(FPSL_THREADS), 0, st, mesh, n, space_dim, mesh_bstride, lengths, start,
                               start_all, m, t, sp, idx, out_mesh, out_len, cand, dist);
        else
            hipLaunchKernelGGL(fps_large_kernel<8>, grid, dim3(FPSL_THREADS), 0, st, mesh, n, space_dim, mesh_bstride, lengths, start,
                               start_all, m, t, sp, idx, out_mesh, out_len, cand, dist);
        PIT_CHECK_LAUNCH();
    }
    return 0;
}
