// Farthest-point sampling of per-sample point clouds (include/pit_hip.h, pit_fps): the latent mesh of a cloud model, m << n
// points chosen from each cloud itself.  One launch, one workgroup per sample; the workgroup runs the whole sequential selection
// of its sample, so the cost is m times the critical path of one pick, not bandwidth.
//
// Every thread keeps PPT points - coordinates and running distance - in registers (point k * THREADS + tid in slot k), loaded once
// through a buffer resource that spans exactly the sample's L real points: a slot beyond the end reads zeros and starts with
// distance 0, which - behind every real point in index order - can never be picked, so the loop has no predicate.  A pick:
//   every thread folds its points into one candidate (distance bits, index, coordinates); distances are >= 0, so their bit
//   patterns order as unsigned integers and the running minimum and the maximum are integer operations;
//   two maxima over the wave on DPP lanes (pit_common.h's wave_sum with v_max_u32, which takes the DPP operand itself): the
//   largest distance, then the largest ~index among the lanes that hold it - the lowest index among equals.  The one lane that
//   holds both writes (~index, distance bits) and its coordinates to the wave's LDS slot;
//   ONE barrier; lane l of every wave reads the pair of slot l % waves, the same two maxima within the 16-lane row give every wave
//   the workgroup's winner, whose coordinates are one more (broadcast) LDS read away.  The slots are double-buffered by the parity
//   of the pick: a wave that runs ahead writes the other set, and cannot lap a wave that still reads, because the next barrier
//   stands between them.
// The loop touches global memory only to store the picked point.  No atomics: the same input gives the same bits.
#include "pit_common.h"

namespace {

template <int CTRL, int ROW_MASK>
__device__ __forceinline__ unsigned dpp_max_u32(unsigned v) {
    // (lanes outside ROW_MASK and sources outside the wave read 0: the identity of an unsigned maximum)
    return max(v, (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, ROW_MASK, 0xf, true));
}
// the maximum over the 16 lanes of every row, in every lane of the row
__device__ __forceinline__ unsigned row_max_u32(unsigned v) {
    v = dpp_max_u32<0xB1, 0xf>(v);                       // quad_perm(1,0,3,2)
    v = dpp_max_u32<0x4E, 0xf>(v);                       // quad_perm(2,3,0,1)
    v = dpp_max_u32<0x124, 0xf>(v);                      // row_ror:4
    v = dpp_max_u32<0x128, 0xf>(v);                      // row_ror:8
    return v;
}
// the maximum over the wave, in every lane
__device__ __forceinline__ unsigned wave_max_u32(unsigned v) {
    v = row_max_u32(v);
    v = dpp_max_u32<0x142, 0xa>(v);                      // row_bcast:15 -> rows 1 and 3
    v = dpp_max_u32<0x143, 0xc>(v);                      // row_bcast:31 -> rows 2 and 3
    return (unsigned)__builtin_amdgcn_readlane((int)v, 63);
}

// MAXD coordinates per point, zero beyond space_dim: a zero coordinate adds (0 - 0)^2 = +0 to the distance, which leaves its bits
// as they are, so one instance serves every space_dim up to MAXD
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

template <int THREADS, int PPT, int MAXD>
__global__ __launch_bounds__(THREADS) void fps_kernel(const float* __restrict__ mesh, int n, int sdim, long mesh_bstride,
                                                      const int* __restrict__ lengths, const int* __restrict__ start, int start_all,
                                                      int m, int* __restrict__ idx, float* __restrict__ out_mesh,
                                                      int* __restrict__ out_len) {
    constexpr int WAVES = THREADS / PIT_WAVE;
    static_assert(WAVES >= 1 && WAVES <= 16 && (WAVES & (WAVES - 1)) == 0, "the slots of one pick are reduced within a 16-lane row");
    constexpr int SLOT = MAXD <= 3 ? 4 : 8;              // floats per slot's coordinates
    __shared__ uint2 s_key[2][16];                      // (~index, distance bits) of every wave's candidate
    __shared__ __attribute__((aligned(16))) float s_pt[2][16][SLOT];
    const int tid = threadIdx.x, lane = tid & (PIT_WAVE - 1), wave = tid / PIT_WAVE;
    const int s = blockIdx.x;
    const int L = min(max(lengths ? lengths[s] : n, 1), n);
    const int picks = min(m, L);
    const float* cloud = mesh + (long)s * mesh_bstride;
    int* idx_s = idx + (long)s * m;
    float* out_s = out_mesh + (long)s * m * sdim;

    // the slots beyond the picks, and the count
    for (int t = picks + tid; t < m; t += THREADS) idx_s[t] = -1;
    for (int t = picks * sdim + tid; t < m * sdim; t += THREADS) out_s[t] = 0.0f;
    if (out_len && tid == 0) out_len[s] = picks;

    // this thread's points: one pass over the cloud
    const __amdgpu_buffer_rsrc_t rs = make_rsrc(cloud, (unsigned)L * (unsigned)sdim * 4u);
    fps_pt<MAXD> p[PPT];
    unsigned dist[PPT];                                  // (the bits of a distance >= 0: they order as unsigned integers)
#pragma unroll
    for (int k = 0; k < PPT; ++k) {
        const unsigned i = (unsigned)(k * THREADS + tid);
#pragma unroll
        for (int c = 0; c < MAXD; ++c)
            p[k].c[c] = c < sdim ? buf_load(rs, (i * (unsigned)sdim + (unsigned)c) * 4u) : 0.0f;     // (beyond the range: 0)
        dist[k] = (int)i < L ? __float_as_uint(__builtin_inff()) : 0u;
    }

    int cur = min(max(start ? start[s] : start_all, 0), L - 1);
    fps_pt<MAXD> pc;
#pragma unroll
    for (int c = 0; c < MAXD; ++c) pc.c[c] = c < sdim ? buf_load(rs, ((unsigned)cur * (unsigned)sdim + (unsigned)c) * 4u) : 0.0f;

    for (int t = 0; t < picks; ++t) {
        if (tid == 0) {
            idx_s[t] = cur;
#pragma unroll
            for (int c = 0; c < MAXD; ++c)
                if (c < sdim) out_s[(long)t * sdim + c] = pc.c[c];
        }
        if (t + 1 == picks) break;
        // this thread's candidate: its slots hold ascending indices, so a strict comparison keeps the lowest index of a tie
        unsigned best_d = 0u, best_i = 0u;
        fps_pt<MAXD> best_p;
#pragma unroll
        for (int k = 0; k < PPT; ++k) {
            dist[k] = min(dist[k], __float_as_uint(fps_dist<MAXD>(p[k], pc)));
            const unsigned b = dist[k];
            const bool take = k == 0 || b > best_d;
            best_d = take ? b : best_d;
            best_i = take ? (unsigned)(k * THREADS + tid) : best_i;
#pragma unroll
            for (int c = 0; c < MAXD; ++c) best_p.c[c] = take ? p[k].c[c] : best_p.c[c];
        }
        // the wave's largest distance, then the largest ~index among the lanes that hold it (never 0: indices stay below 2^14)
        const unsigned wave_d = wave_max_u32(best_d);
        const unsigned mine = best_d == wave_d ? ~best_i : 0u;
        const unsigned wave_i = wave_max_u32(mine);
        const int par = t & 1;
        if (mine == wave_i) {                            // (indices are unique: exactly one lane)
            s_key[par][wave] = make_uint2(wave_i, wave_d);
#pragma unroll
            for (int c = 0; c < MAXD; ++c) s_pt[par][wave][c] = best_p.c[c];
        }
        __syncthreads();
        const uint2 slot = s_key[par][lane & (WAVES - 1)];
        const unsigned all_d = WAVES > 1 ? row_max_u32(slot.y) : slot.y;
        const unsigned cand = slot.y == all_d ? slot.x : 0u;
        const unsigned all = (unsigned)__builtin_amdgcn_readlane((int)(WAVES > 1 ? row_max_u32(cand) : cand), 0);
        const unsigned win = ~all;             // the picked index
        cur = (int)min(win, (unsigned)(L - 1));          // (a real point always wins; clamped whatever the coordinates hold)
        const int wslot = (cur & (THREADS - 1)) / PIT_WAVE;       // the wave that holds point `cur`
#pragma unroll
        for (int c = 0; c < MAXD; ++c) pc.c[c] = s_pt[par][wslot][c];
    }
}

template <int THREADS, int PPT, int MAXD>
void fps_launch(const float* mesh, int batch, int n, int sdim, long mesh_bstride, const int* lengths, const int* start,
                int start_all, int m, int* idx, float* out_mesh, int* out_len, hipStream_t stream) {
    hipLaunchKernelGGL((fps_kernel<THREADS, PPT, MAXD>), dim3((unsigned)batch), dim3(THREADS), 0, stream, mesh, n, sdim,
                       mesh_bstride, lengths, start, start_all, m, idx, out_mesh, out_len);
}

}  // namespace

extern "C" int pit_fps(const float* mesh, int batch, int n, int space_dim, long mesh_bstride, const int* lengths,
                       const int* start, int start_all, int m, int* idx, float* out_mesh, int* out_len, void* stream) {
    if (!mesh || !idx || !out_mesh) return PIT_ERR_NULL;
    if (batch < 1 || batch > 65535 || n < 1 || m < 1 || m > n) return PIT_ERR_SIZE;
    if (space_dim < 1 || space_dim > PIT_MAX_SPACE_DIM) return PIT_ERR_SIZE;
    if (mesh_bstride < (long)n * space_dim) return PIT_ERR_SIZE;
    if (n > (space_dim <= 3 ? PIT_FPS_MAX_POINTS : PIT_FPS_MAX_POINTS_WIDE)) return PIT_ERR_UNSUPPORTED;
    hipStream_t st = (hipStream_t)stream;
    if (space_dim <= 3) {
        if (n <= 1024) fps_launch<256, 4, 3>(mesh, batch, n, space_dim, mesh_bstride, lengths, start, start_all, m, idx, out_mesh, out_len, st);
        else if (n <= 4096) fps_launch<1024, 4, 3>(mesh, batch, n, space_dim, mesh_bstride, lengths, start, start_all, m, idx, out_mesh, out_len, st);
        else fps_launch<1024, 16, 3>(mesh, batch, n, space_dim, mesh_bstride, lengths, start, start_all, m, idx, out_mesh, out_len, st);
    } else {
        if (n <= 1024) fps_launch<256, 4, 8>(mesh, batch, n, space_dim, mesh_bstride, lengths, start, start_all, m, idx, out_mesh, out_len, st);
        else fps_launch<1024, 4, 8>(mesh, batch, n, space_dim, mesh_bstride, lengths, start, start_all, m, idx, out_mesh, out_len, st);
    }
    PIT_CHECK_LAUNCH();
    return 0;
}
