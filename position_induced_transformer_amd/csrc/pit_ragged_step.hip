// What a training step on a ragged batch launches around the model (engine.TrainStep with lengths), and the clouds' evaluation
// metric.  Kernels of their own: nothing in pit_ragged.hip / pit_loss.hip changes, so no existing instance's registers, LDS or
// bits can move.
//
// pit_rel_lp_loss_ragged_fwd_grad - RelLpNorm over the first len[s] points of every sample (utils.py:80-98 on the truncated
//   sample), its gradient for d loss = 1 and the clear of a caller buffer (the step's flat gradient accumulators) in ONE launch,
//   where pit_rel_lp_loss_ragged_fwd + pit_rel_lp_loss_ragged_bwd take three and the clear a memset.  The same bits as those two
//   entries: a (sample, channel) series belongs to one workgroup, which sums it as ragged_loss_norms_kernel does (stride-256 fp64
//   partials, wave_sum_d, the four wave sums in order) and then writes the unit gradient of its own series with
//   ragged_loss_bwd_kernel's expressions - no grid-wide dependency.  The clear is spread over all workgroups, and over planes
//   of clear-only workgroups when it is large.  The pairs' terms are added as ragged_loss_sum_kernel adds them
//   (64 lanes, stride 64, wave_sum_d) by the first wave of the workgroup that arrives LAST: an arrival ticket in `workspace`, zero
//   before the first call and left zero by every call.
// pit_rel_max_norm_ragged - RelMaxNorm (utils.py:59-77) of every truncated sample: forward only, one small launch, no workspace, every
//   sum in a fixed order.
//
// Padding is never read: every loop over a series ends at the clamped length.
#include "pit_common.h"

namespace {

// pit_ragged.hip's clamp: a bad length cannot address outside a buffer
__device__ __forceinline__ int clamp_len(const int* len, int s, int n) { return max(1, min(len[s], n)); }

__device__ __forceinline__ float rag_pow_abs(float x, int p) {
    const float ax = fabsf(x);
    if (p == 1) return ax;
    if (p == 2) return ax * ax;
    return powf(ax, (float)p);
}

// zero clear_n floats at clear_buf, spread over the whole grid: the head up to a 16-byte boundary and the tail in single floats,
// the body in float4
__device__ __forceinline__ void clear_slice(float* clear_buf, long clear_n) {
    const long nthreads = (long)gridDim.x * gridDim.y * gridDim.z * blockDim.x;
    const long first = (((long)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x) * blockDim.x + threadIdx.x;
    const long head = std::min<long>(clear_n, (long)((4u - (unsigned)((reinterpret_cast<uintptr_t>(clear_buf) >> 2) & 3u)) & 3u));
    const long quads = (clear_n - head) >> 2;
    const long tail0 = head + 4 * quads;
    float4* body = reinterpret_cast<float4*>(clear_buf + head);
    for (long i = first; i < quads; i += nthreads) body[i] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (first < head) clear_buf[first] = 0.0f;
    if (first < clear_n - tail0) clear_buf[tail0 + first] = 0.0f;
}

// one workgroup per (channel, sample) in the grid's z = 0 plane; the planes z > 0 (only with a large clear: a series is never
// split, so the loss alone would leave the clear to batch * nch workgroups) clear their slice and leave
__global__ __launch_bounds__(256) void ragged_loss_step_kernel(const float* __restrict__ tru, const float* __restrict__ pred,
                                                               const int* __restrict__ len, int npts, int nch, int p,
                                                               float* norms, float* __restrict__ loss, unsigned* ticket,
                                                               float* __restrict__ d_pred_unit, float* __restrict__ clear_buf,
                                                               long clear_n) {
    __shared__ double s_num[4], s_den[4];
    __shared__ float s_norm[2];
    __shared__ int s_last;
    if (clear_n > 0) clear_slice(clear_buf, clear_n);
    if (blockIdx.z > 0) return;
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
        s_norm[0] = (float)nn;
        s_norm[1] = (float)dn;
        norms[((long)s * nch + c) * 2 + 0] = (float)nn;
        norms[((long)s * nch + c) * 2 + 1] = (float)dn;
        // the pair's norms leave this CU (agent-scope release, its wait written out) BEFORE the ticket; the last arriver drops its
        // CU's stale lines (agent-scope acquire) before the barrier that lets its first wave read every pair's norms
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        const unsigned pairs = gridDim.x * gridDim.y;
        const int last = __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == pairs - 1u;
        if (last) {
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
        s_last = last;
    }
    __syncthreads();
    if (d_pred_unit) {                                    // ragged_loss_bwd_kernel's expressions for gloss = NULL (g = 1)
        const float nn = s_norm[0], dn = s_norm[1];
        for (int l = threadIdx.x; l < n; l += 256) {
            const long e = base + (long)l * nch;
            const float d = pred[e] - tru[e];
            float dnorm;
            if (p == 1) dnorm = (d > 0.0f) ? 1.0f : (d < 0.0f ? -1.0f : 0.0f);
            else if (p == 2) dnorm = (nn > 0.0f) ? d / nn : 0.0f;
            else dnorm = (nn > 0.0f) ? copysignf(powf(fabsf(d) / nn, (float)(p - 1)), d) : 0.0f;
            d_pred_unit[e] = 1.0f * dnorm / (dn * nch);
        }
        for (int l = n + threadIdx.x; l < npts; l += 256) d_pred_unit[base + (long)l * nch] = 0.0f;       // padded points: exact zeros
    }
    if (s_last && threadIdx.x < 64) {                     // loss = sum_s mean_c nn / dn, ragged_loss_sum_kernel's order
        const int pairs = gridDim.x * gridDim.y;
        double v = 0.0;
        for (int i = threadIdx.x; i < pairs; i += 64) {
            const float a = __hip_atomic_load(norms + 2 * i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            const float b = __hip_atomic_load(norms + 2 * i + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            v += (double)a / (double)b / nch;
        }
        v = wave_sum_d(v);
        if (threadIdx.x == 0) {
            *loss = (float)v;
            __hip_atomic_store(ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);       // left zero for the next call
        }
    }
}

// ONE workgroup of 16 waves: wave w takes the pairs w, w + 16, ... in ascending order - a pair's maxima over its first len[s]
// points with 64 lanes (max is exact in any order; NaN in a real point propagates, as torch.max does), its ratio / nch added to the
// wave's fp64 sum - and the 16 wave sums are added in wave order: an order that depends on (batch, nch) only, nothing stored between
__global__ __launch_bounds__(1024) void ragged_max_kernel(const float* __restrict__ tru, const float* __restrict__ pred,
                                                          const int* __restrict__ len, int batch, int npts, int nch,
                                                          float* __restrict__ out) {
    __shared__ double s_sum[16];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int pairs = batch * nch;
    double acc = 0.0;
    for (int pair = wave; pair < pairs; pair += 16) {
        const int s = pair / nch, c = pair - s * nch;
        const int n = clamp_len(len, s, npts);
        const long base = (long)s * npts * nch + c;
        float num = 0.0f, den = 0.0f;
        bool bad = false;
        for (int l = lane; l < n; l += 64) {
            const long e = base + (long)l * nch;
            const float t = tru[e], d = fabsf(t - pred[e]);
            bad |= (d != d) || (t != t);
            num = fmaxf(num, d);
            den = fmaxf(den, fabsf(t));
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            num = fmaxf(num, __shfl_xor(num, o, 64));
            den = fmaxf(den, __shfl_xor(den, o, 64));
        }
        float r = num / den;                              // fp32 division as in the reference (0/0 -> NaN, x/0 -> inf)
        if (__builtin_amdgcn_ballot_w64(bad)) r = __builtin_nanf("");
        acc += (double)r / nch;
    }
    if (lane == 0) s_sum[wave] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        double total = 0.0;
        for (int w = 0; w < 16; ++w) total += s_sum[w];
        *out = (float)total;
    }
}

}  // namespace

extern "C" int pit_rel_lp_loss_ragged_fwd_grad(const float* tru, const float* pred, const int* len, int batch, int npts, int nch, int p,
                                               float* norms, float* loss, unsigned* workspace, float* d_pred_unit, float* clear_buf,
                                               long clear_n, void* stream) {
    if (!tru || !pred || !len || !norms || !loss || !workspace) return PIT_ERR_NULL;
    if (batch <= 0 || batch > 65535 || npts <= 0 || nch <= 0 || p < 1 || clear_n < 0 || (clear_n > 0 && !clear_buf)) return PIT_ERR_SIZE;
    // planes of clear-only workgroups: about 16 K floats (sixteen 16-byte stores per thread) per workgroup, at most 512 workgroups
    const long pairs = (long)batch * nch;
    const long want = std::min<long>((clear_n + 16383) / 16384, 512L);
    const unsigned planes = (unsigned)std::max<long>(1L, std::min<long>((want + pairs - 1) / pairs, 64L));
    hipLaunchKernelGGL(ragged_loss_step_kernel, dim3((unsigned)nch, (unsigned)batch, planes), dim3(256), 0, (hipStream_t)stream, tru, pred, len,
                       npts, nch, p, norms, loss, workspace, d_pred_unit, clear_n > 0 ? clear_buf : nullptr, clear_n);
    PIT_CHECK_LAUNCH();
    return 0;
}

extern "C" int pit_rel_max_norm_ragged(const float* tru, const float* pred, const int* len, int batch, int npts, int nch, float* out,
                                       void* stream) {
    if (!tru || !pred || !len || !out) return PIT_ERR_NULL;
    if (batch <= 0 || batch > 65535 || npts <= 0 || nch <= 0) return PIT_ERR_SIZE;
    hipLaunchKernelGGL(ragged_max_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, tru, pred, len, batch, npts, nch, out);
    PIT_CHECK_LAUNCH();
    return 0;
}
