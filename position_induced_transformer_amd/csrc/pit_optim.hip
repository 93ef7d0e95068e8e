// Fused Adam step over the flat parameter / gradient buffers with the cosine-annealed learning
// rate of the reference loops (torch.optim.Adam(lr=1e-3) + CosineAnnealingLR(T_max=iterations),
// train_darcy.py:115-116,131-134), sync-free: the step counter lives on the device so the launch
// can be replayed from a hipGraph.
#include "pit_common.h"

namespace {

// One launch: every thread derives the step's learning rate and bias corrections from the device
// step counter (read before any workgroup can have advanced it: the LAST workgroup to finish -
// arrival ticket in scalars[3] - writes the new count and clears the ticket), updates its
// elements and, with zero_grads, clears the gradient it consumed (the next step's backward
// accumulates into zeros without a separate memset).
// scalars[0..2] = lr_t, 1 - beta1^t, 1 - beta2^t of the step just taken (for inspection); [3] = ticket
__global__ __launch_bounds__(256) void adam_step_kernel(float* __restrict__ p, float* __restrict__ g, float* __restrict__ m,
                                                        float* __restrict__ v, long n, long long* step, float lr0,
                                                        float eta_min, int t_max, float beta1, float beta2, float eps,
                                                        float weight_decay, int zero_grads, float* scalars) {
    __shared__ float s_sc[3];
    const long long t = *step + 1;
    if (threadIdx.x == 0) {                    // fp64 cos / pow once per workgroup, not per thread
        // CosineAnnealingLR closed form: the rate used by the t-th optimizer.step() is that of epoch t-1
        float lr_t = lr0;
        if (t_max > 0) {
            const double ph = 3.14159265358979323846 * (double)(t - 1) / (double)t_max;
            lr_t = (float)((double)eta_min + 0.5 * ((double)lr0 - (double)eta_min) * (1.0 + cos(ph)));
        }
        s_sc[0] = lr_t;
        s_sc[1] = (float)(1.0 - pow((double)beta1, (double)t));
        s_sc[2] = (float)(1.0 - pow((double)beta2, (double)t));
    }
    __syncthreads();
    const float lr = s_sc[0], bc1 = s_sc[1], bc2 = s_sc[2];
    const float step_size = lr / bc1;
    const float inv_sqrt_bc2 = 1.0f / sqrtf(bc2);
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
        float gi = g[i];
        if (zero_grads) g[i] = 0.0f;
        if (weight_decay != 0.0f) gi += weight_decay * p[i];
        const float mi = beta1 * m[i] + (1.0f - beta1) * gi;
        const float vi = beta2 * v[i] + (1.0f - beta2) * gi * gi;
        m[i] = mi;
        v[i] = vi;
        const float denom = sqrtf(vi) * inv_sqrt_bc2 + eps;       // torch: (sqrt(v)/sqrt(bc2)) + eps
        p[i] -= step_size * (mi / denom);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned* ticket = reinterpret_cast<unsigned*>(scalars + 3);
        if (atomicAdd(ticket, 1u) == gridDim.x - 1u) {            // every workgroup has read *step by now
            *step = t;
            scalars[0] = lr; scalars[1] = bc1; scalars[2] = bc2;
            atomicExch(ticket, 0u);
        }
    }
}

// ---- the guarded step (include/pit_hip.h, pit_adam_step_guarded): two launches --------------------------------------------------
constexpr int GUARD_T = 256;            // threads of both kernels
static_assert(GUARD_T >= PIT_GUARD_MAX_PARTS, "one thread stages one partial");
constexpr long GUARD_UNIT = 1024;       // a run is a whole number of these: one 16-byte group per thread

__host__ __device__ inline long guard_run(long n) {
    return GUARD_UNIT * ((n + GUARD_UNIT * PIT_GUARD_MAX_PARTS - 1) / (GUARD_UNIT * PIT_GUARD_MAX_PARTS));
}

// Launch 1: partials[b] = sum of g[i]^2 over run b, in fp64 (a square of an fp32 value is exact there and cannot overflow).
// Thread t owns the groups of four consecutive elements number t, t + 256, ... of its workgroup's run and adds them in that
// order, element by element; the wave sums run over the DPP lanes and thread 0 adds the four waves in order: the partition
// and every order of addition depend on n alone, so do the bits.  A group is one 16-byte load when the base is 16-byte
// aligned (run starts are multiples of 1024 elements) and the group ends inside the buffer, four guarded dwords otherwise -
// the same elements in the same places either way.
__global__ __launch_bounds__(GUARD_T) void grad_sumsq_kernel(const float* __restrict__ g, long n, long run, int vec,
                                                             double* __restrict__ partials) {
    __shared__ double s_w[GUARD_T / PIT_WAVE];
    const int tid = threadIdx.x;
    const long a = (long)blockIdx.x * run, b = min(n, a + run);
    double acc = 0.0;
    for (long e = a + 4L * tid; e < b; e += 4L * GUARD_T) {
        float x[4];
        if (vec && e + 4 <= b) {
            const float4 q = *reinterpret_cast<const float4*>(g + e);
            x[0] = q.x; x[1] = q.y; x[2] = q.z; x[3] = q.w;
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) x[j] = e + j < b ? g[e + j] : 0.0f;
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const double d = (double)x[j];
            acc += d * d;
        }
    }
    const double w = wave_sum_d(acc);
    if ((tid & (PIT_WAVE - 1)) == 0) s_w[tid / PIT_WAVE] = w;
    __syncthreads();
    if (tid == 0) partials[blockIdx.x] = ((s_w[0] + s_w[1]) + s_w[2]) + s_w[3];
}

// Launch 2: every workgroup adds the partials in index order (identical bits everywhere), decides from the norm alone and
// either runs adam_step_kernel's arithmetic on g * coef or leaves parameters and moments alone.  Both counters - calls
// (the schedule's position) and step (the applied updates behind the bias corrections) - are read by every workgroup
// before its ticket; the workgroup of the last ticket writes them back together with the statistics.
//
// Two instances.  adam_step_guarded_kernel<> (no trailing argument) is the guarded step.  adam_step_guarded_kernel<avg_args>
// (include/pit_hip.h, pit_adam_step_averaged) also keeps an average of the parameters: its weight is one more value thread 0
// forms in fp64, the average one more buffer read and written per element from the parameter still in its register, and
// *n_averaged one more counter of the last ticket.  Everything the trailing argument adds is compiled out of the first
// instance, whose argument list and instructions are those of the kernel before the second existed.
struct avg_args {
    float* average;
    long long* n_averaged;
    int mode;
    double decay;
    int ramp;
    long long start;
};
__device__ inline avg_args avg_of() { return avg_args{}; }
__device__ inline avg_args avg_of(const avg_args& a) { return a; }

template <typename... Avg>
__global__ __launch_bounds__(GUARD_T) void adam_step_guarded_kernel(
        float* __restrict__ p, float* __restrict__ g, float* __restrict__ m, float* __restrict__ v, long n, long long* step,
        long long* calls, float lr0, float eta_min, int t_max, int warmup_steps, double warmup_start, float beta1, float beta2,
        float eps, float weight_decay, int decoupled, double max_norm, int zero_grads, const float* loss,
        const double* __restrict__ partials, int parts, double* state, float* scalars, Avg... avg_pack) {
    constexpr bool AVG = sizeof...(Avg) == 1;
    static_assert(sizeof...(Avg) <= 1, "no trailing argument, or one avg_args");
    [[maybe_unused]] const avg_args avg = avg_of(avg_pack...);
    __shared__ double s_part[PIT_GUARD_MAX_PARTS];
    __shared__ double s_norm;
    __shared__ float s_sc[AVG ? 6 : 5];
    __shared__ int s_skip;
    const int tid = threadIdx.x;
    const long long t = __hip_atomic_load(step, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) + 1;      // this update, if applied
    const long long k = __hip_atomic_load(calls, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) + 1;     // this call
    if (tid < parts) s_part[tid] = partials[tid];
    __syncthreads();
    if (tid == 0) {
        double sum = 0.0;
        // index order (reading by eights with the loads in flight gained nothing: DESIGN section 20)
        for (int i = 0; i < parts; ++i) sum += s_part[i];
        const double norm = sqrt(sum);
        const bool finite = norm <= 1.79769313486231570815e308;        // false for NaN and +inf
        float coef = 1.0f;
        if (finite && max_norm > 0.0) coef = (float)fmin(1.0, max_norm / (norm + 1e-6));       // clip_grad_norm_
        float lr_t = lr0;
        if (k <= (long long)warmup_steps) {
            lr_t = (float)((double)lr0 * (warmup_start + (1.0 - warmup_start) * (double)(k - 1) / (double)warmup_steps));
        } else if (t_max > 0) {
            // adam_step_kernel's expression on the calls after the warm-up (warmup_steps = 0: the same bits)
            const double ph = 3.14159265358979323846 * (double)(k - 1 - warmup_steps) / (double)t_max;
            lr_t = (float)((double)eta_min + 0.5 * ((double)lr0 - (double)eta_min) * (1.0 + cos(ph)));
        }
        s_sc[0] = lr_t;
        s_sc[1] = (float)(1.0 - pow((double)beta1, (double)t));
        s_sc[2] = (float)(1.0 - pow((double)beta2, (double)t));
        s_sc[3] = coef;
        s_sc[4] = (float)(1.0 - (double)lr_t * (double)weight_decay);  // AdamW: p *= 1 - lr_t * wd
        s_norm = norm;
        s_skip = finite ? 0 : 1;
        if constexpr (AVG) {
            float w = 1.0f;             // t <= start: the average follows the weights
            if (t > avg.start) {
                const double mm = (double)(t - avg.start);
                if (avg.mode == 0) {
                    const double d = avg.ramp ? fmin(avg.decay, (1.0 + mm) / (10.0 + mm)) : avg.decay;
                    w = (float)(1.0 - d);
                } else {
                    w = (float)(1.0 / mm);
                }
            }
            s_sc[5] = w;
        }
    }
    __syncthreads();
    const float lr = s_sc[0], bc1 = s_sc[1], bc2 = s_sc[2], coef = s_sc[3], shrink = s_sc[4];
    const bool skip = s_skip != 0;
    const float step_size = lr / bc1;
    const float inv_sqrt_bc2 = 1.0f / sqrtf(bc2);
    const float wd_coupled = decoupled ? 0.0f : weight_decay;
    const bool shrinks = decoupled && weight_decay != 0.0f;
    float w_avg = 1.0f;
    if constexpr (AVG) w_avg = s_sc[5];
    if (skip) {
        if (zero_grads)                 // (the non-finite values would live on in the accumulator)
            for (long i = (long)blockIdx.x * blockDim.x + tid; i < n; i += (long)gridDim.x * blockDim.x) g[i] = 0.0f;
    } else {
        for (long i = (long)blockIdx.x * blockDim.x + tid; i < n; i += (long)gridDim.x * blockDim.x) {
            float gi = g[i];
            if (zero_grads) g[i] = 0.0f;
            gi *= coef;                 // (x * 1.0f is x: an inert guard has adam_step_kernel's bits; the build contracts nothing)
            float pi = p[i];
            if (shrinks) pi *= shrink;
            if (wd_coupled != 0.0f) gi += wd_coupled * pi;
            const float mi = beta1 * m[i] + (1.0f - beta1) * gi;
            const float vi = beta2 * v[i] + (1.0f - beta2) * gi * gi;
            m[i] = mi;
            v[i] = vi;
            const float denom = sqrtf(vi) * inv_sqrt_bc2 + eps;       // torch: (sqrt(v)/sqrt(bc2)) + eps
            pi -= step_size * (mi / denom);
            p[i] = pi;
            if constexpr (AVG) {
                if (w_avg == 1.0f) {
                    avg.average[i] = pi;
                } else {
                    const float a = avg.average[i];
                    avg.average[i] = a + w_avg * (pi - a);              // (three roundings: the build contracts nothing)
                }
            }
        }
    }
    __syncthreads();
    if (tid == 0) {
        unsigned* ticket = reinterpret_cast<unsigned*>(scalars + 3);
        if (atomicAdd(ticket, 1u) == gridDim.x - 1u) {                // every workgroup has read both counters by now
            const double norm = s_norm;
            __hip_atomic_store(calls, k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            scalars[0] = lr;
            state[PIT_GUARD_CALLS] += 1.0;
            state[PIT_GUARD_LAST_NORM] = norm;
            state[PIT_GUARD_LAST_COEF] = (double)coef;
            if (skip) {
                state[PIT_GUARD_SKIPPED] += 1.0;
            } else {
                __hip_atomic_store(step, t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                scalars[1] = bc1; scalars[2] = bc2;
                state[PIT_GUARD_APPLIED] += 1.0;
                if (coef < 1.0f) state[PIT_GUARD_CLIPPED] += 1.0;
                if (norm > state[PIT_GUARD_MAX_NORM]) state[PIT_GUARD_MAX_NORM] = norm;
                if constexpr (AVG) {
                    if (t > avg.start) *avg.n_averaged = t - avg.start;
                }
            }
            if (loss) {
                const float l = *loss;
                if (fabsf(l) <= 3.40282346638528859812e38f) {
                    state[PIT_GUARD_LOSS_SUM] += (double)l;
                    state[PIT_GUARD_LOSS_FINITE] += 1.0;
                } else {
                    state[PIT_GUARD_LOSS_NONFINITE] += 1.0;
                }
            }
            atomicExch(ticket, 0u);
        }
    }
}

// ---- pit_exchange_words: two disjoint buffers change places, word for word ---------------------------------------------------------
// Word w of either buffer belongs to one of three runs: `head` single words, `nvec` 16-byte groups, `tail` single words; the
// host picks head so that both group bases are 16-byte aligned (equal distance from a boundary) or makes every word a head word.
// Each word is read from both sides and written to both sides by ONE thread, so no thread sees another's store.
__global__ __launch_bounds__(256) void exchange_words_kernel(unsigned* __restrict__ a, unsigned* __restrict__ b, long head,
                                                             long nvec, long tail) {
    const long first = (long)blockIdx.x * blockDim.x + threadIdx.x, stride = (long)gridDim.x * blockDim.x;
    for (long i = first; i < head; i += stride) {
        const unsigned x = a[i], y = b[i];
        a[i] = y;
        b[i] = x;
    }
    uint4* __restrict__ a4 = reinterpret_cast<uint4*>(a + head);
    uint4* __restrict__ b4 = reinterpret_cast<uint4*>(b + head);
    for (long i = first; i < nvec; i += stride) {
        const uint4 x = a4[i], y = b4[i];
        a4[i] = y;
        b4[i] = x;
    }
    const long t0 = head + 4 * nvec;
    for (long i = first; i < tail; i += stride) {
        const unsigned x = a[t0 + i], y = b[t0 + i];
        a[t0 + i] = y;
        b[t0 + i] = x;
    }
}

// [x, x + bytes) and [y, y + bytes) share a byte
inline bool ranges_overlap(const void* x, const void* y, unsigned long long bytes) {
    const uintptr_t p = (uintptr_t)x, q = (uintptr_t)y;
    return p < q ? q - p < bytes : p - q < bytes;
}

}  // namespace

extern "C" int pit_adam_guard_parts(long n) {
    if (n <= 0) return PIT_ERR_SIZE;
    const long run = guard_run(n);
    return (int)((n + run - 1) / run);
}

extern "C" int pit_adam_step_guarded(float* params, float* grads, float* exp_avg, float* exp_avg_sq, long n, long long* step,
                                     long long* calls, float lr0, float eta_min, int cosine_t_max, int warmup_steps,
                                     double warmup_start, float beta1, float beta2, float eps, float weight_decay,
                                     int decoupled, double max_norm, int zero_grads, const float* loss, double* partials,
                                     double* state, float* scalars, void* stream) {
    if (!params || !grads || !exp_avg || !exp_avg_sq || !step || !calls || !partials || !state || !scalars) return PIT_ERR_NULL;
    if (n <= 0) return PIT_ERR_SIZE;
    if (!(max_norm >= 0.0) || warmup_steps < 0 || !(warmup_start >= 0.0 && warmup_start <= 1.0)) return PIT_ERR_UNSUPPORTED;
    if ((uintptr_t)grads & 3u) return PIT_ERR_SIZE;
    const long run = guard_run(n);
    const int parts = (int)((n + run - 1) / run);
    const int vec = ((uintptr_t)grads & 15u) == 0 ? 1 : 0;
    hipLaunchKernelGGL(grad_sumsq_kernel, dim3(parts), dim3(GUARD_T), 0, (hipStream_t)stream, grads, n, run, vec, partials);
    PIT_CHECK_LAUNCH();
    const int blocks = (int)std::min<long>((n + 255) / 256, 2048L);
    hipLaunchKernelGGL(adam_step_guarded_kernel<>, dim3(blocks), dim3(GUARD_T), 0, (hipStream_t)stream, params, grads, exp_avg,
                       exp_avg_sq, n, step, calls, lr0, eta_min, cosine_t_max, warmup_steps, warmup_start, beta1, beta2, eps,
                       weight_decay, decoupled ? 1 : 0, max_norm, zero_grads, loss, partials, parts, state, scalars);
    PIT_CHECK_LAUNCH();
    return 0;
}

extern "C" int pit_adam_step_averaged(float* params, float* grads, float* exp_avg, float* exp_avg_sq, long n, long long* step,
                                      long long* calls, float lr0, float eta_min, int cosine_t_max, int warmup_steps,
                                      double warmup_start, float beta1, float beta2, float eps, float weight_decay,
                                      int decoupled, double max_norm, int zero_grads, const float* loss, double* partials,
                                      double* state, float* scalars, float* average, long long* n_averaged, int avg_mode,
                                      double avg_decay, int avg_ramp, long long avg_start, void* stream) {
    if (!params || !grads || !exp_avg || !exp_avg_sq || !step || !calls || !partials || !state || !scalars || !average ||
        !n_averaged)
        return PIT_ERR_NULL;
    if (n <= 0) return PIT_ERR_SIZE;
    if ((uintptr_t)grads & 3u) return PIT_ERR_SIZE;
    if (!(max_norm >= 0.0) || warmup_steps < 0 || !(warmup_start >= 0.0 && warmup_start <= 1.0)) return PIT_ERR_UNSUPPORTED;
    if (avg_mode != 0 && avg_mode != 1) return PIT_ERR_UNSUPPORTED;
    if (avg_mode == 0 && !(avg_decay >= 0.0 && avg_decay < 1.0)) return PIT_ERR_UNSUPPORTED;
    if (avg_start < 0) return PIT_ERR_UNSUPPORTED;
    if (ranges_overlap(average, params, 4ull * (unsigned long long)n)) return PIT_ERR_UNSUPPORTED;
    const long run = guard_run(n);
    const int parts = (int)((n + run - 1) / run);
    const int vec = ((uintptr_t)grads & 15u) == 0 ? 1 : 0;
    hipLaunchKernelGGL(grad_sumsq_kernel, dim3(parts), dim3(GUARD_T), 0, (hipStream_t)stream, grads, n, run, vec, partials);
    PIT_CHECK_LAUNCH();
    const int blocks = (int)std::min<long>((n + 255) / 256, 2048L);
    const avg_args avg{average, n_averaged, avg_mode, avg_decay, avg_ramp ? 1 : 0, avg_start};
    hipLaunchKernelGGL(adam_step_guarded_kernel<avg_args>, dim3(blocks), dim3(GUARD_T), 0, (hipStream_t)stream, params, grads, exp_avg,
                       exp_avg_sq, n, step, calls, lr0, eta_min, cosine_t_max, warmup_steps, warmup_start, beta1, beta2, eps,
                       weight_decay, decoupled ? 1 : 0, max_norm, zero_grads, loss, partials, parts, state, scalars, avg);
    PIT_CHECK_LAUNCH();
    return 0;
}

extern "C" int pit_exchange_words(void* a, void* b, long n_words, void* stream) {
    if (!a || !b) return PIT_ERR_NULL;
    if (n_words <= 0 || ((uintptr_t)a & 3u) || ((uintptr_t)b & 3u)) return PIT_ERR_SIZE;
    if (ranges_overlap(a, b, 4ull * (unsigned long long)n_words)) return PIT_ERR_UNSUPPORTED;
    long head = n_words, nvec = 0, tail = 0;               // bases unequally far from a 16-byte boundary: single words throughout
    if ((((uintptr_t)a ^ (uintptr_t)b) & 15u) == 0) {
        head = std::min<long>(n_words, (long)(((16u - ((uintptr_t)a & 15u)) & 15u) / 4u));
        nvec = (n_words - head) / 4;
        tail = n_words - head - 4 * nvec;
    }
    const long items = std::max(std::max(head, tail), nvec);
    const int blocks = (int)std::min<long>((items + 255) / 256, 2048L);
    hipLaunchKernelGGL(exchange_words_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, static_cast<unsigned*>(a),
                       static_cast<unsigned*>(b), head, nvec, tail);
    PIT_CHECK_LAUNCH();
    return 0;
}

extern "C" int pit_adam_step(float* params, float* grads, float* exp_avg, float* exp_avg_sq, long n,
                             long long* step, float lr0, float eta_min, int cosine_t_max, float beta1, float beta2,
                             float eps, float weight_decay, int zero_grads, float* scalars, void* stream) {
    if (!params || !grads || !exp_avg || !exp_avg_sq || !step || !scalars) return PIT_ERR_NULL;
    if (n <= 0) return PIT_ERR_SIZE;
    const int blocks = (int)std::min<long>((n + 255) / 256, 2048L);
    hipLaunchKernelGGL(adam_step_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, params, grads, exp_avg,
                       exp_avg_sq, n, step, lr0, eta_min, cosine_t_max, beta1, beta2, eps, weight_decay, zero_grads,
                       scalars);
    PIT_CHECK_LAUNCH();
    return 0;
}
