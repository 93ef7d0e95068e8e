// Evaluation metrics of a whole pass on the device (include/pit_hip.h, pit_eval_metrics): per launch, for every valid sample
// and channel over the sample's real points,
//   ||true - pred'||_p / ||true||_p   and   max|true - pred'| / max|true|,     pred' = pred*scale + shift (two fp32 roundings),
// their means over the channels per sample (utils.py:59-98), and the pass totals kept in eight doubles that survive from launch
// to launch: the loops of train_darcy.py:136-144 / train_vorticity.py:131-141 without their .item() per batch.
//
// One workgroup per (sample, channel, part); how many parts a series is split into depends on (batch, npts, nch) only
// (eval_parts), lengths and n_valid only switch work off.  A workgroup leaves its four partial results (two fp64 sums, two
// maxima) in its own slot of the workspace and takes an arrival ticket; the workgroup of the last ticket combines the parts in
// part order, the channels in channel order, writes the per-sample table and adds the samples in index order.  Same inputs and
// state, same bits.
#include "pit_common.h"

namespace {

constexpr int EVAL_T = 256;             // threads per workgroup
constexpr int EVAL_MAX_PARTS = 64;      // PIT_EVAL_MAX_PARTS
constexpr int EVAL_MIN_CHUNK = 1024;    // a part keeps at least this many points (4 per thread)
constexpr int EVAL_FILL = 512;          // workgroups that occupy the chip (two per CU); no further split beyond

// parts per (sample, channel) series: 1, 2, 4, ..., 64 - the dispatch instances (PIT_EVAL_PARTS_* of the tests)
int eval_parts(int batch, int npts, int nch) {
    int parts = 1;
    while (parts < EVAL_MAX_PARTS && (long)batch * nch * parts < EVAL_FILL && npts / (2 * parts) >= EVAL_MIN_CHUNK) parts *= 2;
    return parts;
}

constexpr int EVAL_SLOT = 4;            // doubles per (sample, channel, part): {sum |t-q|^p, sum |t|^p, max|t-q|, max|t|}
constexpr long EVAL_HEAD_BYTES = 16;    // the ticket word, padded

__device__ __forceinline__ float pow_abs_e(float x, int p) {
    const float ax = fabsf(x);
    if (p == 1) return ax;
    if (p == 2) return ax * ax;
    return powf(ax, (float)p);
}
// torch.max propagates NaN
__device__ __forceinline__ double nan_max(double a, double b) { return (a != a || b != b) ? __builtin_nan("") : fmax(a, b); }
__device__ __forceinline__ double root_p(double v, int p) { return p == 1 ? v : (p == 2 ? sqrt(v) : pow(v, 1.0 / p)); }

__device__ __forceinline__ void slot_store(double* q, double v) { __hip_atomic_store(q, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ double slot_load(const double* q) {
    return __hip_atomic_load(const_cast<double*>(q), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// lane k's value, to every lane (k wave-uniform)
__device__ __forceinline__ double lane_get(double v, int k) {
    const long long b = __double_as_longlong(v);
    const int lo = __builtin_amdgcn_readlane((int)b, k), hi = __builtin_amdgcn_readlane((int)(b >> 32), k);
    return __longlong_as_double(((long long)hi << 32) | (unsigned int)lo);
}

__global__ __launch_bounds__(EVAL_T) void eval_metrics_kernel(const float* __restrict__ tru, const float* __restrict__ pred,
                                                              const float* __restrict__ scale, const float* __restrict__ shift,
                                                              const int* __restrict__ len, const int* __restrict__ n_valid,
                                                              int batch, int npts, int nch, int p, int parts, double* state,
                                                              float* per_sample, long ps_stride, float* pred_store,
                                                              long store_stride, long capacity, int advance, int store_true,
                                                              unsigned* ticket,
                                                              double* slots) {
    __shared__ double s_num[EVAL_T / 64], s_den[EVAL_T / 64];
    __shared__ float s_mnum[EVAL_T / 64], s_mden[EVAL_T / 64];
    __shared__ double s_lp[EVAL_T], s_mx[EVAL_T];
    __shared__ int s_last;
    const int tid = threadIdx.x;
    const int c = blockIdx.x % nch, part = blockIdx.x / nch, s = blockIdx.y;
    const int nv = n_valid ? min(max(*n_valid, 0), batch) : batch;
    // the cursor: read by EVERY workgroup before its ticket (the fence below), rewritten by the last arriver alone
    const double cursor = state[4];
    // (a cursor no pass can have produced writes no row at all)
    const long row0 = (cursor >= 0.0 && cursor < 9.0e15) ? (long)cursor : capacity;
    const bool live = s < nv;
    const int chunk = (npts + parts - 1) / parts;
    const int lbeg = min(npts, part * chunk), lend = min(npts, lbeg + chunk);
    double num = 0.0, den = 0.0;
    float mnum = 0.0f, mden = 0.0f;
    bool bad = false;
    if (live) {
        const int n = len ? min(max(len[s], 0), npts) : npts;          // the sample's real points
        const int rend = min(lend, n);
        const long row = row0 + s;
        float* store = (pred_store && row < capacity) ? pred_store + row * store_stride + c : nullptr;
        const long base = (long)s * npts * nch + c;
        for (int l0 = lbeg + tid; l0 < rend; l0 += 4 * EVAL_T) {       // 4 points per thread in flight
            float qv[4], tv[4], sc[4], sh[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int l = l0 + u * EVAL_T;
                const bool ok = l < rend;
                const long e = base + (long)(ok ? l : lbeg) * nch;
                qv[u] = ok ? pred[e] : 0.0f;
                tv[u] = ok ? tru[e] : 0.0f;
                sc[u] = (scale && ok) ? scale[(long)l * nch + c] : 1.0f;
                sh[u] = (scale && ok) ? shift[(long)l * nch + c] : 0.0f;
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int l = l0 + u * EVAL_T;
                if (l >= rend) continue;
                const float q = scale ? __fadd_rn(__fmul_rn(qv[u], sc[u]), sh[u]) : qv[u];
                const float t = tv[u], d = t - q;
                bad |= (d != d) || (t != t);
                num += (double)pow_abs_e(d, p);
                den += (double)pow_abs_e(t, p);
                mnum = fmaxf(mnum, fabsf(d));
                mden = fmaxf(mden, fabsf(t));
                if (store) store[(long)l * nch] = store_true ? t : q;
            }
        }
        if (store)                                                     // padded points of a stored row: zeros, nothing read
            for (int l = max(lbeg, n) + tid; l < lend; l += EVAL_T) store[(long)l * nch] = 0.0f;
    }
    num = wave_sum_d(num);
    den = wave_sum_d(den);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        mnum = fmaxf(mnum, __shfl_xor(mnum, o, 64));
        mden = fmaxf(mden, __shfl_xor(mden, o, 64));
    }
    const int any_bad = __syncthreads_or(bad ? 1 : 0);
    if ((tid & 63) == 0) { s_num[tid >> 6] = num; s_den[tid >> 6] = den; s_mnum[tid >> 6] = mnum; s_mden[tid >> 6] = mden; }
    __syncthreads();
    const unsigned total = gridDim.x * gridDim.y;
    if (tid == 0) {
        if (live) {
            num = ((s_num[0] + s_num[1]) + s_num[2]) + s_num[3];
            den = ((s_den[0] + s_den[1]) + s_den[2]) + s_den[3];
            double dn = (double)fmaxf(fmaxf(s_mnum[0], s_mnum[1]), fmaxf(s_mnum[2], s_mnum[3]));
            double dd = (double)fmaxf(fmaxf(s_mden[0], s_mden[1]), fmaxf(s_mden[2], s_mden[3]));
            if (any_bad) dn = dd = __builtin_nan("");
            double* slot = slots + (((long)s * nch + c) * parts + part) * EVAL_SLOT;
            slot_store(slot + 0, num); slot_store(slot + 1, den); slot_store(slot + 2, dn); slot_store(slot + 3, dd);
        }
        __threadfence();                                               // slot and cursor read: performed before the ticket
        s_last = (atomicAdd(ticket, 1u) == total - 1u) ? 1 : 0;
    }
    __syncthreads();
    if (!s_last) return;
    __threadfence();
    // ---- the last arriver: every live workgroup's slot is in
    double tot_lp = 0.0, tot_mx = 0.0, worst_lp = 0.0, worst_mx = 0.0;
    if (tid == 0) { worst_lp = state[2]; worst_mx = state[3]; }
    for (int first = 0; first < nv; first += EVAL_T) {
        if (parts == 1) {                                              // a thread per sample
            const int smp = first + tid;
            if (smp < nv) {
                double lp = 0.0, mx = 0.0;
                for (int ch = 0; ch < nch; ++ch) {
                    const double* slot = slots + ((long)smp * nch + ch) * EVAL_SLOT;
                    lp += root_p(slot_load(slot + 0), p) / root_p(slot_load(slot + 1), p);
                    mx += slot_load(slot + 2) / slot_load(slot + 3);
                }
                lp /= nch; mx /= nch;
                s_lp[tid] = lp; s_mx[tid] = mx;
                const long row = row0 + smp;
                if (per_sample && row < capacity) {
                    per_sample[row * ps_stride + 0] = (float)lp;
                    per_sample[row * ps_stride + 1] = (float)mx;
                }
            }
        } else {
            // a wavefront per sample: lane k fetches part k's slot (parts <= 64, one coalesced fetch per value instead of a chain
            // of round trips), then every lane adds the parts in part order
            const int lane = tid & 63, last = min(nv, first + EVAL_T);
            for (int smp = first + (tid >> 6); smp < last; smp += EVAL_T / 64) {
                double lp = 0.0, mx = 0.0;
                for (int ch = 0; ch < nch; ++ch) {
                    const double* slot = slots + (((long)smp * nch + ch) * parts + min(lane, parts - 1)) * EVAL_SLOT;
                    const double va = slot_load(slot + 0), vb = slot_load(slot + 1), vma = slot_load(slot + 2), vmb = slot_load(slot + 3);
                    double a = 0.0, b = 0.0, ma = 0.0, mb = 0.0;
                    for (int k = 0; k < parts; ++k) {
                        a += lane_get(va, k);
                        b += lane_get(vb, k);
                        ma = nan_max(ma, lane_get(vma, k));
                        mb = nan_max(mb, lane_get(vmb, k));
                    }
                    lp += root_p(a, p) / root_p(b, p);
                    mx += ma / mb;
                }
                lp /= nch; mx /= nch;
                const long row = row0 + smp;
                if (lane == 0) {
                    s_lp[smp - first] = lp; s_mx[smp - first] = mx;
                    if (per_sample && row < capacity) {
                        per_sample[row * ps_stride + 0] = (float)lp;
                        per_sample[row * ps_stride + 1] = (float)mx;
                    }
                }
            }
        }
        __syncthreads();
        if (tid == 0) {
            const int cnt = min(EVAL_T, nv - first);
            for (int i = 0; i < cnt; ++i) {                            // the samples in index order
                tot_lp += s_lp[i]; tot_mx += s_mx[i];
                worst_lp = nan_max(worst_lp, s_lp[i]); worst_mx = nan_max(worst_mx, s_mx[i]);
            }
        }
        __syncthreads();
    }
    if (tid == 0) {
        state[0] += tot_lp;
        state[1] += tot_mx;
        state[2] = worst_lp;
        state[3] = worst_mx;
        if (advance) state[4] = cursor + (double)nv;
        state[5] += 1.0;
        atomicExch(ticket, 0u);
    }
}

}  // namespace

extern "C" long pit_eval_metrics_workspace(int batch, int npts, int nch) {
    if (batch <= 0 || npts <= 0 || nch <= 0) return PIT_ERR_SIZE;
    return EVAL_HEAD_BYTES + (long)batch * nch * eval_parts(batch, npts, nch) * EVAL_SLOT * (long)sizeof(double);
}

extern "C" int pit_eval_metrics(const float* tru, const float* pred, const float* pred_scale, const float* pred_shift,
                                const int* len, const int* n_valid, int batch, int npts, int nch, int p, double* state,
                                float* per_sample, long ps_stride, float* pred_store, long store_stride, long capacity,
                                int advance, void* workspace, void* stream) {
    if (!tru || !pred || !state || !workspace) return PIT_ERR_NULL;
    if ((pred_scale == nullptr) != (pred_shift == nullptr)) return PIT_ERR_NULL;
    if (batch <= 0 || npts <= 0 || nch <= 0 || p < 1 || batch > 65535 || capacity < 0) return PIT_ERR_SIZE;
    if (advance & ~(PIT_EVAL_ADVANCE | PIT_EVAL_STORE_TRUE)) return PIT_ERR_SIZE;
    if (per_sample && (capacity == 0 || ps_stride < 2)) return PIT_ERR_SIZE;
    if (pred_store && (capacity == 0 || store_stride < (long)npts * nch)) return PIT_ERR_SIZE;
    const int parts = eval_parts(batch, npts, nch);
    if ((long)nch * parts > 0x7fffffffL) return PIT_ERR_SIZE;
    unsigned* ticket = reinterpret_cast<unsigned*>(workspace);
    double* slots = reinterpret_cast<double*>(reinterpret_cast<char*>(workspace) + EVAL_HEAD_BYTES);
    hipLaunchKernelGGL(eval_metrics_kernel, dim3(nch * parts, batch), dim3(EVAL_T), 0, (hipStream_t)stream, tru, pred, pred_scale,
                       pred_shift, len, n_valid, batch, npts, nch, p, parts, state, per_sample, ps_stride, pred_store,
                       store_stride, capacity, (advance & PIT_EVAL_ADVANCE) ? 1 : 0, (advance & PIT_EVAL_STORE_TRUE) ? 1 : 0, ticket,
                       slots);
    PIT_CHECK_LAUNCH();
    return 0;
}
