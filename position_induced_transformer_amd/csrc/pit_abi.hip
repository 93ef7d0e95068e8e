// Version / error text / layout probe of the C ABI (include/pit_hip.h).
#include "pit_common.h"

namespace {
// D(32x32) = A(32x8) * B(8x32) with the fragment maps documented in pit_common.h.
__global__ void mfma_probe_kernel(const float* a, const float* b, float* d) {
    const int lane = threadIdx.x & 63, half = lane >> 5, l31 = lane & 31;
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.0f;
#pragma unroll
    for (int k = 0; k < 8; k += 2) acc = mfma_32x32x2(a[l31 * 8 + k + half], b[(k + half) * 32 + l31], acc);
#pragma unroll
    for (int r = 0; r < 16; ++r) d[acc_row(r, half) * 32 + l31] = acc[r];
}
}  // namespace

thread_local int t_call_math = PIT_MATH_FP32;

extern "C" int pit_version(void) { return PIT_ABI_VERSION; }

namespace {
thread_local int t_rider_counts[PIT_RIDER_KINDS];
thread_local int t_gemm_counts[PIT_GEMM_KINDS];
thread_local int t_att_counts[PIT_ATT_KINDS];
thread_local int t_dense_counts[PIT_DENSE_KINDS];
thread_local int t_rider_mute = 0;
}  // namespace

void pit_rider_note(int kind) {
    if (!t_rider_mute && kind >= 0 && kind < PIT_RIDER_KINDS) ++t_rider_counts[kind];
}
void pit_rider_mute(int on) { t_rider_mute = on; }

extern "C" int pit_debug_rider_counts(int* out, int n, int reset) {
    for (int k = 0; out && k < n && k < PIT_RIDER_KINDS; ++k) out[k] = t_rider_counts[k];
    if (reset)
        for (int k = 0; k < PIT_RIDER_KINDS; ++k) t_rider_counts[k] = 0;
    return PIT_RIDER_KINDS;
}

void pit_gemm_note(int kind) {
    if (kind >= 0 && kind < PIT_GEMM_LAST_FWD16) ++t_gemm_counts[kind];
}
void pit_gemm_note_last(int slot, int value) {
    if (slot >= PIT_GEMM_LAST_FWD16 && slot < PIT_GEMM_KINDS) t_gemm_counts[slot] = value;
}

extern "C" int pit_debug_gemm_counts(int* out, int n, int reset) {
    for (int k = 0; out && k < n && k < PIT_GEMM_KINDS; ++k) out[k] = t_gemm_counts[k];
    if (reset)
        for (int k = 0; k < PIT_GEMM_KINDS; ++k) t_gemm_counts[k] = 0;
    return PIT_GEMM_KINDS;
}

void pit_att_note(int kind) {
    if (kind >= 0 && kind < PIT_ATT_LAST_ROWS) ++t_att_counts[kind];
}
void pit_att_note_last(int slot, int value) {
    if (slot >= PIT_ATT_LAST_ROWS && slot < PIT_ATT_KINDS) t_att_counts[slot] = value;
}

extern "C" int pit_debug_att_counts(int* out, int n, int reset) {
    for (int k = 0; out && k < n && k < PIT_ATT_KINDS; ++k) out[k] = t_att_counts[k];
    if (reset)
        for (int k = 0; k < PIT_ATT_KINDS; ++k) t_att_counts[k] = 0;
    return PIT_ATT_KINDS;
}

void pit_dense_note(int kind) {
    if (kind >= 0 && kind < PIT_DENSE_LAST_ROWS) ++t_dense_counts[kind];
}
void pit_dense_note_last(int slot, int value) {
    if (slot >= PIT_DENSE_LAST_ROWS && slot < PIT_DENSE_KINDS) t_dense_counts[slot] = value;
}

extern "C" int pit_debug_dense_counts(int* out, int n, int reset) {
    for (int k = 0; out && k < n && k < PIT_DENSE_KINDS; ++k) out[k] = t_dense_counts[k];
    if (reset)
        for (int k = 0; k < PIT_DENSE_KINDS; ++k) t_dense_counts[k] = 0;
    return PIT_DENSE_KINDS;
}

extern "C" const char* pit_error_string(int code) {
    switch (code) {
        case 0: return "ok";
        case PIT_ERR_NULL: return "pit: required pointer is NULL";
        case PIT_ERR_SIZE: return "pit: invalid size / stride argument";
        case PIT_ERR_METRIC: return "pit: unknown metric";
        case PIT_ERR_UNSUPPORTED: return "pit: unsupported configuration";
        default: return code > 0 ? hipGetErrorString((hipError_t)code) : "pit: unknown error";
    }
}

extern "C" int pit_debug_mfma_tile(const float* a, const float* b, float* d, void* stream) {
    if (!a || !b || !d) return PIT_ERR_NULL;
    hipLaunchKernelGGL(mfma_probe_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, a, b, d);
    PIT_CHECK_LAUNCH();
    return 0;
}
