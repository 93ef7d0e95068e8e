// Weight gradients of a pointwise MLP in a FIXED summation order on fp32 MFMA (the reproducible mode).
//   dW1 = dZ1^T X, db1 = colsum(dZ1), dW2 = dZ2^T H, db2 = colsum(dZ2)
// Both contractions run in ONE launch: the rows are cut into equal slabs - a pure function of (rows, n0, n1, n2), see
// ord_partition - and a workgroup contracts one slab into one 64 x 64 tile of that slab's own partial matrices, which it
// writes with plain stores.  A second launch adds the partials slab by slab in index order.  No atomics anywhere, and no
// value depends on which workgroup ran first: the same inputs give the same bits on every run.
// The main loop is the one of gemm_rr_tile (pit_gemm_rd.h): [k][i] LDS images of both operands written by coalesced 16-byte
// buffer loads, two buffers, v_mfma_f32_32x32x2_f32 with two alternating accumulators.  That helper itself is not used: its
// epilogue ADDS to memory (PIT_RR_ADD), this kernel's stores.
#include "pit_common.h"

namespace {

constexpr int OM_BK = 32;          // rows of a chunk: 2 x 32 x 64 floats per operand = 32 KiB of LDS in all
constexpr int OM_TILE = 64;

struct OrdProb {
    const float* A; long lda;      // A[r][m], m < M: the matrix whose columns become the gradient's ROWS (dZ)
    const float* B; long ldb;      // B[r][n], n < N: the layer's input (X or H)
    int M, N;
    int a_vec, b_vec;              // 16-byte loads legal: width and row stride multiples of 4 floats, base 16-byte aligned
    int tx, tiles;                 // tiles along n, tiles in all
    long off;                      // where this problem's [M*N + M] partials start inside a slab's block
};
struct OrdMfmaArgs {
    OrdProb p[2];
    int rows, slabs, slab_rows, tiles;
    float* part; long per_slab;    // [slabs][per_slab]
    float* dst[4]; long len[4];    // finishing launch: d_w1, d_b1, d_w2, d_b2 in the order of a slab's block
    int accumulate;
};

// 4 consecutive floats of row k (relative to the slab) starting at column c, zero where the row or the column is out of range:
// the predicate selects the OFFSET (an offset at the resource's size returns 0 in hardware), never a value
__device__ __forceinline__ void om_load4(__amdgpu_buffer_rsrc_t r, unsigned bytes, bool vec, bool row_ok, unsigned k, unsigned ld,
                                         int c, int width, float (&v)[4]) {
    const unsigned base = (k * ld + (unsigned)c) * 4u;
    if (vec) {
        buf_load4(r, (row_ok && c < width) ? base : bytes, v);
        return;
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = buf_load(r, (row_ok && c + e < width) ? base + 4u * e : bytes);
}

__global__ __launch_bounds__(256) void ordered_dw_mfma_kernel(OrdMfmaArgs g) {
    __shared__ __attribute__((aligned(16))) float As_[2 * OM_BK * OM_TILE], Bs_[2 * OM_BK * OM_TILE];
    constexpr int BK = OM_BK, BM = OM_TILE, BN = OM_TILE;
    constexpr int PL = BK * BM / 1024;                               // 16-byte loads per thread, operand and chunk
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int half = lane >> 5, l31 = lane & 31;
    const int slab = blockIdx.x / g.tiles;
    int t = blockIdx.x % g.tiles;
    const bool second = t >= g.p[0].tiles;
    if (second) t -= g.p[0].tiles;
    const float* A = second ? g.p[1].A : g.p[0].A;
    const float* B = second ? g.p[1].B : g.p[0].B;
    const long lda = second ? g.p[1].lda : g.p[0].lda, ldb = second ? g.p[1].ldb : g.p[0].ldb;
    const int M = second ? g.p[1].M : g.p[0].M, N = second ? g.p[1].N : g.p[0].N;
    const bool a_vec = (second ? g.p[1].a_vec : g.p[0].a_vec) != 0, b_vec = (second ? g.p[1].b_vec : g.p[0].b_vec) != 0;
    const int tx = second ? g.p[1].tx : g.p[0].tx;
    const long off = second ? g.p[1].off : g.p[0].off;
    const int bx = t % tx, by = t / tx;
    const int m0 = by * BM, n0 = bx * BN;
    const int wm = (wave & 1) * 32, wn = (wave >> 1) * 32;
    const int kbeg = slab * g.slab_rows, nk = min(g.rows, kbeg + g.slab_rows) - kbeg;      // nk >= 1 (ord_partition)
    // the descriptors cover exactly this slab's rows (the last one only as far as its last column): offsets are slab-relative
    const unsigned a_bytes = (unsigned)(((long)(nk - 1) * lda + M) * 4), b_bytes = (unsigned)(((long)(nk - 1) * ldb + N) * 4);
    const __amdgpu_buffer_rsrc_t ra = make_rsrc(A + (long)kbeg * lda, a_bytes);
    const __amdgpu_buffer_rsrc_t rb = make_rsrc(B + (long)kbeg * ldb, b_bytes);

    float sa[PL][4], sb[PL][4];
    auto gload = [&](int kc) {
#pragma unroll
        for (int p = 0; p < PL; ++p) {
            const int q = p * 256 + tid, k = kc + q / (BM / 4), c = (q % (BM / 4)) * 4;
            om_load4(ra, a_bytes, a_vec, k < nk, (unsigned)k, (unsigned)lda, m0 + c, M, sa[p]);
            om_load4(rb, b_bytes, b_vec, k < nk, (unsigned)k, (unsigned)ldb, n0 + c, N, sb[p]);
        }
    };
    auto lstore = [&](int buf) {
#pragma unroll
        for (int p = 0; p < PL; ++p) {
            *reinterpret_cast<float4*>(&As_[buf * BK * BM + (p * 256 + tid) * 4]) = make_float4(sa[p][0], sa[p][1], sa[p][2], sa[p][3]);
            *reinterpret_cast<float4*>(&Bs_[buf * BK * BN + (p * 256 + tid) * 4]) = make_float4(sb[p][0], sb[p][1], sb[p][2], sb[p][3]);
        }
    };

    // two accumulators take the even and the odd MFMA steps (no dependent MFMA chain): each sums its rows in ascending order,
    // the two are added once at the end - a fixed order
    f32x16 acc0, acc1;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc0[r] = acc1[r] = 0.0f;
    const bool want_colsum = bx == 0 && wn == 0;          // db: the column sums of A, by the waves of the first tile column
    float csum = 0.0f;
    gload(0);
    lstore(0);
    __syncthreads();
    int cur = 0;
    for (int kc = 0; kc < nk; kc += BK) {
        const bool more = kc + BK < nk;
        if (more) gload(kc + BK);
        const float* as = &As_[cur * BK * BM + half * BM + wm + l31];          // this half-wave's k of a step: 2 st + half
        const float* bs = &Bs_[cur * BK * BN + half * BN + wn + l31];
#pragma unroll
        for (int st = 0; st < BK / 2; st += 2) {
            const float a0 = as[2 * st * BM], b0 = bs[2 * st * BN];
            const float a1 = as[2 * (st + 1) * BM], b1 = bs[2 * (st + 1) * BN];
            if (want_colsum) csum = (csum + a0) + a1;
            acc0 = mfma_32x32x2(a0, b0, acc0);
            acc1 = mfma_32x32x2(a1, b1, acc1);
        }
        if (more) lstore(cur ^ 1);
        __syncthreads();
        cur ^= 1;
    }

    float* part = g.part + (long)slab * g.per_slab + off;
    if (want_colsum) {
        const float v = csum + __shfl_xor(csum, 32);       // (both halves form the same sum: a + b == b + a)
        const int row = m0 + wm + l31;
        if (half == 0 && row < M) part[(long)M * N + row] = v;
    }
    const int col = n0 + wn + l31;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int row = m0 + wm + acc_row(r, half);
        if (row < M && col < N) part[(long)row * N + col] = acc0[r] + acc1[r];
    }
}

// adds the slabs' partials in slab order and writes (accumulate: adds to) the four gradients
__global__ __launch_bounds__(256) void ordered_dw_mfma_finish_kernel(OrdMfmaArgs g) {
    for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < g.per_slab; e += (long)gridDim.x * blockDim.x) {
        float v = g.part[e];
        for (int s = 1; s < g.slabs; ++s) v += g.part[(long)s * g.per_slab + e];
        long i = e;
        float* dst = g.dst[0];
        if (i >= g.len[0]) { i -= g.len[0]; dst = g.dst[1];
            if (i >= g.len[1]) { i -= g.len[1]; dst = g.dst[2];
                if (i >= g.len[2]) { i -= g.len[2]; dst = g.dst[3]; } } }
        dst[i] = g.accumulate ? dst[i] + v : v;
    }
}

inline int om_tiles(int n) { return (n + OM_TILE - 1) / OM_TILE; }

// The partition: a pure function of the four sizes (never of the device, the environment or an address).
//   tiles     = ceil(n1/64) ceil(n0/64) + ceil(n2/64) ceil(n1/64)
//   wanted    = clamp(ceil(512 / tiles), 1, 64), at most ceil(rows / 64)        (a few hundred workgroups, slabs of >= 64 rows)
//   slab_rows = ceil(rows / wanted) rounded up to a multiple of 32              (only the last slab has a partial chunk)
//   slabs     = ceil(rows / slab_rows)                                          (no empty slab)
void ord_partition(int rows, int n0, int n1, int n2, int* slabs, int* slab_rows) {
    const long tiles = (long)om_tiles(n1) * om_tiles(n0) + (long)om_tiles(n2) * om_tiles(n1);
    long want = std::min<long>(64, (512 + tiles - 1) / tiles);
    want = std::max<long>(1, std::min<long>(want, (rows + 63) / 64));
    long sr = (rows + want - 1) / want;
    sr = (sr + OM_BK - 1) / OM_BK * OM_BK;
    *slab_rows = (int)sr;
    *slabs = (int)((rows + sr - 1) / sr);
}

inline long om_per_slab(int n0, int n1, int n2) { return (long)n1 * n0 + n1 + (long)n2 * n1 + n2; }

bool om_sizes_ok(int rows, int n0, int n1, int n2) {
    return rows > 0 && n0 > 0 && n1 > 0 && n2 > 0 && om_per_slab(n0, n1, n2) * 64 * (long)sizeof(float) < (1L << 40)
        && (long)om_tiles(n1) * om_tiles(n0) + (long)om_tiles(n2) * om_tiles(n1) <= (1L << 24);
}

int om_vec(const float* p, long ld, int width) { return (ld % 4 == 0 && width % 4 == 0 && ((uintptr_t)p % 16) == 0) ? 1 : 0; }

}  // namespace

extern "C" long pit_mlp_bwd_params_ordered_mfma_workspace(int rows, int n0, int n1, int n2) {
    if (!om_sizes_ok(rows, n0, n1, n2)) return 0;
    int slabs, slab_rows;
    ord_partition(rows, n0, n1, n2, &slabs, &slab_rows);
    return (long)slabs * om_per_slab(n0, n1, n2) * (long)sizeof(float);
}

extern "C" int pit_mlp_bwd_params_ordered_mfma(const float* x, long ldx, int rows, int n0, int n1, int n2, const float* h,
                                               int out_gelu, const float* d_y, long ld_dy,
                                               float* d_w1, float* d_b1, float* d_w2, float* d_b2,
                                               int accumulate, const float* scratch, float* workspace, void* stream) {
    if (!x || !h || !d_y || !d_w1 || !d_b1 || !d_w2 || !d_b2 || !scratch || !workspace) return PIT_ERR_NULL;
    if (!om_sizes_ok(rows, n0, n1, n2) || ldx < n0 || ld_dy < n2) return PIT_ERR_SIZE;
    hipStream_t s = (hipStream_t)stream;
    OrdMfmaArgs g;
    ord_partition(rows, n0, n1, n2, &g.slabs, &g.slab_rows);
    const float* dz1 = scratch;                                           // the layout of pit_mlp_bwd_data
    const float* dz2 = out_gelu ? scratch + (long)rows * n1 : d_y;
    const long ld_dz2 = out_gelu ? n2 : ld_dy;
    // a slab of any operand must fit a 32-bit byte offset
    const long ld_max = std::max(std::max(ldx, ld_dz2), (long)std::max(n1, n0));
    if (((long)g.slab_rows * ld_max + OM_TILE) * 4 >= (long)PIT_MAX_BUFFER_BYTES) return PIT_ERR_SIZE;
    OrdProb& p1 = g.p[0];
    p1.A = dz1; p1.lda = n1; p1.B = x; p1.ldb = ldx; p1.M = n1; p1.N = n0;
    p1.a_vec = om_vec(p1.A, p1.lda, p1.M); p1.b_vec = om_vec(p1.B, p1.ldb, p1.N);
    p1.tx = om_tiles(n0); p1.tiles = om_tiles(n1) * om_tiles(n0); p1.off = 0;
    OrdProb& p2 = g.p[1];
    p2.A = dz2; p2.lda = ld_dz2; p2.B = h; p2.ldb = n1; p2.M = n2; p2.N = n1;
    p2.a_vec = om_vec(p2.A, p2.lda, p2.M); p2.b_vec = om_vec(p2.B, p2.ldb, p2.N);
    p2.tx = om_tiles(n1); p2.tiles = om_tiles(n2) * om_tiles(n1); p2.off = (long)n1 * n0 + n1;
    g.rows = rows; g.tiles = p1.tiles + p2.tiles;
    g.part = workspace; g.per_slab = om_per_slab(n0, n1, n2);
    g.dst[0] = d_w1; g.len[0] = (long)n1 * n0;
    g.dst[1] = d_b1; g.len[1] = n1;
    g.dst[2] = d_w2; g.len[2] = (long)n2 * n1;
    g.dst[3] = d_b2; g.len[3] = n2;
    g.accumulate = accumulate;
    const long wgs = (long)g.tiles * g.slabs;
    if (wgs > 0x7fffffffL) return PIT_ERR_SIZE;
    hipLaunchKernelGGL(ordered_dw_mfma_kernel, dim3((unsigned)wgs), dim3(256), 0, s, g);
    PIT_CHECK_LAUNCH();
    hipLaunchKernelGGL(ordered_dw_mfma_finish_kernel, dim3((unsigned)std::min<long>((g.per_slab + 255) / 256, 4096L)), dim3(256), 0, s, g);
    PIT_CHECK_LAUNCH();
    return 0;
}
