/* pit_hip.h -- C ABI of the MI355X-native PiT position-attention hot path.
 *
 * The reference (junfeng-chen/position_induced_transformer) has no FFI: its hot path
 * is a sequence of torch ops inside pit.py.  Each entry point below replaces one such
 * sequence (cited as pit.py:line) and is what a ctypes / pybind / cgo binding for this
 * path would bind.  Conventions:
 *   - plain `extern "C"`, raw DEVICE pointers (fp32 unless stated), int sizes, strides
 *     in ELEMENTS; `stream` is a hipStream_t passed as void* (NULL = default stream);
 *   - every function returns 0 on success, a negative PIT_ERR_* for an argument error,
 *     or a positive hipError_t; nothing allocates, frees or synchronises, so every call can
 *     be captured into a hipGraph; there is no MUTABLE process-global state (the math mode, the head-scale convention and
 *     the storage formats are arguments).  What the library does read once per process: diagnostic environment switches
 *     (PIT_NO_* / PIT_LDS_* / PIT_RR_*: force a slower kernel family for A/B measurements, listed in DESIGN.md section 4;
 *     never needed for correct results), and per-kernel function attributes (dynamic LDS limits) set on first use;
 *   - outputs and workspaces are caller-owned (the PyTorch host code allocates them).
 *
 * Mesh conventions: `mesh_batch` = 1 for the batch-free (fixed) meshes of
 * posatt_fixed / _periodic1d / _periodic2d (pit.py:129-144,186-200,243-258) where
 * the attention weights are shared by the whole batch, and = b for the per-sample
 * meshes of posatt (pit.py:46-52).  Meshes are (mesh_batch, n, space_dim) contiguous,
 * 1 <= space_dim <= PIT_MAX_SPACE_DIM (ABI 26; 1..3 before) for pit_select_wide_fwd, pit_plan_fwd, pit_neighbors_fwd,
 * pit_posatt_fwd / _fwd_job / _bwd, pit_posatt_dmesh and its workspace query: with 4..8 coordinates these run per-layer
 * kernels (streaming selection passes, dense rows / cols, candidate-list rows / cols, wave-per-row / per-key mesh
 * gradients).  pit_select_fwd keeps 1..3 (PIT_ERR_SIZE beyond).  The fused entries keep 1..3: pit_block_weights,
 * pit_slab_plan_build, pit_encoder_fwd / _bwd return PIT_ERR_SIZE, pit_satt_fwd / _bwd PIT_ERR_UNSUPPORTED; their
 * *_supported predicates do not see space_dim, so the caller routes around them (ops.py does).  Distances follow
 * ATen-CPU's summation order for torch.sum.
 */
#ifndef PIT_HIP_H
#define PIT_HIP_H

#ifdef __cplusplus
extern "C" {
#endif

#define PIT_ABI_VERSION 31
#define PIT_MAX_SPACE_DIM 8   /* largest space_dim any entry accepts */
#define PIT_DSCALE_SLOTS 1024 /* fp64 accumulators per head in pit_posatt_bwd's workspace */

/* distance metric (dist2att variants) */
#define PIT_METRIC_EUCLID     0   /* pit.py:47,134  sum_c (xo_c-xi_c)^2                         */
#define PIT_METRIC_PERIODIC1D 1   /* pit.py:190-194 wrap |dx| to min(|dx|, l-|dx|), coordinate 0 */
#define PIT_METRIC_PERIODIC2D 2   /* pit.py:248-253 per-coordinate wrap, then sum of squares     */

/* argument errors */
#define PIT_ERR_NULL     -1
#define PIT_ERR_SIZE     -2
#define PIT_ERR_METRIC   -3
#define PIT_ERR_UNSUPPORTED -4

int pit_version(void);
/* human-readable text for a return code of any function below */
const char* pit_error_string(int code);

/* Math mode of the MFMA contractions (attention forward and d(values), MLP GEMMs): the `math_mode`
 * ARGUMENT of every call that contracts - the library keeps no process-wide mode (thread-safe; a
 * captured hipGraph keeps the mode its launches were captured with).  The reference computes in
 * fp32 (pit.py has no autocast), so
 *   PIT_MATH_FP32: v_mfma_f32_32x32x2_f32, exact fp32 products - the parity mode;
 *   PIT_MATH_BF16: operands rounded to bf16 (RNE), bf16 MFMA with fp32 accumulation.  Distances,
 *     head scale, quantile thresholds, mask, softmax weights, the d(scale) reduction, loss and
 *     optimiser stay fp32 in both modes, so the kept sets are identical; outputs agree with the
 *     fp32 mode to ~1e-2 relative L2 (tests/test_gpu_bf16.py states the tolerance).
 *     Exception (stated, not silent): the small-regime fused kernels - pit_mlp_fwd / pit_mlp_bwd_data on 16-row slabs
 *     (mlp_fwd16_kernel, mlp_bwd16_kernel) and the fused processor blocks (pit_block_*: PIT_MATH_FP32 only, they
 *     return PIT_ERR_UNSUPPORTED otherwise) - are latency-bound, not MFMA-bound, and contract in fp32 in BOTH modes.
 * Any other value returns PIT_ERR_UNSUPPORTED. */
#define PIT_MATH_FP32 0
#define PIT_MATH_BF16 1
/* bf16 STORAGE of the large decoder-side tensors, OR-ed into the `math_mode` argument (PIT_MATH_BF16 only; ABI 11).
 * BASELINE configs 3 and 5 (Vorticity, NACA) are bound by the fp32 traffic of the decoder tail - the up-projection's
 * output (rows x H*hid), the decoder MLP's saved pre-activations and their gradients: 81 920 / 225 420 rows - not by
 * the matrix pipe; with these flags those tensors live in memory as bf16 (widened exactly on load, RNE on store), every
 * accumulation stays fp32.  Distances, mask, softmax weights, the d(scale) reduction, parameters and their gradients
 * are untouched.  A call whose shape does not take the kernels that implement a flag returns PIT_ERR_UNSUPPORTED
 * (ask pit_mlp_bf16_io_supported first).
 *   pit_posatt_fwd   PIT_IO_OUT_BF16   `out` is bf16 (candidate-list layers, no input copy)
 *   pit_posatt_bwd   PIT_IO_DOUT_BF16  `d_out` is bf16 (candidate-list layers)
 *   pit_mlp_fwd      PIT_IO_X_BF16     `x` is bf16;  PIT_IO_SAVE_BF16: z1, h are written as bf16
 *   pit_mlp_bwd*     PIT_IO_X_BF16, PIT_IO_SAVE_BF16 (z1, h and the dZ1 scratch - rows*n1 bf16 - are bf16),
 *                    PIT_IO_DX_BF16    `d_x` is written as bf16 */
#define PIT_IO_X_BF16    0x100
#define PIT_IO_SAVE_BF16 0x200
#define PIT_IO_DX_BF16   0x400
#define PIT_IO_OUT_BF16  0x800
#define PIT_IO_DOUT_BF16 0x1000
/* pit_posatt_fwd / pit_posatt_bwd, masked layers on candidate lists (round 4): OR-ed into math_mode, PIT_ATT_UNION asks for the
 * UNION-TILE kernels - 16 consecutive rows (one wavefront) contract against the union of their candidate keys (every key's value
 * row fetched once per tile, v_mfma_f32_16x16x4_f32) instead of one wavefront per row gathering its own keys.  Exact for any
 * input, fast when consecutive rows share their keys (grids, body-fitted meshes: a 16-row tile's union is 25-60 keys); the
 * caller decides per mesh plan.  Ignored where it does not apply: coordinate channels, self-attention concat, n_in > 4096,
 * n_head > 2, list capacity > 64, dim not a multiple of 8 or rows not 16-byte aligned (the per-row kernels run instead).
 * pit_posatt_bwd with this flag: d(scale) from the tiles; d(values) from the transposed lists when rev_ptr / rev_row are
 * given, else from the tiles (256-row blocks contracted on MFMA, their sums ADDED to memory with fp32 atomics - the call
 * zeroes d_values first; needs a dense d_values: ld_dvalues = dim, dvalues_bstride = n_in*dim; sums differ in the last
 * bits from run to run). */
#define PIT_ATT_UNION    0x2000
/* 1 if pit_mlp_fwd / pit_mlp_bwd* of this shape accept PIT_IO_X_BF16 | PIT_IO_SAVE_BF16 | PIT_IO_DX_BF16 (thin output
 * layer n2 <= 4 without trailing gelu, large regime, widths multiples of 8) */
int pit_mlp_bf16_io_supported(int rows, int n0, int n1, int n2, int out_gelu);

/* pit.py:48 (and :135,:196,:254): c_h = tan(0.25*pi*(1-1e-7)*(1+sin(lmda_h))).
 * Evaluated through fp64 with the reference's fp32 intermediate roundings. */
int pit_head_scale(const float* lmda, int n_head, float* scale_out, void* stream);

/* Selection pre-pass replacing the sort inside torch.quantile (pit.py:49,136,197,255).
 * For every row (mesh_batch*n_out rows of length n_in) of the UNSCALED squared distance
 * writes stats[0][row] = m_(k), stats[1][row] = m_(k+1) (k+1 clipped to n_in-1) and
 * stats[2][row] = min_j m.  rank_k = floor(fl32(q)*fl32(n_in-1)) (0-based).  With
 * need_kth = 0 only the row minimum is computed (locality 1.0: nothing is masked).
 * stats is 3*mesh_batch*n_out floats. */
int pit_select_fwd(const float* mesh_out, const float* mesh_in, int mesh_batch, int n_out, int n_in,
                   int space_dim, int metric, float period, int rank_k, int need_kth,
                   float* stats, void* stream);
/* pit_select_fwd for 1 <= space_dim <= PIT_MAX_SPACE_DIM (ABI 26); pit_select_fwd itself keeps space_dim in {1,2,3}. */
int pit_select_wide_fwd(const float* mesh_out, const float* mesh_in, int mesh_batch, int n_out, int n_in,
                        int space_dim, int metric, float period, int rank_k, int need_kth,
                        float* stats, void* stream);

/* The transposed lists (key -> listing rows) of candidate lists that were built WITHOUT them (rev_ptr = NULL in pit_plan_fwd /
 * pit_neighbors_fwd): round 4 - per-sample plans are rebuilt every step and only a backward that walks the lists by key
 * (d(values) of the candidate-list kernels) needs the transpose; the forward and d(scale) do not.  rev_ptr (mesh_batch, n_in+1),
 * rev_row (mesh_batch, n_out*cap), workspace 2*mesh_batch*n_in ints - as in pit_neighbors_fwd.  n_in <= 4096
 * (PIT_ERR_UNSUPPORTED otherwise: rebuild the plan with rev_ptr). */
int pit_lists_transpose(const int* nbr_idx, const int* nbr_cnt, int mesh_batch, int n_out, int n_in, int cap,
                        int* rev_ptr, int* rev_row, int* workspace, void* stream);

/* pit_select_fwd (need_kth = 1) and pit_neighbors_fwd in ONE pass over the rows: the distances of
 * a row stay in registers, the order statistics are searched on a narrowed candidate set and the
 * lists are emitted from the same registers (rows longer than 4096 keys fall back to the two
 * streaming passes).  Arguments as in those two functions; stats is written, then used.
 * flags (0 = let the library choose; ABI 17 - these were environment reads per call): PIT_PLAN_WAVE_PER_ROW keeps the
 * wave-per-row kernel where the one-row-per-lane kernel (per-sample meshes from 32 768 rows) would run, PIT_PLAN_TWO_PASSES
 * forces the two streaming passes.  Same results either way (tests compare them). */
#define PIT_PLAN_WAVE_PER_ROW 1
#define PIT_PLAN_TWO_PASSES   2
int pit_plan_fwd(const float* mesh_out, const float* mesh_in, int mesh_batch, int n_out, int n_in,
                 int space_dim, int metric, float period, int rank_k, float* stats, int cap,
                 int* nbr_idx, int* nbr_cnt, int* rev_ptr, int* rev_row, int* workspace, int flags, void* stream);

/* Candidate lists for the masked layers (sparse path).  For every row: the keys with
 * m <= m_(k+1)*(1+2^-21) - a superset of the kept set of pit.py:50 for ANY head scale (k+2 keys
 * plus ties), so it depends on the meshes only.  nbr_idx (rows, cap) int32, nbr_cnt (rows) int32
 * holds the TRUE count (a row with count > cap is truncated and consumers scan all keys for it).
 * stats: from pit_select_fwd with need_kth=1.
 * Optionally (rev_ptr != NULL) also the transposed lists (key -> rows listing it) as CSR per mesh
 * sample, for d(values): rev_ptr (mesh_batch, n_in+1), rev_row (mesh_batch, n_out*cap) row
 * indices local to the sample, -1 = unused slot; workspace: 2*mesh_batch*n_in ints.  Rows with
 * count > cap are left out of the transpose (pit_posatt_bwd adds them densely). */
int pit_neighbors_fwd(const float* mesh_out, const float* mesh_in, int mesh_batch, int n_out, int n_in,
                      int space_dim, int metric, float period, const float* stats, int cap,
                      int* nbr_idx, int* nbr_cnt, int* rev_ptr, int* rev_row, int* workspace, void* stream);

/* Fused dist2att + convolution forward (pit.py:46-57 / 133-144 and the periodic
 * variants; posatt.forward :37-44 with copy_inputs, posatt_cross*.forward :63-71).
 *   values   (batch, n_in, dim)   rows ld_values apart, samples values_bstride apart
 *   head     n_head floats: lmda (head_is_scale=0) or the scale c itself (=1)
 *   stats    from pit_select_fwd (may be NULL when masked=0 and self_attn=1: min is 0)
 *   rank_w   fractional part of the quantile rank (fp32), used when masked=1
 *   out      (batch, n_out, ...) rows ld_out apart; head h / channel d is written at
 *            column out_col0 + h*dim + d; with copy_inputs=1 (self attention, n_out ==
 *            n_in) values[b,n,:] is also copied to columns [0,dim) -> torch.cat of :44
 *   rowstat  (mesh_batch, n_head, n_out, 4) = {T, S_min, 1/rowsum, sum_j P*m} saved for
 *            the backward; scale_out (n_head) receives the c that was used.
 *   nbr_idx/nbr_cnt/nbr_cap: candidate lists from pit_neighbors_fwd (masked layers); NULL = the
 *            dense MFMA kernel.  With lists the layer costs O(n_out * k * columns).
 *   coord_dims: > 0 fuses the coordinate concat of the task forwards (train_darcy.py:51-55:
 *            func_in = cat((tile(mesh_in), func_in), -1)): value channels [0, coord_dims) are the key
 *            coordinates, read from mesh_in; `values` then holds the other dim - coord_dims channels (and
 *            d_values of pit_posatt_bwd has that many).  Candidate-list kernels only
 *            (PIT_ERR_UNSUPPORTED otherwise: the caller materialises the concat). */
int pit_posatt_fwd(const float* mesh_out, const float* mesh_in, int mesh_batch, int n_out, int n_in,
                   int space_dim, int metric, float period,
                   const float* values, int batch, int dim, long ld_values, long values_bstride,
                   const float* head, int n_head, int head_is_scale,
                   const float* stats, float rank_w, int masked, int self_attn,
                   float* out, long ld_out, long out_bstride, int out_col0, int copy_inputs,
                   float* rowstat, float* scale_out,
                   const int* nbr_idx, const int* nbr_cnt, int nbr_cap, int coord_dims, int math_mode, void* stream);

struct pit_mlp_params_job;

/* pit_posatt_fwd with a RIDER (round 4): the processor's block weights (pit_block_weights, declared below - they depend on
 * the latent mesh and the lmda's only, not on this layer's data) formed by extra workgroups of the SAME launch when this
 * layer runs on the small candidate-list kernel (the down-projection of the small regime), by a launch of their own
 * right after it otherwise.  job == NULL: exactly pit_posatt_fwd.  The job's fields are pit_block_weights' arguments. */
struct pit_block_weights_job {
    const float* mesh; int n_pts, space_dim, metric; float period;
    int n_layers; const float* const* heads; int head_is_scale, n_head;
    float *e, *q, *inv, *rowstat, *scale_out;
};
int pit_posatt_fwd_job(const float* mesh_out, const float* mesh_in, int mesh_batch, int n_out, int n_in,
                       int space_dim, int metric, float period,
                       const float* values, int batch, int dim, long ld_values, long values_bstride,
                       const float* head, int n_head, int head_is_scale,
                       const float* stats, float rank_w, int masked, int self_attn,
                       float* out, long ld_out, long out_bstride, int out_col0, int copy_inputs,
                       float* rowstat, float* scale_out,
                       const int* nbr_idx, const int* nbr_cnt, int nbr_cap, int coord_dims, int math_mode, void* stream,
                       const struct pit_block_weights_job* job);

/* Backward of pit_posatt_fwd (closed form; the reference uses
 * autograd).  d_out has the layout of `out` (columns out_col0 + h*dim + d).
 *   d_values (batch, n_in, dim): written (NULL = not needed).  With add_residual=1 (self
 *            attention) the gradient of the copied inputs, d_out[b,j,0:dim], is added.
 *   scale    the c written to scale_out by the forward (NULL = recompute from head)
 *   d_head   n_head floats (NULL = not needed): gradient w.r.t. lmda (head_is_scale=0) or
 *            w.r.t. c (=1); accumulate_head is a bit set: PIT_HEAD_ACCUMULATE adds to the current
 *            contents instead of writing; PIT_HEAD_DEFER leaves the fp64 accumulators LOADED and
 *            skips the finishing kernel - the caller later drains several layers at once with
 *            pit_posatt_dhead_finish (each deferred layer then needs its own workspace).
 *   workspace: n_head*PIT_DSCALE_SLOTS doubles: fp64 accumulators for d c.  They must be ZERO
 *            on entry and are left zero on exit (the finishing kernel drains them with atomic
 *            exchanges, applies d c/d lmda and writes d_head), so a caller allocates and zeroes
 *            them once; no per-call memset.
 *   nbr_complete: 1 = the caller knows that no row's candidate list overflowed (nbr_cnt <= nbr_cap
 *            everywhere, e.g. checked once for a cached fixed-mesh plan): the pass that adds the
 *            overflowed rows to d_values is not launched.  0 = unknown (always correct).
 * d_values and d_head are computed by independent kernels: a caller may issue two calls (one
 * with d_values == NULL, one with d_head == NULL) on different streams to overlap them.
 *   rider    NULL, or the arguments of a pit_mlp_bwd_params call the caller has postponed (the weight-gradient
 *            reductions of the MLP whose d_x is this call's d_out: pit.py:116-121 runs mlp -> attention, so the
 *            backward runs them in this order and nothing downstream needs d_w*).  The call performs it: inside
 *            the attention launch when both are small (latency-bound grids sharing the chip), otherwise as the
 *            separate launches pit_mlp_bwd_params would have made.  Read during the call only. */
typedef struct pit_mlp_params_job {          /* = the argument list of pit_mlp_bwd_params */
    const float* x; long ldx; int rows, n0, n1, n2; const float* h; int out_gelu;
    const float* d_y; long ld_dy;
    float *d_w1, *d_b1, *d_w2, *d_b2; int accumulate; const float* scratch; int math_mode;
} pit_mlp_params_job;
#define PIT_HEAD_ACCUMULATE 1
#define PIT_HEAD_DEFER      2
#define PIT_HEAD_IS_SCALE   4   /* pit_posatt_dhead_finish only: d_head is w.r.t. c, no chain rule */
int pit_posatt_bwd(const float* mesh_out, const float* mesh_in, int mesh_batch, int n_out, int n_in,
                   int space_dim, int metric, float period,
                   const float* values, int batch, int dim, long ld_values, long values_bstride,
                   const float* head, int n_head, int head_is_scale, const float* scale,
                   const float* rowstat, int masked,
                   const float* d_out, long ld_dout, long dout_bstride, int out_col0,
                   float* d_values, long ld_dvalues, long dvalues_bstride, int add_residual,
                   float* d_head, int accumulate_head, double* workspace,
                   const int* nbr_idx, const int* nbr_cnt, int nbr_cap, int nbr_complete,
                   const int* rev_ptr, const int* rev_row, const pit_mlp_params_job* rider,
                   int coord_dims, int math_mode, void* stream);

/* Gradients w.r.t. the mesh coordinates of one pit_posatt_fwd call (ABI 25).  The reference forms the distances with ordinary
 * tensor ops, m = sum((mesh_out[:,None] - mesh_in[None])**2) (pit.py:47,134), so autograd differentiates through the meshes.
 * Per head, with P the kept weights, g_i = d_out[i, out_col0 + h*dim : +dim], gv_ij = g_i . values_j, a_i = sum_j P_ij gv_ij and
 * s_ij = P_ij (gv_ij - a_i):
 *     d_mesh_out[i] = 2c sum_j s_ij (mesh_in[j] - mesh_out[i]),   d_mesh_in[j] = 2c sum_i s_ij (mesh_out[i] - mesh_in[j])
 * summed over the heads and, for batch-free meshes (mesh_batch = 1), over the samples.  The quantile threshold only feeds a
 * comparison and contributes nothing.
 *   Arguments up to rev_row: those of the pit_posatt_bwd call of the same layer (rowstat / scale from the forward; the candidate
 *            lists select the same kernels, rev_ptr / rev_row are needed for d_mesh_in; nbr_complete as there).
 *   d_mesh_out (mesh_batch, n_out, space_dim), d_mesh_in (mesh_batch, n_in, space_dim): written, or added to with accumulate=1;
 *            NULL = not needed.  Self attention may pass the same buffer for both: the key terms are then added to the row terms.
 *   workspace: pit_posatt_dmesh_workspace(...) bytes, no initial contents needed.  Per-sample partials are summed in a fixed
 *            order (no atomics): the same bits on every run.  No host synchronisation, no allocation.
 * fp32 only (the d_out and values of the fp32 math mode); a periodic metric returns PIT_ERR_UNSUPPORTED (the reference also
 * differentiates through the period and the minimum / abs tie rules, pit.py:190-191,248-250).  No coordinate channels
 * (coord_dims = 0: the caller materialises the concat). */
int pit_posatt_dmesh(const float* mesh_out, const float* mesh_in, int mesh_batch, int n_out, int n_in,
                     int space_dim, int metric, float period,
                     const float* values, int batch, int dim, long ld_values, long values_bstride,
                     const float* head, int n_head, int head_is_scale, const float* scale,
                     const float* rowstat, int masked,
                     const float* d_out, long ld_dout, long dout_bstride, int out_col0,
                     const int* nbr_idx, const int* nbr_cnt, int nbr_cap, int nbr_complete,
                     const int* rev_ptr, const int* rev_row,
                     float* d_mesh_out, float* d_mesh_in, int accumulate, void* workspace, void* stream);
/* Bytes of pit_posatt_dmesh's workspace (0 for invalid sizes). */
long pit_posatt_dmesh_workspace(int mesh_batch, int n_out, int n_in, int space_dim, int batch, int n_head);

/* Finishing step of n_layers (<= 32) pit_posatt_bwd calls issued with PIT_HEAD_DEFER, in ONE
 * launch: per layer l drains workspaces[l] (n_heads[l]*PIT_DSCALE_SLOTS doubles, left zero), applies
 * d c / d lmda (heads[l] = lmda, scales[l] = the forward's c or NULL to recompute; with
 * PIT_HEAD_IS_SCALE in flags[l] the result is d c itself) and writes or (PIT_HEAD_ACCUMULATE) adds to
 * d_heads[l].  The arrays are HOST arrays of device pointers / ints, read during the call.
 * rider (ABI 17): NULL, or a postponed pit_mlp_bwd_params the pass has no later launch for (the encoder MLP's, when its fused
 * backward is the pass's last launch): performed by extra workgroups of this launch when small, else by its own launches. */
int pit_posatt_dhead_finish(int n_layers, double* const* workspaces, float* const* d_heads,
                            const float* const* heads, const float* const* scales, const int* n_heads,
                            const int* flags, const pit_mlp_params_job* rider, void* stream);

/* ---- Fused processor blocks (batch-free meshes, small regime; csrc/pit_block.hip) ------------------------------
 * pit.processor (pit.py:114-122) is n_blocks x [posatt.forward (self attention on the latent mesh, locality 1.0:
 * pit.py:102) -> kaiming_mlp -> gelu].  For the batch-free operators the softmax weights of every block depend on
 * (mesh_ltt, lmda_l) only, so ONE launch forms them for all blocks of the step and each block's forward / backward
 * chain becomes one launch (attention as plain MFMA contractions + the MLP phases on the same 16-row slab).
 *
 * pit_block_supported: 1 when this shape takes the fused path (dim = hid_dim = 64, n_head in {1,2}, n_pts a multiple
 * of 256 and <= 2048 (E and Q are n_layers*n_head*n_pts^2 floats each), 256 <= batch*n_pts <= 16384 rows (measured on MI355X: +27 % per step at
 * Darcy batch 16, +19 % at 32, +2 % at 64 over the unfused kernels)); callers fall back to pit_posatt_* + pit_mlp_* otherwise. */
int pit_block_supported(int n_pts, int n_head, int dim, int batch);

/* Weights of n_layers (<= 16) self-attention layers on one batch-free mesh (n_pts, space_dim), nothing masked:
 *   e   (n_layers, n_head, n_pts, n_pts)  exp(-c_lh m[n,j])  - un-normalised and symmetric (S_min = 0: every row holds
 *                                          its own point), so e serves the forward (rows) and d(values) (columns)
 *   q   (same shape, or NULL: forward only) e (m - mbar_n) / rowsum_n : the weights of the d(scale) contraction
 *   inv (n_layers, n_head, n_pts)          1 / rowsum
 *   rowstat (n_layers, n_head, n_pts, 4)   {T = +inf, S_min = 0, 1/rowsum, mbar} exactly as pit_posatt_fwd saves it, so
 *                                          pit_posatt_bwd can serve any layer of the stack as well
 *   scale_out (n_layers, n_head)           the c that was used
 * heads: HOST array of n_layers device pointers (n_head floats each: lmda, or c itself with head_is_scale = 1). */
int pit_block_weights(const float* mesh, int n_pts, int space_dim, int metric, float period, int n_layers,
                      const float* const* heads, int head_is_scale, int n_head, float* e, float* q,
                      float* inv, float* rowstat, float* scale_out, void* stream);

/* One processor block forward: xcat (batch*n_pts, (1+n_head)*dim) holds the block's input in columns [0, dim); the
 * attention output of head h is written to columns [(1+h)*dim, (2+h)*dim) (torch.cat((inputs, conv), -1), pit.py:44)
 * and the block's MLP ((1+n_head)*dim -> dim -> dim, arguments as pit_mlp_fwd) runs on the slab in the same launch.
 * e / inv: this layer's slices of pit_block_weights' outputs. */
int pit_block_fwd(const float* e, const float* inv, int n_pts, int n_head, int dim, int batch, float* xcat,
                  const float* w1, const float* b1, const float* w2, const float* b2, int out_gelu,
                  float* z1, float* h, float* z2, float* y, long ldy, int math_mode, void* stream);

/* One block of the backward chain.  Given d_xcat (gradient of this block's concat tensor, complete):
 *   d(values) = d_xcat[:, 0:dim] + sum_h e_h^T (d_xcat[:, head h] / rowsum_h)   per 16-point slab, then
 *   - with the PREVIOUS block's MLP (w1 (dim, n0_prev), w2 (dim, dim), its saved z1 / z2, out_gelu): the data path of
 *     that MLP's backward on the slab - dZ2, dZ1 into scratch_prev (rows*(2*dim) floats, the layout of
 *     pit_mlp_bwd_data) and dX into d_xprev (rows, n0_prev) (NULL = not needed);
 *   - with w1 == NULL: d(values) is written to d_values (rows, dim).
 *   dscale != NULL: this layer's d(scale) partial sums are ADDED to these accumulators (n_head*PIT_DSCALE_SLOTS
 *     doubles, the PIT_HEAD_DEFER convention of pit_posatt_bwd: drain with pit_posatt_dhead_finish); needs qw and
 *     xcat (the block's concat tensor, whose first dim columns are the attention's values).
 *   rider: as in pit_posatt_bwd (the weight-gradient reductions of this block's own MLP).
 *   rider2: a second postponed job carried the same way - typically a SLICE of rows of a larger one (the decoder MLP's
 *     reductions are row sums: any partition of the rows, each slice with accumulate = 1, gives the same gradient), so
 *     that a job too big for one launch is spread over the block launches of the backward chain. */
int pit_block_bwd(const float* e, const float* inv, const float* qw, int n_pts, int n_head, int dim, int batch,
                  const float* d_xcat, const float* xcat, double* dscale,
                  const float* w1, const float* w2, const float* z1, const float* z2, int out_gelu, int n0_prev,
                  float* d_xprev, long ld_dxprev, float* scratch_prev,
                  float* d_values, long ld_dvalues,
                  const struct pit_mlp_params_job* rider, const struct pit_mlp_params_job* rider2,
                  int math_mode, void* stream);

/* ---- Fused encoder-side and decoder-side launches (batch-free meshes, small regime; round 5; csrc/pit_edge.hip) ------------
 * pit.encoder (pit.py:108-112) = cross attention mesh_in -> mesh_ltt + kaiming_mlp + gelu, pit.decoder (pit.py:124-127) =
 * cross attention mesh_ltt -> mesh_out + kaiming_mlp, each as ONE launch per direction on 16-row slabs of one sample: the
 * attention output of a slab stays in LDS as the A operand of the MLP, and in the backward the gradient of that tensor
 * ((batch, n_out, n_head*dim): 7.6 MB at Darcy b=8) never exists in memory.
 *
 * pit_slab_plan: the lmda-independent part of a masked cross-attention layer on a FIXED mesh pair, per 16-row slab - built once
 * (pit_slab_plan_build) from the candidate lists of pit_plan_fwd, which must be complete (no row's count above cap; report[1]
 * says so) and, for the decoder, have unions of at most PIT_SLAB_UNION_MAX keys (report[0] = the largest union):
 *   m     (n_slabs*16, cap) squared distance of every candidate (rows beyond n_out: unused), the fp32 expression of pit.py:47 /
 *         :192-194 / :251-253; slot (n_slabs*16, cap) the candidate's position in the sorted union of its slab's keys;
 *   keys  (n_slabs, PIT_SLAB_UNION_MAX) that union, nkeys (n_slabs) its size.  stats / rank_w / idx / cnt / cap as pit_posatt_fwd.
 * Which mesh rows a slab holds (patch geometry): patch_w == 0 - `rows` CONSECUTIVE rows, slab s = rows [s*rows, (s+1)*rows), n_slabs =
 * ceil(n_out / rows).  patch_w > 0 (pit_decoder_weights / _fwd / _bwd only; rows == 16) - mesh_out is a row-major grid_w x grid_h
 * tensor-product grid (n_out == grid_w*grid_h, mesh row of grid point (i, j) = i*grid_w + j) and a slab is a patch_w x patch_h PATCH
 * of it (patch_w*patch_h == rows, patch_w a power of two): with ppr = ceil(grid_w / patch_w), slab s is patch (s / ppr, s % ppr) and
 * its row r the grid point (pi*patch_h + r / patch_w, pj*patch_w + r % patch_w) - valid when inside the grid; n_slabs =
 * ceil(grid_h / patch_h) * ppr.  The rows of a patch list neighbouring keys, so the union is about half a strip's (Darcy 43x43 ->
 * 16x16: 12.9 keys on average, at most 19 - the 32-slot tile - against 24.5 / 32 of the consecutive plan).  m / slot stay slab-relative ((s*rows + r)*cap + i, zero for invalid
 * rows); every tensor of the launches keeps its mesh-row layout.
 * All pointers are device memory owned by the caller; the struct is passed by pointer and read during the call. */
#define PIT_SLAB_UNION_MAX 64
typedef struct pit_slab_plan {
    int n_out, n_in, cap, n_slabs, umax;
    const float* stats; float rank_w;
    const int* idx; const int* cnt;
    const float* m; const unsigned short* slot; const int* keys; const int* nkeys;
    int rows;       /* rows per slab (ABI 19): 16 for the fused launches and pit_union_att_*, 64 / 128 / 256 for pit_fold_* */
    int grid_w, grid_h, patch_w, patch_h;       /* slab geometry; all 0: consecutive rows */
} pit_slab_plan;
/* report: 3 ints, ZERO on entry (largest union, 1 if a list overflowed, longest list).  n_in <= 16384.  rows_per_slab: 16, 64, 128
 * or 256; m / slot hold n_slabs*rows_per_slab rows, n_slabs = ceil(n_out / rows_per_slab). */
int pit_slab_plan_build(const float* mesh_out, const float* mesh_in, int n_out, int n_in, int space_dim, int metric, float period,
                        const int* nbr_idx, const int* nbr_cnt, int cap, int rows_per_slab, float* m, unsigned short* slot,
                        int* keys, int* nkeys, int* report, void* stream);
/* The same for slabs that are patch_w x patch_h patches of a row-major grid_w x grid_h output grid (see pit_slab_plan):
 * n_out == grid_w*grid_h, patch_w*patch_h == 16, patch_w a power of two; n_slabs = ceil(grid_h / patch_h) * ceil(grid_w / patch_w).
 * stats / rank_w: the plan's (pit_plan_fwd).  The union holds only the candidates SOME head scale can keep - m <= lerp(m_(k),
 * m_(k+1), rank_w) + 2^-20 m_(k+1), which covers every fp32 rounding of the mask decision - not the whole lists (every key up to
 * m_(k+1)): a candidate beyond it has slot 65535 and belongs to no tile.  report[0] is the largest such union. */
int pit_slab_plan_build_patch(const float* mesh_out, const float* mesh_in, int n_out, int n_in, int space_dim, int metric,
                              float period, const int* nbr_idx, const int* nbr_cnt, int cap, int grid_w, int grid_h, int patch_w,
                              int patch_h, const float* stats, float rank_w, float* m, unsigned short* slot, int* keys, int* nkeys,
                              int* report, void* stream);
/* 1 when the fused launches cover this shape: n_head 1 or 2, dim (= the MLP's hidden width) 32 or 64, 256 <= batch*rows <= 2^20 */
int pit_edge_supported(int n_head, int dim, int batch, int rows_per_sample);
/* The up-projection's softmax weights for one step: they depend on (mesh pair, lmda) only, so they are formed ONCE (one workgroup
 * per slab) and every (sample, slab) workgroup of pit_decoder_fwd / _bwd reads its tile as an MFMA operand:
 *   pw (n_slabs, n_head, 16, um) = P (normalised), qw (same shape; NULL: forward only) = P (m - mbar), zeros where a row does not
 *   list a slot; um = 16 (patch plans), 32, 48 or 64 >= max_union (report[0] of pit_slab_plan_build), max_count = report[2];
 *   scale_out (n_head) = c.
 * As a launch of its own, or - the job struct - as extra workgroups of pit_encoder_fwd's launch. */
/* um of pit_decoder_weights / _fwd / _bwd for this plan and largest union (what sizes pw / qw); negative: an argument error */
int pit_decoder_union_slots(const pit_slab_plan* plan, int max_union);
int pit_decoder_weights(const pit_slab_plan* plan, const float* head, int head_is_scale, int n_head, int max_union, int max_count,
                        float* pw, float* qw, float* scale_out, const float* w1, float* w1f, int dim, void* stream);
/* w1 / w1f (both or neither; ABI 18): the decoder MLP's first weight w1 (dim, n_head*dim), copied to w1f in the order the lanes of
 * pit_decoder_fwd consume it as MFMA operand fragments (the copy is part of the step because w1 changes once per step). */
typedef struct pit_decoder_weights_job {
    const pit_slab_plan* plan; const float* head; int head_is_scale, n_head, max_union, max_count;
    float *pw, *qw, *scale_out;
    const float* w1; float* w1f; int dim;
} pit_decoder_weights_job;
/* pit.decoder forward.  values (batch, n_in, dim) rows ld_values apart; pw from pit_decoder_weights; the MLP is
 * (n_head*dim -> dim -> n2), n2 <= 4, no trailing gelu; y (batch*n_out, n2).  Saved for the backward when given (all or none):
 * x (batch*n_out, n_head*dim) the attention's output, z1 / h (batch*n_out, dim).  zero_buf: zero_n floats cleared on the way (the
 * d_values buffer pit_decoder_bwd adds to).  loss_part != NULL: the slab's partial sums of RelLpNorm(true, y*scale + shift)
 * (utils.py:86-98, p = 1 or 2) as (batch, n2, n_slabs, 2) doubles - plain stores, nothing to zero, the same bits on every run.
 * max_union: report[0] of pit_slab_plan_build: sizes the launch's LDS tiles (as in pit_decoder_weights).
 * w1f: the fragment-order copy of w1 formed by pit_decoder_weights for THIS w1, or NULL (the launch then reads w1's rows). */
int pit_decoder_fwd(const pit_slab_plan* plan, const float* values, long ld_values, long values_bstride, int batch,
                    int n_head, int dim, const float* pw,
                    const float* w1, const float* w1f, const float* b1, const float* w2, const float* b2, int n2,
                    float* x, float* z1, float* h, float* y, float* zero_buf, long zero_n,
                    const float* loss_true, const float* loss_scale, const float* loss_shift, int loss_p, double* loss_part,
                    int max_union, void* stream);
/* pit.decoder backward: d_y (batch*n_out, n2) -> dz1 (batch*n_out, dim: the scratch of the MLP's weight-gradient reductions,
 * pit_mlp_bwd_params with d_y and this scratch), d_values (batch, n_in, dim) ADDED to (fp32 atomics; zero on entry), the layer's
 * d(scale) accumulators (PIT_HEAD_DEFER convention; finish with the scale_out of pit_decoder_weights).  d_y == NULL: the loss
 * inside - d(pred) is formed from loss_part (the forward's partial sums), multiplied by *loss_seed when given, written to d_pred
 * (batch*n_out, n2); *loss_out receives sum_b mean_c ||true - pred'|| / ||true||, norms_out (batch, n2, 2) the norms (may be NULL). */
int pit_decoder_bwd(const pit_slab_plan* plan, const float* values, long ld_values, long values_bstride, int batch,
                    int n_head, int dim, const float* pw, const float* qw,
                    const float* w1, const float* w2, int n2, const float* z1,
                    const float* d_y, long ld_dy, float* dz1, float* d_values, long dvalues_bstride, double* dscale,
                    const float* loss_pred, const float* loss_true, const float* loss_scale, const float* loss_shift,
                    const float* loss_seed, int loss_p, const double* loss_part, float* d_pred, float* loss_out,
                    float* norms_out, int max_union, void* stream);
/* The same union-tile contraction WITHOUT the MLP, for any value width that is a multiple of 64 (masked cross attention on a
 * batch-free mesh pair with a slab plan: the up-projections of Vorticity / Cylinder at hid 256): a workgroup per (sample, slab,
 * 64-column chunk).  out[b, n, h*dim + d] (no input copy, column offset 0) fp32 or - out_bf16 - bf16; the backward reads d_out of the
 * same layout ONCE, ADDS d(values) (fp32 atomics; zero on entry; NULL: not needed) and / or the d(scale) accumulators (PIT_HEAD_DEFER
 * convention; NULL: not needed).  pw / qw from pit_decoder_weights. */
int pit_union_att_supported(int n_head, int dim, int batch, int rows_per_sample);
int pit_union_att_fwd(const pit_slab_plan* plan, const float* values, long ld_values, long values_bstride, int batch,
                      int n_head, int dim, const float* pw, void* out, long ld_out, long out_bstride, int out_bf16,
                      int max_union, void* stream);
int pit_union_att_bwd(const pit_slab_plan* plan, const float* values, long ld_values, long values_bstride, int batch,
                      int n_head, int dim, const float* pw, const float* qw,
                      const void* d_out, long ld_dout, long dout_bstride, int dout_bf16,
                      float* d_values, long ld_dvalues, long dvalues_bstride, double* dscale, int max_union, void* stream);
/* ---- The decoder side with the decoder MLP's first layer folded into the values (round 6; csrc/pit_fold.hip) -------------------
 * pit.decoder (pit.py:124-127) = de(up(values)) with nothing non-linear between the up-projection and de.mlp1, so
 *     Z1 = sum_h P_h (V W1_h^T) + b1,   W1_h = W1[:, h*dim : (h+1)*dim]
 * - the first Linear runs on the n_in LATENT points instead of the n_out output points, and the (batch, n_out, n_head*dim) tensor of
 * pit.py:125 never exists.  vw (batch, n_in, dim*n_head) is HEAD-INTERLEAVED: vw[b, j, n*n_head + h] = sum_d values[b, j, d] W1[n][h*dim + d]
 * = pit_linear_fwd(values, w = W1's memory read as an (n_head*dim, dim) row-major matrix) - no permuted copy of W1, and the weight
 * gradient of that Linear has W1.grad's layout.  For batch-free mesh pairs:
 *   pit_slab_plan_build(..., rows_per_slab = 64 | 128 | 256)  the plan (tall slabs: their unions must fit PIT_SLAB_UNION_MAX)
 *   pit_fold_weights   pw / qw (n_slabs*n_head, rows, um) for one step, as pit_decoder_weights; pw16 / qw16 (optional): the same tiles
 *                      rounded to bf16 - what pit_fold_att_fwd / _bwd take as pw / qw in the bf16 math mode
 *   pit_fold_att_fwd   z[b, n, c] = sum_h sum_j P_h[n][j] vw[b, j, c*n_head + h]        (fp32, or bf16 with PIT_IO_OUT_BF16)
 *   pit_fold_att_bwd   d_vw[b, j, c*n_head + h] += sum_n P_h[n][j] dz[b, n, c] (fp32 atomics, ZERO on entry; NULL: not needed),
 *                      d(scale) accumulators (PIT_HEAD_DEFER convention; NULL: not needed); dz bf16 with PIT_IO_DOUT_BF16
 * math_mode PIT_MATH_FP32: v_mfma_f32_16x16x4_f32 on the fp32 pw / qw; PIT_MATH_BF16: pw / qw ARE pw16 / qw16 (a workgroup reads half the
 * bytes per pass and rounds nothing), the value rows rounded to bf16 in LDS, v_mfma_f32_16x16x32_bf16.
 * dim a multiple of 64, n_head 1 or 2, every tensor below 2 GiB (pit_fold_supported). */
int pit_fold_supported(int n_head, int dim, int batch, int rows_per_sample, int n_in);
int pit_fold_weights(const pit_slab_plan* plan, const float* head, int head_is_scale, int n_head, int max_union, int max_count,
                     float* pw, float* qw, float* scale_out, unsigned short* pw16, unsigned short* qw16, void* stream);
int pit_fold_att_fwd(const pit_slab_plan* plan, const float* vw, long ld_vw, long vw_bstride, int batch, int n_head, int dim,
                     const void* pw, void* z, long ld_z, long z_bstride, int max_union, int math_mode, void* stream);
int pit_fold_att_bwd(const pit_slab_plan* plan, const float* vw, long ld_vw, long vw_bstride, int batch, int n_head, int dim,
                     const void* pw, const void* qw, const void* dz, long ld_dz, long dz_bstride,
                     float* d_vw, long ld_dvw, long dvw_bstride, double* dscale,
                     float* tiles, const int* rev_ptr, const int* rev_ent, int max_union, int math_mode, void* stream);
/* tiles != NULL (with d_vw): NO atomics - every (sample, slab) writes its sums into its own tile of `tiles` (batch, n_slabs,
 * PIT_SLAB_UNION_MAX, dim*n_head floats) and a second launch writes d_vw[b, j, :] = the sum of the tile rows that hold key j, in the
 * fixed order of the CSR lists rev_ptr (n_in + 1) / rev_ent (entries slab*PIT_SLAB_UNION_MAX + slot, grouped by key): d_vw need not
 * be zero on entry and is the same bits on every run. */
/* The rest of `de` (pit.py:21-26 after the first Linear) for out_dim = n2 <= 4 and n1 in {64, 128, 256}:
 *   pit_thin_tail_fwd   y[m][o] = sum_n gelu_erf(z[m][n] + b1[n]) w2[o][n] + b2[o]                      (nothing is saved)
 *   pit_thin_tail_bwd   dz[m][n] = (sum_o d_y[m][o] w2[o][n]) gelu'(z[m][n] + b1[n]), and ADDS d_b1[n] = sum_m dz[m][n],
 *                       d_w2[o][n] = sum_m d_y[m][o] gelu(z[m][n] + b1[n]), d_b2[o] = sum_m d_y[m][o] to the gradients (partial sums meet
 *                       in `scratch` - pit_thin_tail_scratch_floats() floats, ZERO on first use, left zero - and a finishing launch adds
 *                       them: the gradients are complete when the call's launches are).
 * math_mode: PIT_MATH_FP32 - libm's erff; PIT_MATH_BF16 - the polynomial normal CDF of pit_common.h (|error| 1.4e-8); PIT_IO_X_BF16:
 * z (and dz) are bf16 in memory. */
int pit_thin_tail_scratch_floats(void);
int pit_thin_tail_fwd(const void* z, long ldz, int rows, int n1, int n2, const float* b1, const float* w2, const float* b2,
                      float* y, long ldy, int math_mode, void* stream);
int pit_thin_tail_bwd(const void* z, long ldz, int rows, int n1, int n2, const float* b1, const float* w2,
                      const float* d_y, long ld_dy, void* dz, long ld_dz, float* d_b1, float* d_w2, float* d_b2,
                      float* scratch, int math_mode, void* stream);
/* y = x w^T without bias (w (n_out, n_in) contiguous; zero_bias: n_out zeros) and its backward d_x = d_y w (NULL: not needed),
 * d_w (+)= d_y^T x (NULL: not needed; accumulate = 0 zeroes it first) - the GEMM launchers of pit_mlp_fwd / _bwd. */
int pit_linear_fwd(const float* x, long ldx, int rows, int n_in, int n_out, const float* w, const float* zero_bias,
                   float* y, long ldy, int math_mode, void* stream);
int pit_linear_bwd(const float* x, long ldx, int rows, int n_in, int n_out, const float* w, const float* d_y, long ld_dy,
                   float* d_x, long ld_dx, float* d_w, int accumulate, int math_mode, void* stream);

/* pit.encoder forward.  Value channels [0, coord_dims) are the key coordinates (mesh_in; train_darcy.py:51-55), the other
 * value_dim channels come from values (batch, n_in, value_dim); n_head*(coord_dims + value_dim) <= 16.  The MLP is
 * (n_head*(coord_dims+value_dim) -> dim -> dim) followed by gelu; y rows ldy apart (the first columns of the processor's concat
 * buffer).  clear_buf: clear_n floats zeroed on the way (the step's flat gradient buffer).  weights: pit_block_weights' arguments,
 * dec_weights: pit_decoder_weights' - each performed by extra workgroups of this launch (dim 64) or a launch of its own right after. */
struct pit_block_weights_job;
int pit_encoder_fwd(const pit_slab_plan* plan, const float* mesh_in, int space_dim, int coord_dims,
                    const float* values, long ld_values, long values_bstride, int value_dim, int batch,
                    int n_head, int dim, const float* head, int head_is_scale,
                    const float* w1, const float* b1, const float* w2, const float* b2,
                    float* x, float* z1, float* h, float* z2, float* y, long ldy, float* rowstat, float* scale_out,
                    float* clear_buf, long clear_n, const struct pit_block_weights_job* weights,
                    const pit_decoder_weights_job* dec_weights, void* stream);
/* pit.encoder backward: d_y (batch*n_out, dim) rows ld_dy apart -> scratch (dZ1 | dZ2: the layout of pit_mlp_bwd_data) and the
 * down-projection's d(scale) accumulators (required).  The inputs get no gradient (data). */
int pit_encoder_bwd(const pit_slab_plan* plan, const float* mesh_in, int space_dim, int coord_dims,
                    const float* values, long ld_values, long values_bstride, int value_dim, int batch,
                    int n_head, int dim, const float* scale, const float* rowstat,
                    const float* w1, const float* w2, const float* z1, const float* z2,
                    const float* d_y, long ld_dy, float* scratch, double* dscale, void* stream);

/* ---- Batch-free self-attention on PRECOMPUTED weights, large regime (round 4; pit.py:133-144 with locality 1.0) --------
 * The large-regime attention kernels re-formed exp(-c m) in every workgroup (posatt_rows_tiles / posatt_cols_tiles: the weight
 * phase and the MFMA phase of a workgroup do not overlap, 47-51 % MFMA busy).  With the weights of pit_block_weights in
 * memory (n_pts <= 2048) the weight phase is a coalesced copy requested one pass ahead:
 *   pit_posatt_pre_fwd   out[b, n, out_col0 + h*dim + d] = (1/rowsum_h[n]) sum_j e_h[n][j] values[b, j, d]  (e symmetric)
 *   pit_posatt_pre_bwd   d_values[b, j, :] = (add_residual ? d_out[b, j, 0:dim] : 0) + sum_h sum_n (e_h[n][j]/rowsum_h[n]) d_out[b, n, head h]
 *                        and, with workspace != NULL, the layer's d(scale) partial sums ADDED to workspace (PIT_HEAD_DEFER
 *                        convention: drain with pit_posatt_dhead_finish) from q = e (m - mbar)/rowsum.
 * e / q: this layer's (n_head, n_pts, n_pts) slices, rowstat its (n_head, n_pts, 4) slice of pit_block_weights' outputs.
 * pit_posatt_pre_supported: 1 when the shape is in the regime these launches cover (else use pit_posatt_fwd / _bwd).
 * Both entries return PIT_ERR_UNSUPPORTED, before any launch and writing nothing, for a shape outside it: n_pts no multiple of 4,
 * n_pts > 2048, or a (n_pts, n_head, batch * dim) that the large-regime (tiles) kernels do not take. */
int pit_posatt_pre_supported(int n_pts, int n_head, int dim, int batch);
int pit_posatt_pre_fwd(const float* e, const float* rowstat, int n_pts, int n_head, int dim, int batch,
                       const float* values, long ld_values, long values_bstride,
                       float* out, long ld_out, long out_bstride, int out_col0, int copy_inputs, int math_mode, void* stream);
int pit_posatt_pre_bwd(const float* e, const float* q, const float* rowstat, int n_pts, int n_head, int dim, int batch,
                       const float* values, long ld_values, long values_bstride,
                       const float* d_out, long ld_dout, long dout_bstride, int out_col0,
                       float* d_values, long ld_dvalues, long dvalues_bstride, int add_residual,
                       double* workspace, int math_mode, void* stream);

/* ---- Dense self-attention of the processor on bf16 MFMA (round 6; csrc/pit_satt.hip; bf16 math mode) ---------------------------
 * posatt.forward (pit.py:37-57) with locality 1.0 on one mesh (per-sample or batch-free): 1-2 heads, dim 128 / 256, 64..2048 points.
 *   pit_satt_fwd  out[b, n, out_col0 + h*dim + d] = sum_j softmax_j(-c_h m[n, j]) values[b, j, d]; copy_inputs: out[b, n, 0:dim] = values.
 *                 x16: batch*n_pts*dim bf16 (the rounded values; keep it for the backward); rowstat (mesh_batch, n_head, n_pts, 4) =
 *                 {-, 0, 1/rowsum, mbar}, scale_out (n_head) = c, as pit_posatt_fwd.
 *   pit_satt_bwd  d_values[b, j, :] = (add_residual ? d_out[b, j, 0:dim] : 0) + sum_h sum_n P_h[n, j] d_out[b, n, out_col0 + h*dim + :] (NULL: not
 *                 needed); the layer's d(scale) accumulators (PIT_HEAD_DEFER convention; NULL: not needed).  scale = the forward's c;
 *                 g16: scratch of batch*n_head*n_pts*dim bf16.
 *   x16_ready / g16_ready: the caller's x16 / g16 already hold bf16(values) / bf16(d_out_h / rowsum_h) - written by the producing
 *                 pit_mlp_chain_fwd (y16) / pit_mlp_chain_bwd (g16): no prep launch (x16_ready needs copy_inputs = 0).
 *   rider (pit_satt_bwd, optional): the postponed weight-gradient reductions of the MLP whose backward produced d_out (pit_posatt_bwd's
 *                 convention): carried as extra workgroups of the one backward launch, or run as pit_mlp_bwd_params would.
 *   e_tiles (optional, NULL: none): (mesh_batch, n_head, pit_satt_tiles_elems(n_pts)) bf16 - the forward leaves its rounded weights there
 *                 in MFMA A-fragment order and pit_satt_bwd's d(values) (the same, symmetric, matrix) reads them instead of forming
 *                 every weight again.
 * Weights, row sums and the d(scale) reduction are fp32 / fp64; the MFMA operands are bf16 (v_mfma_f32_16x16x32_bf16). */
int pit_satt_supported(int n_pts, int n_head, int dim, int batch, int mesh_batch);
int pit_satt_fwd(const float* mesh, int mesh_batch, int n_pts, int space_dim, int metric, float period,
                 const float* values, long ld_values, long values_bstride, int batch, int dim,
                 const float* head, int n_head, int head_is_scale, unsigned short* x16,
                 float* out, long ld_out, long out_bstride, int out_col0, int copy_inputs,
                 float* rowstat, float* scale_out, unsigned short* e_tiles, int x16_ready, void* stream);
int pit_satt_bwd(const float* mesh, int mesh_batch, int n_pts, int space_dim, int metric, float period,
                 int batch, int dim, const float* scale, int n_head, const float* rowstat,
                 const unsigned short* x16, unsigned short* g16,
                 const float* d_out, long ld_dout, long dout_bstride, int out_col0,
                 float* d_values, long ld_dvalues, long dvalues_bstride, int add_residual, double* dscale,
                 const unsigned short* e_tiles, int g16_ready, const pit_mlp_params_job* rider, void* stream);
long pit_satt_tiles_elems(int n_pts);

/* kaiming_mlp.forward (pit.py:21-26): y = W2 * gelu_erf(W1 x + b1) + b2, optionally
 * followed by the trailing gelu of pit.py:111,121 (out_gelu=1).
 *   x (rows, n0) rows ldx apart; w1 (n1,n0), b1 (n1), w2 (n2,n1), b2 (n2) contiguous;
 *   z1 (rows,n1) and h (rows,n1) are saved for the backward (pre-activation and
 *   gelu(z1)); z2 (rows,n2) is the pre-activation of the trailing gelu (out_gelu=1,
 *   else may be NULL); y (rows, n2) rows ldy apart. */
int pit_mlp_fwd(const float* x, long ldx, int rows, int n0, int n1, int n2,
                const float* w1, const float* b1, const float* w2, const float* b2, int out_gelu,
                float* z1, float* h, float* z2, float* y, long ldy, int math_mode, void* stream);

/* One-launch kaiming_mlp + gelu chains of the bf16 math mode for hid 128 / 256 on a few thousand rows (round 6; csrc/pit_chain.hip):
 * pit_mlp_fwd(..., out_gelu = 1) / pit_mlp_bwd_data as ONE launch each on 32-row slabs, the weights streamed through LDS as bf16
 * panels.  w1_bf16 (n1, n0) / w2_bf16 (n1, n1): row-major bf16 copies of the weights (pit_cast_bf16_multi); n2 == n1 in {128, 256},
 * n0 a multiple of n1 (the processor's (1 + H) hid), <= 1024.  z1 / h / z2 (rows, n1) fp32 as pit_mlp_fwd saves them; y rows ldy apart.
 * Backward: scratch = dZ1 | dZ2 (rows*n1 floats each: what pit_mlp_bwd_params reads), d_x (rows, n0) rows ld_dx apart or NULL.
 * gelu / gelu' are the polynomial CDF of the bf16 mode (pit_thin_tail_*). */
int pit_mlp_chain_supported(int rows, int n0, int n1, int n2);
int pit_mlp_chain_fwd(const float* x, long ldx, int rows, int n0, int n1, const unsigned short* w1_bf16, const float* b1,
                      const unsigned short* w2_bf16, const float* b2, float* z1, float* h, float* z2, float* y, long ldy,
                      unsigned short* y16 /* optional: bf16(y), (rows, n1) - the x16 of the next layer's pit_satt_fwd */, void* stream);
int pit_mlp_chain_bwd(int rows, int n0, int n1, const unsigned short* w1_bf16, const unsigned short* w2_bf16,
                      const float* z1, const float* z2, const float* d_y, long ld_dy, float* d_x, long ld_dx, float* scratch,
                      unsigned short* g16 /* optional: the g16 of the producing layer's pit_satt_bwd: bf16(d_x[:, (1+h) n1 + :] / rowsum_h), (rows / pts, n0 / n1 - 1, pts, n1) */,
                      const float* rowstat /* that layer's */, int pts, int mesh_batch, void* stream);
/* dst[i] = bf16(src[i]) (RNE) for n <= 32 tensors of count[i] floats (multiples of 4; 16-byte aligned sources): one launch. */
int pit_cast_bf16_multi(int n, const float* const* src, unsigned short* const* dst, const long* count, void* stream);

/* Backward of pit_mlp_fwd.  d_y (rows,n2) rows ld_dy apart (ld_dy == n2 when out_gelu).
 * d_x (rows,n0) rows ld_dx apart (NULL = not needed).  d_w1,d_b1,d_w2,d_b2 receive the
 * parameter gradients through fp32 atomics over row slabs: accumulate=0 zeroes them first
 * (plain gradient), accumulate=1 adds into their current contents (e.g. the parameters'
 * .grad inside a flat gradient buffer - no memset, no separate add).
 * scratch: rows*(n1+n2) floats. */
int pit_mlp_bwd(const float* x, long ldx, int rows, int n0, int n1, int n2,
                const float* w1, const float* w2, const float* z1, const float* h, const float* z2,
                int out_gelu, const float* d_y, long ld_dy,
                float* d_x, long ld_dx, float* d_w1, float* d_b1, float* d_w2, float* d_b2,
                int accumulate, float* scratch, int math_mode, void* stream);

/* The two halves of pit_mlp_bwd as separate entry points, so a caller can put the
 * parameter-gradient GEMMs (which nothing downstream in the backward pass depends on) on a
 * second stream: _data computes dZ1 (and dZ2 when out_gelu) into scratch and d_x; _params
 * consumes scratch and must be ordered after _data (event / same stream). */
int pit_mlp_bwd_data(int rows, int n0, int n1, int n2, const float* w1, const float* w2,
                     const float* z1, const float* z2, int out_gelu, const float* d_y, long ld_dy,
                     float* d_x, long ld_dx, float* scratch, int math_mode, void* stream);
int pit_mlp_bwd_params(const float* x, long ldx, int rows, int n0, int n1, int n2, const float* h,
                       int out_gelu, const float* d_y, long ld_dy,
                       float* d_w1, float* d_b1, float* d_w2, float* d_b2,
                       int accumulate, const float* scratch, int math_mode, void* stream);
/* 1 if postponing pit_mlp_bwd_params of this shape and handing it to the next pit_posatt_bwd as `rider` costs
 * nothing when the attention call cannot merge it (i.e. pit_mlp_bwd would have issued _data and _params as
 * separate launches anyway), else 0 (pit_mlp_bwd merges d_x with the reductions: keep the single call). */
int pit_mlp_bwd_params_deferrable(int rows, int n0, int n1, int n2, int out_gelu, long ld_dy);

/* RelLpNorm (utils.py:80-98): loss = sum_b mean_c ||true - pred'||_p / ||true||_p with norms
 * over the point axis of (batch, npts, nch) contiguous tensors, pred' = pred*scale + shift when
 * the optional per-pixel (npts, nch) affine of PixelWiseNormalization.denormalize
 * (utils.py:25-34, train_darcy.py:129) is given (both NULL = identity).
 * norms (batch, nch, 2) = {||true-pred'||_p, ||true||_p} is saved for the backward; loss is one
 * float.  workspace: PIT_REL_LP_WS_FLOATS(batch, nch) floats, 16-byte aligned (loss accumulator + arrival
 * counter, and per (sample, channel) two fp64 partial sums + a counter: a series is split over several
 * workgroups), zero before the first call and left zero by every call.  grad_loss: device pointer to the upstream scalar (NULL = 1).
 * The backward writes d loss/d pred and/or d loss/d true (either may be NULL): the scripts pass
 * the model output as `pred` (train_darcy.py:130) or as `true` (train_vorticity.py:124). */
#define PIT_REL_LP_WS_FLOATS(batch, nch) (4 + 5 * (batch) * (nch))
int pit_rel_lp_loss_fwd(const float* tru, const float* pred, const float* pred_scale,
                        const float* pred_shift, int batch, int npts, int nch, int p,
                        float* norms, float* loss, float* workspace, void* stream);
int pit_rel_lp_loss_bwd(const float* tru, const float* pred, const float* pred_scale,
                        const float* pred_shift, int batch, int npts, int nch, int p,
                        const float* norms, const float* grad_loss, float* d_pred, float* d_true, void* stream);

/* pit_rel_lp_loss_fwd that ALSO writes, in the same launch, the gradients for an upstream gradient
 * of 1 - d_pred_unit and/or d_true_unit, (batch,npts,nch), NULL = not wanted - and clears clear_n
 * floats at clear_buf (e.g. the flat gradient accumulators of the step whose backward pass follows;
 * clear_n = 0: nothing).  A training step seeded with d loss = 1 then needs neither the loss
 * backward launch nor a memset. */
int pit_rel_lp_loss_fwd_grad(const float* tru, const float* pred, const float* pred_scale,
                             const float* pred_shift, int batch, int npts, int nch, int p,
                             float* norms, float* loss, float* workspace, float* d_pred_unit,
                             float* d_true_unit, float* clear_buf, long clear_n, void* stream);

/* ABI 29, reproducible mode: pit_rel_lp_loss_fwd_grad (same arguments, same workspace, d_pred_unit / d_true_unit / clear_buf
 * may be NULL) with every sum in an order that depends on the sizes only: a series is never split over workgroups (one
 * 1024-thread workgroup where the series fits it, else one 256-thread workgroup), and the terms of the (sample, channel)
 * pairs are added in index order by the workgroup that arrives last.  Same call, same bits; no environment switch is read. */
int pit_rel_lp_loss_fwd_grad_ordered(const float* tru, const float* pred, const float* pred_scale,
                                     const float* pred_shift, int batch, int npts, int nch, int p,
                                     float* norms, float* loss, float* workspace, float* d_pred_unit,
                                     float* d_true_unit, float* clear_buf, long clear_n, void* stream);

/* RelMaxNorm (utils.py:59-77), the evaluation metric of train_burgers.py:80 / train_sod.py:84 /
 * train_elasticity.py:118 / train_naca.py:132:  out = sum_b mean_c max_l|true - pred| / max_l|true|
 * over (batch, npts, nch) contiguous tensors.  Forward only (the scripts never differentiate it).
 * workspace: 2 doubles (accumulator + arrival counter), zero before the first call, left zero. */
int pit_rel_max_norm(const float* tru, const float* pred, int batch, int npts, int nch, float* out,
                     double* workspace, void* stream);

/* nn.InstanceNorm1d over the point axis as train_vorticity.py:43,56,59 applies it
 * (norm(x.permute(0,2,1)).permute(0,2,1); no affine, no running statistics, biased variance),
 * computed directly on the (batch, points, channels) layout:
 *   y[b,l,c] = (x[b,l,c] - mean_l x[b,:,c]) * rstd[b,c],  rstd = 1/sqrt(var_l + eps).
 * x rows ldx apart, samples x_bstride apart; y (batch,npts,nch) and rstd (batch,nch) contiguous. */
int pit_instance_norm_fwd(const float* x, long ldx, long x_bstride, int batch, int npts, int nch, float eps,
                          float* y, float* rstd, void* stream);
/* d_x = rstd * (d_y - mean_l d_y - y * mean_l(d_y * y)); all (batch,npts,nch) contiguous. */
int pit_instance_norm_bwd(const float* d_y, const float* y, const float* rstd, int batch, int npts, int nch,
                          float* d_x, void* stream);

/* torch.optim.Adam step (no amsgrad) over FLAT fp32 buffers of n elements, learning rate following
 * CosineAnnealingLR(T_max=cosine_t_max, eta_min) when cosine_t_max > 0 (train_darcy.py:115-116),
 * else constant lr0.  `step` (device int64, starts at 0) is incremented here; `scalars` is 4
 * floats of device scratch, ZERO before the first call (slot 3 is an arrival ticket; slots 0-2
 * receive lr_t and the bias corrections of the step taken).  With zero_grads=1 the gradients are
 * cleared as they are consumed (the next backward pass accumulates into zeros: no memset launch).
 * One launch, no host sync: replayable from a hipGraph. */
int pit_adam_step(float* params, float* grads, float* exp_avg, float* exp_avg_sq, long n,
                  long long* step, float lr0, float eta_min, int cosine_t_max, float beta1, float beta2,
                  float eps, float weight_decay, int zero_grads, float* scalars, void* stream);

/* ---- Ragged batches of per-sample clouds (ABI 27; csrc/pit_ragged.hip) --------------------------------------------------------
 * Padded tensors plus per-sample lengths ON THE DEVICE: sample s of a (mesh_batch, n, ...) tensor holds len[s] real points
 * followed by padding, and comes out as pit.py:46-57 computes it for that cloud ALONE (a batch of one with len[s] points): its own
 * quantile rank floor(fl32(q) * fl32(len_in[s] - 1)), its own kept sets, its own softmax.  len_out / len_in: mesh_batch int32 each
 * in device memory, read by the kernels (no host synchronisation: one captured hipGraph serves every mix of sizes up to the padded
 * n_out / n_in); self attention passes one buffer for both.  Precondition 1 <= len[s] <= padded width; the kernels clamp into that
 * range, so a bad length cannot address outside the buffers.  Per-sample meshes only (batch = mesh_batch), Euclidean metric,
 * 1 <= space_dim <= 3 (PIT_ERR_UNSUPPORTED beyond), PIT_MATH_FP32 only (PIT_ERR_UNSUPPORTED otherwise).  The rules:
 *   - keys j >= len_in[s] are never read (coordinates, value rows): the padding may hold anything, NaN included;
 *   - rows i >= len_out[s]: `out` is written as ZERO in every head column (with copy_inputs the copied columns are copied as they
 *     are), their stats / rowstat are zeros, their d_out is never read;
 *   - d_values of keys j >= len_in[s] is written as zero, residual included.
 * Every sum has a fixed order except d(scale)'s fp64 slots (see pit_posatt_ragged_bwd).
 *
 * pit_plan_ragged_fwd: the selection statistics of pit_select_fwd over the first len_in[s] keys of every row: stats
 *   (3*mesh_batch*n_out floats, the layout of pit_select_fwd), rank k_s and interpolation weight w_s formed in the kernel with
 *   the fp32 operations of torch.quantile (fp32 product, floor, fp32 difference); rank_w (mesh_batch floats) receives w_s.
 *   locality: the quantile q in [0, 1]; need_kth = 0: only the row minimum (nothing masked).
 *   nbr_idx != NULL (need_kth = 1): also the candidate lists of pit_neighbors_fwd over the first len_in[s] keys - nbr_idx
 *   (rows, cap), nbr_cnt (rows) the TRUE count; `cap` is the caller's, chosen from the padded width, so it does not depend on the
 *   lengths; a row with count > cap is truncated and its consumers scan all keys of the sample (the existing convention); rows
 *   i >= len_out[s] get count 0.  The transposed lists come from pit_lists_transpose on these lists: padded rows appear in no
 *   range and padded keys have empty ranges. */
int pit_plan_ragged_fwd(const float* mesh_out, const float* mesh_in, int mesh_batch, int n_out, int n_in,
                        int space_dim, const int* len_out, const int* len_in, float locality, int need_kth,
                        float* stats, float* rank_w, int cap, int* nbr_idx, int* nbr_cnt, void* stream);
/* pit_posatt_fwd on a ragged batch.  stats / rank_w from pit_plan_ragged_fwd (rank_w may be NULL when masked = 0); the other
 * arguments as in pit_posatt_fwd (batch = mesh_batch; no coordinate channels).  nbr_idx / nbr_cnt / nbr_cap: the candidate lists
 * of pit_plan_ragged_fwd (masked layers; NULL = the dense kernel): one wave per row walks its list, or all keys when it overflowed. */
int pit_posatt_ragged_fwd(const float* mesh_out, const float* mesh_in, int mesh_batch, int n_out, int n_in,
                          int space_dim, const int* len_out, const int* len_in,
                          const float* values, int dim, long ld_values, long values_bstride,
                          const float* head, int n_head, int head_is_scale,
                          const float* stats, const float* rank_w, int masked,
                          float* out, long ld_out, long out_bstride, int out_col0, int copy_inputs,
                          float* rowstat, float* scale_out,
                          const int* nbr_idx, const int* nbr_cnt, int nbr_cap, int math_mode, void* stream);
/* pit_posatt_bwd on a ragged batch: d_values (NULL = not needed), d_head (NULL = not needed), scale, rowstat, accumulate_head
 * (PIT_HEAD_ACCUMULATE / PIT_HEAD_DEFER) and workspace (n_head*PIT_DSCALE_SLOTS doubles, zero on entry, left zero unless
 * deferred) as in pit_posatt_bwd.  With lists, d(scale) walks them by row; d(values) walks rev_ptr / rev_row (pit_lists_transpose)
 * by key, rows in ascending order, then the overflowed rows - no atomics; rev_ptr = NULL: the dense d(values) kernel.
 * d(scale) partial sums meet in the workspace's fp64 slots through atomics, as in pit_posatt_bwd: the order inside a slot is
 * not fixed, and the fp32 result is the same from run to run only in so far as fp64 rounding differences vanish in the final
 * rounding.  Everything else has a fixed summation order. */
int pit_posatt_ragged_bwd(const float* mesh_out, const float* mesh_in, int mesh_batch, int n_out, int n_in,
                          int space_dim, const int* len_out, const int* len_in,
                          const float* values, int dim, long ld_values, long values_bstride,
                          const float* head, int n_head, int head_is_scale, const float* scale,
                          const float* rowstat, int masked,
                          const float* d_out, long ld_dout, long dout_bstride, int out_col0,
                          float* d_values, long ld_dvalues, long dvalues_bstride, int add_residual,
                          float* d_head, int accumulate_head, double* workspace,
                          const int* nbr_idx, const int* nbr_cnt, int nbr_cap, const int* rev_ptr, const int* rev_row,
                          int math_mode, void* stream);
/* ---- A mesh shared by the whole batch against per-sample clouds (ABI 28; csrc/pit_ragged.hip) -------------------------------
 * The three entries above with, for each mesh, a sample stride in POINTS and a length pointer that may be NULL:
 *   out_stride / in_stride: points between two samples' meshes; 0 = ONE (n, space_dim) mesh shared by every sample, read in
 *     place (no expanded copy); otherwise >= n_out / n_in (PIT_ERR_SIZE for anything between);
 *   len_out / len_in: NULL = every sample has the full width n_out / n_in.
 * Sample s comes out as pit.py:46-57 computes it for (shared mesh, cloud_s) as a batch of one - the broadcast of a (n, s) mesh
 * against a (b, n', s) mesh in pit.py:47-48 - and, with a length on the cloud side, for the cloud's first len[s] points alone:
 * the rank floor(fl32(q) * fl32(len_in[s] - 1)) is per sample when the keys are the cloud and that of the full width when the
 * keys are the shared mesh; row tiles end at len_out[s] only when the rows are the cloud.  Only coordinates are shared: stats
 * (3*mesh_batch*n_out), rank_w, nbr_idx / nbr_cnt (choose cap from the full / padded n_in), the transposed lists of
 * pit_lists_transpose (call it with mesh_batch samples as before), rowstat, values, out and d_values are all PER SAMPLE - the
 * d(values) of a shared-key layer has mesh_batch * n_in rows.  The zero rules of ABI 27 hold on the side that has lengths.
 * With strides n_out / n_in and both lengths given these are pit_plan_ragged_fwd / pit_posatt_ragged_fwd / _bwd bit for bit
 * (one implementation); those three keep refusing NULL lengths. */
int pit_plan_ragged_strided_fwd(const float* mesh_out, const float* mesh_in, int mesh_batch, int n_out, int n_in,
                                int space_dim, long out_stride, long in_stride, const int* len_out, const int* len_in,
                                float locality, int need_kth, float* stats, float* rank_w, int cap, int* nbr_idx,
                                int* nbr_cnt, void* stream);
int pit_posatt_ragged_strided_fwd(const float* mesh_out, const float* mesh_in, int mesh_batch, int n_out, int n_in,
                                  int space_dim, long out_stride, long in_stride, const int* len_out, const int* len_in,
                                  const float* values, int dim, long ld_values, long values_bstride,
                                  const float* head, int n_head, int head_is_scale,
                                  const float* stats, const float* rank_w, int masked,
                                  float* out, long ld_out, long out_bstride, int out_col0, int copy_inputs,
                                  float* rowstat, float* scale_out,
                                  const int* nbr_idx, const int* nbr_cnt, int nbr_cap, int math_mode, void* stream);
int pit_posatt_ragged_strided_bwd(const float* mesh_out, const float* mesh_in, int mesh_batch, int n_out, int n_in,
                                  int space_dim, long out_stride, long in_stride, const int* len_out, const int* len_in,
                                  const float* values, int dim, long ld_values, long values_bstride,
                                  const float* head, int n_head, int head_is_scale, const float* scale,
                                  const float* rowstat, int masked,
                                  const float* d_out, long ld_dout, long dout_bstride, int out_col0,
                                  float* d_values, long ld_dvalues, long dvalues_bstride, int add_residual,
                                  float* d_head, int accumulate_head, double* workspace,
                                  const int* nbr_idx, const int* nbr_cnt, int nbr_cap, const int* rev_ptr, const int* rev_row,
                                  int math_mode, void* stream);

/* RelLpNorm (utils.py:86-98) of every sample TRUNCATED to its first len[s] points: true / pred (batch, npts, nch) contiguous,
 * norms (batch, nch, 2) = {||true - pred||_p, ||true||_p}, *loss = sum_s mean_c of their ratio.  Padded points are skipped (not
 * multiplied by zero).  The backward writes d_pred (batch, npts, nch) = *gloss (NULL: 1) times the gradient, zero on padded points. */
int pit_rel_lp_loss_ragged_fwd(const float* tru, const float* pred, const int* len, int batch, int npts, int nch, int p,
                               float* norms, float* loss, void* stream);
int pit_rel_lp_loss_ragged_bwd(const float* tru, const float* pred, const int* len, int batch, int npts, int nch, int p,
                               const float* norms, const float* gloss, float* d_pred, void* stream);

/* pit_mlp_bwd_params with a FIXED summation order (ABI 27): the rows are cut into at most 16 slabs, every slab is contracted into
 * partial matrices of its own (no atomics) and a second launch adds them slab by slab - the same bits on every run, where
 * pit_mlp_bwd_params adds its slabs with fp32 atomics.  fp32 tensors only; arguments as pit_mlp_bwd_params, plus workspace:
 * pit_mlp_bwd_params_ordered_workspace(...) bytes, no initial contents needed.  The ragged path uses it so that "padding never
 * enters the arithmetic" can be stated bit for bit; plain fp32 FMAs, about the cost of the data path it follows. */
long pit_mlp_bwd_params_ordered_workspace(int rows, int n0, int n1, int n2);
int pit_mlp_bwd_params_ordered(const float* x, long ldx, int rows, int n0, int n1, int n2, const float* h,
                               int out_gelu, const float* d_y, long ld_dy,
                               float* d_w1, float* d_b1, float* d_w2, float* d_b2,
                               int accumulate, const float* scratch, float* workspace, void* stream);

/* pit_mlp_bwd_params_ordered on fp32 MFMA (ABI 29; csrc/pit_dw_ordered.hip): the weight-gradient reductions of the reproducible
 * mode (ops.set_reproducible).  Arguments as pit_mlp_bwd_params_ordered.  ONE contraction launch for both reductions - a
 * workgroup contracts one row slab into one 64 x 64 tile of that slab's own partial matrices (v_mfma_f32_32x32x2_f32, plain
 * stores, bias gradients as fixed-order column sums in the same launch) - and one finishing launch that adds the partials in slab
 * order and writes (accumulate: adds to) d_w1 (n1, n0), d_b1 (n1), d_w2 (n2, n1), d_b2 (n2).  The slabs are a pure function of
 * (rows, n0, n1, n2): at most 64 equal slabs of a multiple of 32 rows, enough for about 512 workgroups; never of the device, the
 * environment or an address.  Same inputs, same bits - but not the bits of pit_mlp_bwd_params_ordered, whose partition differs.
 * fp32 tensors; ldx >= n0, ld_dy >= n2 (PIT_ERR_SIZE otherwise, and for a slab beyond a 32-bit byte offset); any alignment.
 * workspace: pit_mlp_bwd_params_ordered_mfma_workspace(...) bytes (0 for invalid sizes), no initial contents needed. */
long pit_mlp_bwd_params_ordered_mfma_workspace(int rows, int n0, int n1, int n2);
int pit_mlp_bwd_params_ordered_mfma(const float* x, long ldx, int rows, int n0, int n1, int n2, const float* h,
                                    int out_gelu, const float* d_y, long ld_dy,
                                    float* d_w1, float* d_b1, float* d_w2, float* d_b2,
                                    int accumulate, const float* scratch, float* workspace, void* stream);

/* Reproducible mode, candidate-list layers (ABI 29).
 * pit_lists_sort_ranges: `sorted` (mesh_batch, rev_stride) <- rev_row with every key's range [rev_ptr[j], rev_ptr[j+1]) in
 * ascending row order, the -1 slots of overflowed rows last; slots outside every range are not written (hand in a copy of
 * rev_row).  Out of place (sorted != rev_row), rev_stride = n_out * cap as in pit_lists_transpose; mesh_batch <= 65535.
 * d(values) of the list kernels is summed in list order, and pit_lists_transpose / pit_plan_fwd fill a range in whatever order
 * their atomics land: with the sorted copy as pit_posatt_bwd's rev_row the sum has ONE order.
 * pit_posatt_overflow_dv_ordered: d_values += the terms of the rows with nbr_cnt > nbr_cap, one wave per key, rows ascending, no
 * atomics; call it after pit_posatt_bwd(..., nbr_complete = 1, ...) on the same stream (that call's own overflow pass adds with
 * fp32 atomics and is skipped by the flag).  Nothing overflowed: every wave leaves after reading the counts.  Arguments as the
 * same-named ones of pit_posatt_bwd (dim includes coord_dims, d_values holds the dim - coord_dims others); fp32 d_out only;
 * 1 <= space_dim <= PIT_MAX_SPACE_DIM, every metric. */
int pit_lists_sort_ranges(const int* rev_ptr, const int* rev_row, int mesh_batch, int n_in, long rev_stride,
                          int* sorted, void* stream);
int pit_posatt_overflow_dv_ordered(const float* mesh_out, const float* mesh_in, int mesh_batch, int n_out, int n_in,
                                   int space_dim, int metric, float period, int batch, int dim,
                                   const float* head, int n_head, int head_is_scale, const float* scale,
                                   const float* rowstat, const float* d_out, long ld_dout, long dout_bstride, int out_col0,
                                   float* d_values, long ld_dvalues, long dvalues_bstride,
                                   const int* nbr_cnt, int nbr_cap, int coord_dims, void* stream);

/* ---- Position attention on caller-supplied squared distances (ABI 31; csrc/pit_distmat.hip) ---------------------------
 * The reference's extension point for another metric is overriding posatt.dist2att (pit.py:42-43,68-69); the layer itself is
 * pit.py:48-57 applied to whatever matrix the metric produced.  These entries take that matrix instead of two meshes:
 *   m        fp32 squared distances, (n_out, n_in) shared by the whole batch (m_bstride = 0) or one matrix per sample, samples
 *            m_bstride floats apart (>= (n_out-1)*ld_m + n_in); rows ld_m floats apart (>= n_in).
 * Precondition: m finite and >= 0 - not checked (a check would synchronise); the kernels form no index from the values of m, so
 * nothing is addressed out of bounds whatever it holds.  PIT_MATH_FP32 only (PIT_ERR_UNSUPPORTED otherwise); a sample's rows of m,
 * values and d_out must each fit a 32-bit byte offset (PIT_ERR_UNSUPPORTED beyond).  No host synchronisation, no allocation.
 * Every sum except d(scale)'s fp64 slots has a fixed order and there are no other atomics: same input, same bits.
 *
 * pit_distmat_select_fwd - the sort inside torch.quantile (pit.py:49) for rows that are GIVEN: for each of the mesh_batch*n_out rows
 *   stats[0][row] = m_(k), stats[1][row] = m_(k+1) (k+1 clipped to n_in-1), stats[2][row] = min_j m, the layout of pit_select_fwd;
 *   rank_k as there; need_kth = 0: only the minimum.  Exact: MSB-first bitwise search over the row's bit patterns; a row of up to
 *   2048 keys is staged in LDS once and searched there, a longer row is streamed.  mesh_batch = number of matrices (1: m_bstride unused).
 * pit_distmat_fwd - pit.py:48-57 on m (posatt.forward :37-44 with copy_inputs, posatt_cross.forward :63-71): out, rowstat
 *   ((m_bstride ? batch : 1), n_head, n_out, 4) = {T, S_min, 1/rowsum, mbar = sum_j P m} and scale_out; the other arguments as the
 *   same-named ones of pit_posatt_fwd.  The kept set is pit_posatt_fwd's: fl(c m_ij) <= T_i = quantile_lerp(fl(c m_(k)), fl(c m_(k+1)), rank_w).
 * pit_distmat_bwd - the backward of pit_distmat_fwd, for what the reference leaves to autograd through pit.py:48-57.  With
 *   g_i = d_out[i, out_col0 + h*dim : +dim], gv_ij = g_i . values_j, a_i = sum_j P_ij gv_ij and s_ij = P_ij (gv_ij - a_i):
 *     d_values[j] = sum_h sum_i P_ij g_i (+ d_out[j, 0:dim] with add_residual)          NULL = not needed
 *     d c_h       = -sum_ij s_ij m_ij -> d_head through `workspace`, accumulate_head and  NULL = not needed
 *                   the finishing step exactly as in pit_posatt_bwd (PIT_HEAD_ACCUMULATE / PIT_HEAD_DEFER)
 *     d_m[i][j]   = -sum_h c_h s_ij, contiguous ((m_bstride ? batch : 1), n_out, n_in); for a   NULL = not needed
 *                   shared matrix summed over the samples in ascending order inside the workgroup that owns the tile
 *   out / ld_out / out_bstride: the forward's result (a_i = g_i . out_i) and a_workspace: pit_distmat_bwd_workspace(batch, n_out,
 *   n_head) bytes (the a_i, (batch, n_head, n_out), no initial contents) - both needed with d_m only.
 *   scale = the c written to scale_out by the forward (NULL = recompute from head).
 * The contractions (P V, P^T g and the gv tiles) run on v_mfma_f32_32x32x2_f32. */
int pit_distmat_select_fwd(const float* m, long ld_m, long m_bstride, int mesh_batch, int n_out, int n_in,
                           int rank_k, int need_kth, float* stats, void* stream);
int pit_distmat_fwd(const float* m, long ld_m, long m_bstride, int n_out, int n_in,
                    const float* values, int batch, int dim, long ld_values, long values_bstride,
                    const float* head, int n_head, int head_is_scale,
                    const float* stats, float rank_w, int masked,
                    float* out, long ld_out, long out_bstride, int out_col0, int copy_inputs,
                    float* rowstat, float* scale_out, int math_mode, void* stream);
long pit_distmat_bwd_workspace(int batch, int n_out, int n_head);
int pit_distmat_bwd(const float* m, long ld_m, long m_bstride, int n_out, int n_in,
                    const float* values, int batch, int dim, long ld_values, long values_bstride,
                    const float* head, int n_head, int head_is_scale, const float* scale,
                    const float* rowstat, int masked,
                    const float* d_out, long ld_dout, long dout_bstride, int out_col0,
                    float* d_values, long ld_dvalues, long dvalues_bstride, int add_residual,
                    float* d_head, int accumulate_head, double* workspace,
                    float* d_m, const float* out, long ld_out, long out_bstride, float* a_workspace,
                    int math_mode, void* stream);

/* ---- The same layer on CANDIDATE LISTS of caller-supplied squared distances (additions to ABI 31; csrc/pit_distlist.hip) --------
 * For problems whose (n_out, n_in) matrix cannot be formed: per row a list of `cap` slots (key, squared distance), O(n_out * cap)
 * memory, any n_in.  A library built from this header defines PIT_HAS_DISTLIST; PIT_ABI_VERSION is unchanged (nothing that
 * existed changed).
 *   idx / sqd  int32 keys and fp32 squared distances of the same layout: (n_out, cap) shared by the whole batch (bstride = 0) or
 *              one pair of lists per sample, samples bstride elements apart (>= (n_out-1)*ld + cap); rows ld elements apart
 *              (>= cap).  n_out * cap < 2^31.
 * A slot whose key lies outside [0, n_in) is PADDING: its sqd is never used (it may hold NaN), its key is never dereferenced and
 * its d_sqd is 0 - so no key can address out of bounds, without a check that would synchronise.  Preconditions, not checked:
 * valid sqd finite and >= 0; no key twice in a row (the result is wrong then, every access stays in bounds); for a masked layer
 * at least rank_k + 2 valid slots per row.  The result is pit.py:48-57 on the dense matrix that holds the listed values and, at
 * every unlisted pair, a value large enough to be masked and to weigh 0: rank_k / rank_w come from n_in (ops.quantile_rank), the
 * order statistics from the valid listed values; slot t is kept iff valid and fl(c sqd) <= T (ties all kept); masked = 0: every
 * valid slot is kept.  A row without a valid slot gives zero output, zero rowstat and zero gradients.
 * PIT_MATH_FP32 only (PIT_ERR_UNSUPPORTED otherwise); a sample's rows of values, out and d_out must each fit a 32-bit byte offset.
 * No host synchronisation, no allocation, capturable.  Every sum except d(scale)'s fp64 slots has a fixed order and there are no
 * other atomics: same input, same bits.  Value, d_out and out rows move in 16-byte pieces where dim, the leading dimensions, the
 * sample strides, out_col0 and the base addresses are all multiples of 4 floats, in 4-byte pieces otherwise.
 *
 * pit_distlist_select_fwd - stats[0..2][row] = {m_(k), m_(k+1) (k+1 clipped to the row's last valid rank), min} over the VALID
 *   slots of each of the mesh_batch*n_out rows, the layout of pit_select_fwd.  Exact: MSB-first bitwise search on the bit patterns,
 *   one wave per row with the row in registers; cap <= 2048 (PIT_ERR_UNSUPPORTED beyond).  need_kth = 0: only the minimum (the
 *   other two rows of stats receive it too).  A row without a valid slot: 0, 0, 0.
 * pit_distlist_fwd - out, rowstat ((bstride ? batch : 1), n_head, n_out, 4) = {T, S_min, 1/rowsum, mbar} and scale_out as
 *   pit_distmat_fwd writes them.  One wave per (sample, row), slots in list order.
 * pit_distlist_bwd - with g_i, gv, a_i = g_i . out_i and s = P (gv - a_i) as in pit_distmat_bwd:
 *     d_values[j]  = sum over the slots that list j, ascending in (row, slot), of sum_h P g_i (+ d_out[j, 0:dim] with
 *                    add_residual); a key nobody lists gets zeros (+ the residual).                        NULL = not needed
 *     d c_h        = -sum s sqd -> d_head through `workspace`, accumulate_head, scale and the finishing step as in pit_distmat_bwd
 *     d_sqd[i][t]  = -sum_h c_h s, contiguous ((bstride ? batch : 1), n_out, cap), 0 at padding and at slots not kept; for shared
 *                    lists summed over the samples in ascending order inside the wave that owns the row; needs `out`.  NULL = not needed
 *   The transposed index (needed with d_values) is the caller's, per list set mb:
 *     rev_ptr    (mesh_batch, n_in + 1): key j is listed by the entries rev_ptr[mb][j] .. rev_ptr[mb][j+1] - 1 of rev_pos[mb]
 *     rev_pos    (mesh_batch, n_out * cap): flat positions row * cap + slot, ascending inside every key's range
 *     chunk_ptr  (mesh_batch, n_in + 1): a key whose range is longer than PIT_DISTLIST_CHUNK entries owns the chunk slots
 *                chunk_ptr[mb][j] .. chunk_ptr[mb][j+1] - 1, ceil(length / PIT_DISTLIST_CHUNK) of them; any other key owns none
 *     chunk_key  (mesh_batch, PIT_DISTLIST_CHUNK_SLOTS(n_out, cap)): the key that owns each chunk slot, n_in for a free slot
 *   Such a key is summed chunk by chunk by separate waves into dv_workspace (pit_distlist_bwd_workspace(batch, n_out, cap, dim)
 *   bytes, no initial contents) and its partial rows are added in chunk order.  Entries of these tables are clamped to their
 *   ranges before use. */
#define PIT_HAS_DISTLIST 1
#define PIT_DISTLIST_MAX_CAP 2048
#define PIT_DISTLIST_CHUNK 512
#define PIT_DISTLIST_CHUNK_SLOTS(n_out, cap) ((long)(n_out) * (long)(cap) / (PIT_DISTLIST_CHUNK / 2) + 1)
int pit_distlist_select_fwd(const int* idx, const float* sqd, long ld, long bstride, int cap, int mesh_batch, int n_out, int n_in,
                            int rank_k, int need_kth, float* stats, void* stream);
int pit_distlist_fwd(const int* idx, const float* sqd, long ld, long bstride, int cap, int n_out, int n_in,
                     const float* values, int batch, int dim, long ld_values, long values_bstride,
                     const float* head, int n_head, int head_is_scale,
                     const float* stats, float rank_w, int masked,
                     float* out, long ld_out, long out_bstride, int out_col0, int copy_inputs,
                     float* rowstat, float* scale_out, int math_mode, void* stream);
long pit_distlist_bwd_workspace(int batch, int n_out, int cap, int dim);
int pit_distlist_bwd(const int* idx, const float* sqd, long ld, long bstride, int cap, int n_out, int n_in,
                     const float* values, int batch, int dim, long ld_values, long values_bstride,
                     const float* head, int n_head, int head_is_scale, const float* scale,
                     const float* rowstat, int masked,
                     const float* d_out, long ld_dout, long dout_bstride, int out_col0,
                     float* d_values, long ld_dvalues, long dvalues_bstride, int add_residual,
                     float* d_head, int accumulate_head, double* workspace,
                     float* d_sqd, const float* out, long ld_out, long out_bstride,
                     const int* rev_ptr, const int* rev_pos, const int* chunk_ptr, const int* chunk_key, float* dv_workspace,
                     int math_mode, void* stream);

/* ---- Ragged batches on candidate lists (additions to ABI 31; csrc/pit_distlist.hip) ------------------------------------------------
 * The three list entries above for a padded batch whose sample s has len_out[s] rows and len_in[s] keys: int32 DEVICE arrays of
 * `batch` entries, read by the kernels and clamped into [1, n_out] / [1, n_in]; either may be NULL = the full width.  No host
 * synchronisation: one captured graph serves every mix of sizes.  Per-sample lists only (bstride != 0, or a batch of one:
 * PIT_ERR_SIZE otherwise).  A library built from this header defines PIT_HAS_DISTLIST_RAGGED; PIT_ABI_VERSION is unchanged
 * (nothing that existed changed: the entries above run the code and give the bits they did).
 * The result for sample s is what the entries above compute for that cloud alone - lists idx[s][0:len_out[s]], values
 * [0:len_in[s]], n_in = len_in[s]:
 *   - a slot is valid iff its key lies in [0, len_in[s]); keys in [len_in[s], n_in) are padding like any key outside [0, n_in):
 *     compared, never dereferenced, their sqd may hold anything;
 *   - the rank (k_s, w_s) comes from len_in[s] and `locality` on the device with the fp32 operations of ops.quantile_rank (the
 *     rule of pit_plan_ragged_fwd); pit_distlist_select_ragged_fwd writes w_s to rank_w[s] (mesh_batch floats), which
 *     pit_distlist_ragged_fwd reads.  The width check (rank_k <= cap - 1) uses the rank of the padded n_in, which bounds k_s;
 *   - a row i >= len_out[s]: stats 0, every head column of out 0 (copy_inputs: the input columns copied as they are), rowstat 0,
 *     d_sqd 0, no contribution to d_values or d_head; its list, its sqd and its d_out row are never read;
 *   - d_values of a key j >= len_in[s] is written as zero; value rows j >= len_in[s] are never read (they may hold NaN).
 * Precondition, not checked: a real row lists at least min(k_s + 2, len_in[s]) valid slots and no key twice.
 * The transposed index is the one of pit_distlist_bwd, built from the keys alone against the padded n_in - it does not depend on
 * the lengths, which filter where the slots are read (an entry whose row is >= len_out[s] weighs 0).  Order of d_values: a
 * key's entries ascend in row * cap + slot, so the entries of padded rows stand behind the real ones; the real entries take the
 * places of the same 64-entry groups and PIT_DISTLIST_CHUNK-entry chunks as in the cloud-alone run and skipped entries add +0:
 * for a key whose whole range fits one chunk the bits are the cloud-alone run's.  A longer range is summed chunk by chunk by
 * separate waves and added in chunk order; it is specified to a tolerance only.  Every other sum is per row and has the
 * cloud-alone order; d(scale) goes through the fp64 slots as above. */
#define PIT_HAS_DISTLIST_RAGGED 1
int pit_distlist_select_ragged_fwd(const int* idx, const float* sqd, long ld, long bstride, int cap, int mesh_batch, int n_out, int n_in,
                                   float locality, int need_kth, const int* len_out, const int* len_in, float* stats, float* rank_w,
                                   void* stream);
int pit_distlist_ragged_fwd(const int* idx, const float* sqd, long ld, long bstride, int cap, int n_out, int n_in,
                            const float* values, int batch, int dim, long ld_values, long values_bstride,
                            const float* head, int n_head, int head_is_scale,
                            const float* stats, const float* rank_w, int masked,
                            const int* len_out, const int* len_in,
                            float* out, long ld_out, long out_bstride, int out_col0, int copy_inputs,
                            float* rowstat, float* scale_out, int math_mode, void* stream);
int pit_distlist_ragged_bwd(const int* idx, const float* sqd, long ld, long bstride, int cap, int n_out, int n_in,
                            const float* values, int batch, int dim, long ld_values, long values_bstride,
                            const float* head, int n_head, int head_is_scale, const float* scale,
                            const float* rowstat, int masked,
                            const int* len_out, const int* len_in,
                            const float* d_out, long ld_dout, long dout_bstride, int out_col0,
                            float* d_values, long ld_dvalues, long dvalues_bstride, int add_residual,
                            float* d_head, int accumulate_head, double* workspace,
                            float* d_sqd, const float* out, long ld_out, long out_bstride,
                            const int* rev_ptr, const int* rev_pos, const int* chunk_ptr, const int* chunk_key, float* dv_workspace,
                            int math_mode, void* stream);

/* ---- A training step and the evaluation metric on ragged batches (additions to ABI 31; csrc/pit_ragged_step.hip) -----------------
 * utils.py:59-98 (RelMaxNorm, RelLpNorm) on every sample TRUNCATED to its first len[s] points, as engine.TrainStep and
 * utils.RelMaxNorm use them with lengths.  A library built from this header defines PIT_HAS_RAGGED_STEP; PIT_ABI_VERSION is
 * unchanged (nothing that existed changed).  true / pred (batch, npts, nch) contiguous fp32, len (batch) int32 on the device,
 * clamped into [1, npts] where it is read; padded points are never read (they may hold NaN).  No host synchronisation, no
 * allocation, capturable; every sum has a fixed order: same input, same bits.
 *
 * pit_rel_lp_loss_ragged_fwd_grad - ONE launch for what pit_rel_lp_loss_ragged_fwd, pit_rel_lp_loss_ragged_bwd(gloss = NULL) and a
 *   memset do in four:
 *     norms (batch, nch, 2) and *loss  exactly as pit_rel_lp_loss_ragged_fwd writes them (the same summation order, the same bits);
 *     d_pred_unit (batch, npts, nch)   the gradient for d loss = 1, as pit_rel_lp_loss_ragged_bwd writes it for gloss = NULL (the
 *                                      same bits), exact zeros on padded points.                              NULL = not wanted
 *     clear_buf                        clear_n floats are zeroed (the step's flat gradient accumulators; any 4-byte alignment);
 *                                      clear_n = 0: nothing is cleared
 *     workspace                        ONE unsigned word, the arrival ticket: zero before the first call, left zero by every call
 *                                      (calls that share it must be stream-ordered)
 *   A (sample, channel) series is never split over workgroups; the pairs' terms are added in index order by the workgroup that
 *   arrives last.  PIT_ERR_NULL for a missing tru, pred, len, norms, loss or workspace; PIT_ERR_SIZE for batch <= 0,
 *   batch > 65535, npts <= 0, nch <= 0, p < 1, clear_n < 0, or clear_buf == NULL with clear_n > 0.
 * pit_rel_max_norm_ragged - *out = sum_s mean_c max_{l < len[s]} |true - pred| / max_{l < len[s]} |true| (utils.py:59-77 per
 *   truncated sample; fp32 division as in the reference, NaN in a real point propagates).  Forward only, no workspace, one
 *   workgroup: an evaluation metric.  PIT_ERR_NULL for a missing pointer; PIT_ERR_SIZE for batch <= 0, batch > 65535, npts <= 0,
 *   nch <= 0. */
#define PIT_HAS_RAGGED_STEP 1
int pit_rel_lp_loss_ragged_fwd_grad(const float* tru, const float* pred, const int* len, int batch, int npts, int nch, int p,
                                    float* norms, float* loss, unsigned* workspace, float* d_pred_unit, float* clear_buf,
                                    long clear_n, void* stream);
int pit_rel_max_norm_ragged(const float* tru, const float* pred, const int* len, int batch, int npts, int nch, float* out,
                            void* stream);

/* ---- The metrics of an evaluation pass, kept on the device (additions to ABI 31; csrc/pit_eval.hip) -------------------------------
 * The reference scripts evaluate after every epoch: under no_grad they loop over the test loader and add
 * myloss(y, out).item() per batch (train_darcy.py:136-144; train_vorticity.py:131-141 around a 20-step rollout, with the model
 * output in the `true` slot, line 139), report utils.RelMaxNorm beside it (train_burgers.py:80, train_naca.py:132) and write each
 * batch's prediction into pred[batch_size*i : ...] (train_darcy.py:167-177).  pit_eval_metrics is one launch per batch for all of
 * that, with totals that live in `state` from launch to launch, so a pass needs ONE device->host copy at its end.  A library
 * built from this header defines PIT_HAS_EVAL_METRICS; PIT_ABI_VERSION is unchanged (nothing that existed changed).
 *
 * tru / pred (batch, npts, nch) contiguous fp32; pred' = pred*pred_scale + pred_shift ((npts, nch) each, both or neither; two fp32
 * roundings, as the loss kernels form it).  For every valid sample s and channel c, over the sample's first len[s] points:
 *   ||tru - pred'||_p / ||tru||_p   (any integer p >= 1, as pit_rel_lp_loss_fwd)   and   max|tru - pred'| / max|tru|;
 * their means over c are RelLp_s and RelMax_s (utils.py:59-98).  A zero denominator gets no special case (the reference has
 * none); NaN in a real point propagates.
 *   len        (batch) int32 on the device, clamped into [0, npts] where it is read; NULL = npts.  Padded points are never read.
 *   n_valid    one int32 on the device, clamped into [0, batch]: samples s >= *n_valid are skipped - never read, no row written
 *              (a last batch that is only partly filled).  NULL = batch.
 *   state      PIT_EVAL_STATE_DOUBLES doubles on the device, zeroed by the caller to start a pass:
 *                [0] += sum_s RelLp_s      [1] += sum_s RelMax_s      [2] = max(old, max_s RelLp_s)      [3] = max(old, max_s RelMax_s)
 *                [4] the cursor: rows consumed so far (+= *n_valid when advance != 0)      [5] += 1 per launch      [6], [7] stay 0
 *   per_sample optional table: row r = cursor + s at per_sample + r * ps_stride receives {RelLp_s, RelMax_s} (ps_stride >= 2)
 *   pred_store optional: row r at pred_store + r * store_stride receives the sample's (npts, nch) values of pred', zeros in the
 *              padded points (store_stride >= npts * nch)
 *   advance    PIT_EVAL_ADVANCE (1): this launch moves the cursor on by *n_valid; 0: it stays (further launches of the same batch
 *              follow, e.g. the steps of a rollout).  | PIT_EVAL_STORE_TRUE (2): pred_store receives the `tru` slot instead of
 *              pred' - for callers that put the model output there (the argument order of train_vorticity.py:139).  Any other
 *              bit: PIT_ERR_SIZE.
 *   capacity   rows of the two optional outputs: rows r >= capacity are not written (nothing out of range is touched); the
 *              totals still count them
 *   workspace  pit_eval_metrics_workspace(batch, npts, nch) bytes, 8-byte aligned; its first word is the arrival ticket: zero
 *              before the first call, left zero by every call (calls that share it must be stream-ordered)
 * Every workgroup reads the cursor before it takes its ticket; the workgroup of the last ticket alone moves the cursor, after the
 * finishing sums - so one launch per batch is all a captured graph needs.  A (sample, channel) series is split into 1, 2, 4, ...,
 * PIT_EVAL_MAX_PARTS workgroups by a rule on (batch, npts, nch) alone (each part keeps >= 1024 points; no further split once 512
 * workgroups exist); len and n_valid only switch work off.  Partial sums are fp64; the last arriver adds the parts in part order,
 * the channels in channel order and the samples in index order: the same inputs and state give the same bits.  No host
 * synchronisation, no allocation, capturable.
 * PIT_ERR_NULL for a missing tru, pred, state or workspace, or one of pred_scale / pred_shift without the other; PIT_ERR_SIZE for
 * batch <= 0, batch > 65535, npts <= 0, nch <= 0, p < 1, capacity < 0, an optional output with capacity == 0 or with a stride
 * smaller than its row.  pit_eval_metrics_workspace returns PIT_ERR_SIZE for a non-positive size. */
#define PIT_HAS_EVAL_METRICS 1
#define PIT_EVAL_STATE_DOUBLES 8
#define PIT_EVAL_MAX_PARTS 64
#define PIT_EVAL_ADVANCE 1
#define PIT_EVAL_STORE_TRUE 2
long pit_eval_metrics_workspace(int batch, int npts, int nch);
int pit_eval_metrics(const float* tru, const float* pred, const float* pred_scale, const float* pred_shift,
                     const int* len, const int* n_valid, int batch, int npts, int nch, int p, double* state,
                     float* per_sample, long ps_stride, float* pred_store, long store_stride, long capacity,
                     int advance, void* workspace, void* stream);

/* ---- The data feed of a captured step (an addition to ABI 31; csrc/pit_feed.hip) -------------------------------------------------
 * The reference loops take every batch from a host DataLoader - shuffle=True over a TensorDataset - and move it to the device per
 * step (train_darcy.py:98,124-126).  pit_batch_feed is one launch for all of that when the dataset lives in device
 * memory: it picks the step's samples, gathers their rows into the step's static buffers and moves a cursor that lives on the
 * device, so a captured step that begins with it walks through epochs by replays alone.  A library built from this header defines
 * PIT_HAS_BATCH_FEED; PIT_ABI_VERSION is unchanged (nothing that existed changed).
 *
 *   src, dst, row_bytes   HOST arrays of n_fields entries (1..PIT_FEED_MAX_FIELDS), read by the call and passed to the kernel by
 *              value: field f of the dataset is n_samples contiguous rows of row_bytes[f] bytes at src[f] (device memory), dst[f]
 *              the static buffer of `batch` such rows.  row_bytes[f] is a positive multiple of 4 and both pointers are 4-byte
 *              aligned: rows are copied as raw words (any dtype; NaN payloads survive).  src and dst must not overlap.
 *   state      two long long on the device: [0] the cursor (feeds so far; a negative value counts as 0), [1] the arrival ticket:
 *              zero before the first call, left zero by every call (calls that share it must be stream-ordered)
 *   order      optional n_samples int32 on the device: the caller's sampler (takes precedence over shuffle)
 *   indices    optional `batch` int32 on the device: the sample index behind every slot
 *   n_valid    optional int32 on the device
 * With S steps per epoch - floor(n_samples / (batch*world)) with drop_last, the ceiling without - and c = state[0]: epoch
 * e = c / S, step i = c % S; slot s holds global position g = (i*world + rank)*batch + s and the sample
 *   order[g % n_samples] clamped into [0, n_samples)      (order given: every address stays in bounds whatever it holds)
 *   g % n_samples                                         (shuffle == 0)
 *   feistel(n_samples, seed, e)(g % n_samples)            (otherwise)
 * *n_valid = clamp(n_samples - (i*world + rank)*batch, 0, batch); positions past the end wrap, so every slot holds a real sample.
 * The keyed permutation (uint32 arithmetic; engine.feed_order restates it on the host, bit for bit):
 *   fmix(h): h ^= h>>16; h *= 0x85EBCA6B; h ^= h>>13; h *= 0xC2B2AE35; h ^= h>>16
 *   bits = max(2, bit_length(n-1)); bits += bits & 1; half = bits/2; mask = (1<<half)-1
 *   key[j] = fmix(seed_lo ^ fmix(seed_hi + 0x9E3779B9*(e+1) + j)), j = 0..3        (e mod 2^32)
 *   x = g; do { L = x>>half; R = x&mask; for j in 0..3: (L, R) = (R, L ^ (fmix(R + key[j]) & mask)); x = (L<<half)|R; } while (x >= n)
 * - four Feistel rounds with cycle walking (the domain is < 4n): a bijection for every n, but no match for a Fisher-Yates shuffle
 * in quality; callers that want a particular sampler pass `order`.
 * Every workgroup reads the cursor before it takes its ticket; the workgroup of the last ticket alone writes cursor + 1 and clears
 * the ticket.  No host synchronisation, no allocation, capturable.
 * PIT_ERR_NULL for a missing src, dst, row_bytes or state, or a null entry of src or dst; PIT_ERR_SIZE for n_fields outside
 * 1..PIT_FEED_MAX_FIELDS, n_samples <= 0, batch <= 0, batch > 65535, world <= 0, rank outside [0, world), a row_bytes[f] that is
 * not a positive multiple of 4, a src[f] or dst[f] that is not 4-byte aligned, drop_last with n_samples < batch*world (no full
 * step), drop_last or shuffle not 0 or 1; PIT_ERR_UNSUPPORTED for n_samples > 2^31 - 1 and for a row_bytes[f] beyond
 * PIT_FEED_MAX_ROW_BYTES (1 GiB: a row is addressed with 32-bit byte offsets).  All before any launch. */
#define PIT_HAS_BATCH_FEED 1
#define PIT_FEED_MAX_FIELDS 8
#define PIT_FEED_MAX_ROW_BYTES (1L << 30)
int pit_batch_feed(const void* const* src, void* const* dst, const long* row_bytes, int n_fields,
                   long n_samples, int batch, int rank, int world, int drop_last, int shuffle,
                   const int* order, long long seed, long long* state, int* indices, int* n_valid,
                   void* stream);

/* ---- A random subset of each cloud's points, drawn by the feed (an addition to ABI 31; csrc/pit_feed.hip) -------------------------
 * The reference loops hand every step the whole cloud of each sample (train_elasticity.py:64,86-88: the loop over a shuffled
 * DataLoader, x, ext, y = x.cuda(), ext.cuda(), y.cuda() and the forward on all of the cloud's points). pit_batch_feed_points is pit_batch_feed
 * with one more thing done in the same launch: of every sample it delivers a random subset of the cloud's points, the same
 * subset for every field of the cloud, a new one in every epoch - so a step trains on m points of clouds that hold n >= m, the
 * batch is rectangular whatever the clouds' lengths are, and the subset is a function of (seed, epoch, sample, group) that
 * engine.feed_points restates on the host.  pit_batch_feed and its kernel are untouched.  A library built from this header defines
 * PIT_HAS_FEED_POINTS; PIT_ABI_VERSION is unchanged (nothing that existed changed).
 *
 *   src, dst, bytes, kind   HOST arrays of n_fields entries (1..PIT_FEED_MAX_FIELDS), passed to the kernel by value.  kind[f]:
 *              PIT_FEED_WHOLE_ROW   pit_batch_feed's field: n_samples rows of bytes[f] bytes, copied whole
 *              PIT_FEED_POINTS_G0/_G1   a point field of group g = 0 / 1: n_samples rows of n_g points of bytes[f] bytes at src[f],
 *                                   `batch` rows of m_g points of bytes[f] bytes at dst[f]
 *              bytes[f] is a positive multiple of 4 and the pointers are 4-byte aligned: raw words of any dtype (NaN payloads survive)
 *   n0, m0, n1, m1   source and destination widths of the two groups, 1 <= m_g <= n_g (a group without fields: pass 0, 0)
 *   len_src0/1 optional n_samples int32 on the device: the number of real points of every sample's cloud
 *   len_dst0/1 optional `batch` int32 on the device: receives M of every slot (the static lengths of a ragged step)
 *   points0/1  optional (batch, m_g) int32 on the device: the source point behind every destination point, -1 beyond M
 *   everything from n_samples on: as in pit_batch_feed, with the same meaning, cursor and ticket rule.
 * Slot s holds the sample idx that pit_batch_feed would choose with the same arguments and cursor (epoch e).  Then, per group g:
 *   L = clamp(len_src_g[idx], 1, n_g) (n_g without len_src_g);  M = min(m_g, L)
 *   key = seed XOR (((idx + 1) * 0x9E3779B97F4A7C15 + g * 0xD1B54A32D192ED03) mod 2^64)
 *   destination point k < M of every field of the group = source point feistel(L, key, e)(k)      (the keyed permutation above,
 *                                   with n = L and key in the place of seed)
 *   destination points k >= M = zero words;  len_dst_g[s] = M;  points_g[s][k] = the source point, -1 for k >= M
 * Source points >= L are never read (they may hold NaN): every source access goes through a buffer resource that spans exactly
 * the sample's L points of that field.  L <= m_g: all of the cloud's points arrive, permuted.  Two groups of one sample, two
 * samples and two epochs have different keys; a sample that `order` repeats within an epoch repeats its subset.  The subset
 * arrives in permutation order, not sorted.
 * Refusals, all before any launch and in this order: PIT_ERR_NULL for a missing src, dst, bytes, kind or state; PIT_ERR_SIZE for
 * n_fields outside 1..PIT_FEED_MAX_FIELDS; PIT_ERR_NULL for a null entry of src or dst; PIT_ERR_SIZE for n_samples <= 0,
 * batch <= 0, batch > 65535, world <= 0, rank outside [0, world), drop_last or shuffle not 0 or 1, a kind[f] outside 0..2, a
 * bytes[f] that is not a positive multiple of 4, a src[f] or dst[f] that is not 4-byte aligned, a point field whose group has no
 * widths (n_g < 1), a group with fields and m_g < 1 or m_g > n_g, a length or point-table pointer that is not 4-byte aligned or
 * that belongs to a group without fields, drop_last with n_samples < batch*world; PIT_ERR_UNSUPPORTED for n_samples > 2^31 - 1
 * and for a sample's field - bytes[f], n_g * bytes[f] for a point field - beyond PIT_FEED_MAX_ROW_BYTES. */
#define PIT_HAS_FEED_POINTS 1
#define PIT_FEED_WHOLE_ROW 0
#define PIT_FEED_POINTS_G0 1
#define PIT_FEED_POINTS_G1 2
int pit_batch_feed_points(const void* const* src, void* const* dst, const long* bytes, const int* kind, int n_fields,
                          int n0, int m0, int n1, int m1, const int* len_src0, const int* len_src1,
                          int* len_dst0, int* len_dst1, int* points0, int* points1,
                          long n_samples, int batch, int rank, int world, int drop_last, int shuffle,
                          const int* order, long long seed, long long* state, int* indices, int* n_valid,
                          void* stream);

/* ---- The guarded optimizer step (an addition to ABI 31; csrc/pit_optim.hip) ------------------------------------------------------
 * The reference loops run Adam behind CosineAnnealingLR and read loss.item() every step (train_darcy.py:115-116,131-134): a
 * diverging run is seen on the host the moment it happens.  A captured step has no such look, and pit_adam_step consumes whatever
 * gradient it is given.  pit_adam_step_guarded is that step with the look built in, in two launches on the caller's stream and
 * no host round trip.  Beyond the reference: global-norm clipping (torch.nn.utils.clip_grad_norm_), skipping an update whose
 * gradient is not finite, decoupled weight decay (torch.optim.AdamW), a linear warm-up in front of the cosine schedule, and the
 * sum of the steps' losses kept on the device (the scripts' train_l2 += loss.item()).  A library built from this header defines
 * PIT_HAS_GUARDED_ADAM; PIT_ABI_VERSION is unchanged (nothing that existed changed; pit_adam_step is as it was).
 *
 * Launch 1 (grad_sumsq_kernel) writes the sum of squares of the n gradients as P = pit_adam_guard_parts(n) fp64 partials: partial
 * b covers the run [b * R, min(n, (b + 1) * R)), R = 1024 * ceil(n / (1024 * PIT_GUARD_MAX_PARTS)); every value is widened to fp64
 * before it is squared (exact, and no overflow: 3e19 in every element has a finite norm), and every addition inside a run has a
 * fixed place, so the partials have the same bits on every call.  16-byte loads when grads is 16-byte aligned, dwords
 * otherwise (the same bits either way); nothing beyond element n - 1 enters the sum.
 * Launch 2 (adam_step_guarded_kernel): every workgroup adds the P partials in index order and forms norm = sqrt(sum) and
 *   coef = max_norm > 0 ? min(1, max_norm / (norm + 1e-6)) : 1      (fp64, then rounded to fp32; max_norm = 0: clipping off).
 * norm not finite: the call is SKIPPED - params, exp_avg, exp_avg_sq and *step keep their bits; with zero_grads the gradients
 * are still cleared.  Otherwise pit_adam_step's arithmetic runs on g * coef with bias corrections from *step + 1:
 *   decoupled = 1:  p *= fl32(1 - lr_t * weight_decay) in front of the update (AdamW)
 *   decoupled = 0:  g * coef + weight_decay * p (the coupled decay of pit_adam_step, after the clip: torch's order of
 *                   clip_grad_norm_ and Adam.step)
 * Gradients that are kept (zero_grads = 0) stay unclipped in memory; the coefficient is reported in state.
 * Two counters on the device, both zero before the first call: *calls counts every call, skipped ones included, and positions
 * the schedule (scheduler.step() runs every iteration in the scripts); *step counts the applied updates and feeds the bias
 * corrections.  The rate of call k = *calls + 1:
 *   k <= warmup_steps:  lr0 * (warmup_start + (1 - warmup_start) * (k - 1) / warmup_steps)
 *   otherwise:          pit_adam_step's cosine closed form at k - 1 - warmup_steps (lr0 when cosine_t_max == 0)
 * in fp64, once per workgroup; with warmup_steps == 0 and no skipped call it has pit_adam_step's bits.  Every workgroup reads
 * both counters before it takes its ticket (scalars[3]); the workgroup of the last ticket writes them back.
 *   partials   PIT_GUARD_MAX_PARTS doubles of device scratch
 *   state      PIT_GUARD_STATE_DOUBLES doubles on the device (the PIT_GUARD_* slots below), zero before the first call; the caller
 *              may zero them between calls (statistics only: the schedule rests on *calls and *step)
 *   scalars    4 floats, zero before the first call: lr_t of the call, the bias corrections of the last APPLIED update, the ticket
 *   loss       optional device scalar (may be null): added to PIT_GUARD_LOSS_SUM by the last workgroup when it is finite and
 *              counted either way; the skip decision rests on the norm alone
 * PIT_ERR_NULL for a missing pointer other than loss; PIT_ERR_SIZE for n <= 0 and for grads off a 4-byte boundary;
 * PIT_ERR_UNSUPPORTED for a negative or NaN max_norm, warmup_steps < 0, warmup_start outside [0, 1] (or NaN).  All before any
 * launch.  No host synchronisation, no allocation, capturable. */
#define PIT_HAS_GUARDED_ADAM 1
#define PIT_GUARD_MAX_PARTS 256
#define PIT_GUARD_STATE_DOUBLES 10
#define PIT_GUARD_CALLS 0            /* calls since the state was last zeroed */
#define PIT_GUARD_APPLIED 1          /* ... that updated the parameters */
#define PIT_GUARD_SKIPPED 2          /* ... that were skipped (norm not finite) */
#define PIT_GUARD_CLIPPED 3          /* ... applied with coef < 1 */
#define PIT_GUARD_LAST_NORM 4        /* the norm of the last call */
#define PIT_GUARD_MAX_NORM 5         /* the largest finite norm seen */
#define PIT_GUARD_LAST_COEF 6        /* the coefficient of the last call (1 when it was skipped) */
#define PIT_GUARD_LOSS_SUM 7         /* sum of the finite losses */
#define PIT_GUARD_LOSS_FINITE 8      /* how many there were */
#define PIT_GUARD_LOSS_NONFINITE 9   /* and how many were not finite */
int pit_adam_guard_parts(long n);    /* P for n elements (1..PIT_GUARD_MAX_PARTS); PIT_ERR_SIZE for n <= 0 */
int pit_adam_step_guarded(float* params, float* grads, float* exp_avg, float* exp_avg_sq, long n, long long* step,
                          long long* calls, float lr0, float eta_min, int cosine_t_max, int warmup_steps,
                          double warmup_start, float beta1, float beta2, float eps, float weight_decay, int decoupled,
                          double max_norm, int zero_grads, const float* loss, double* partials, double* state,
                          float* scalars, void* stream);

/* ---- Averaged weights in the guarded step, and the exchange behind their evaluation (additions to ABI 31; csrc/pit_optim.hip) ----
 * The reference saves {'model_state': ...} once, at the end (train_darcy.py:150): no optimizer state, no resume, and no averaged
 * copy of the weights.  Beyond the reference: pit_adam_step_averaged is pit_adam_step_guarded with an exponential (EMA) or equal
 * (SWA) average of the parameters kept in the SAME two launches, and pit_exchange_words swaps two buffers in place, so that a
 * captured evaluation graph reads the average where it read the live weights.  A library built from this header defines
 * PIT_HAS_AVERAGED_ADAM; PIT_ABI_VERSION is unchanged (nothing that existed changed; the guarded entry is as it was).
 *
 * The averaged step.  Its arguments are the guarded entry's up to `scalars`, then average, n_averaged, avg_mode, avg_decay,
 * avg_ramp, avg_start, then stream.  Launch 1 is grad_sumsq_kernel; launch 2 (a second instance of
 * adam_step_guarded_kernel) runs the guarded kernel's arithmetic expression for expression: params, both moments, *step, *calls, state and scalars come
 * out with the guarded entry's bits, and the average never feeds back into the update.  On an APPLIED update, with t the new
 * value of *step and p the parameter just written:
 *   t <= avg_start:  average[i] = p; *n_averaged stays 0 (the average follows the weights until averaging starts)
 *   t >  avg_start:  m = t - avg_start, the weight w once per workgroup in fp64, rounded to fp32:
 *                      avg_mode 0 (EMA):    d = avg_ramp ? min(avg_decay, (1 + m) / (10 + m)) : avg_decay;  w = 1 - d
 *                      avg_mode 1 (equal):  w = 1 / m
 *                    a = average[i]; average[i] = (w == 1.0f) ? p : a + w * (p - a)     (three separately rounded fp32 operations)
 *                    *n_averaged = m, written by the workgroup of the last ticket beside the other counters
 * On a SKIPPED call (norm not finite) average and *n_averaged keep their bits.
 *   average     n floats on the device, disjoint from params; the caller starts it as a copy of params
 *   n_averaged  one long long on the device, zero before the first call
 * Refusals, all before any launch, in the order pointers, sizes, values: the guarded entry's, and PIT_ERR_NULL for a missing
 * average or n_averaged; PIT_ERR_UNSUPPORTED for avg_mode other than 0 or 1, for an EMA avg_decay outside [0, 1) (or NaN), for
 * avg_start < 0, and for an average whose n floats overlap those of params.
 *
 * The exchange.  The n_words 4-byte words at a and at b change places, as raw bits (NaN payloads survive), in one launch of a
 * grid-stride loop (at most 2048 workgroups): 16-byte loads and stores where a and b sit equally far from a 16-byte boundary
 * (up to three head and three tail words go one by one), single words otherwise.  PIT_ERR_NULL for a null pointer; PIT_ERR_SIZE
 * for n_words <= 0 and for a base that is not 4-byte aligned; PIT_ERR_UNSUPPORTED when the two ranges overlap.  All before any
 * launch.  No host synchronisation, no allocation, capturable (both entries). */
#define PIT_HAS_AVERAGED_ADAM 1
int pit_adam_step_averaged(float* params, float* grads, float* exp_avg, float* exp_avg_sq, long n, long long* step,
                           long long* calls, float lr0, float eta_min, int cosine_t_max, int warmup_steps,
                           double warmup_start, float beta1, float beta2, float eps, float weight_decay, int decoupled,
                           double max_norm, int zero_grads, const float* loss, double* partials, double* state,
                           float* scalars, float* average, long long* n_averaged, int avg_mode, double avg_decay,
                           int avg_ramp, long long avg_start, void* stream);
int pit_exchange_words(void* a, void* b, long n_words, void* stream);

/* ---- Farthest-point sampling of per-sample clouds (an addition to ABI 31; csrc/pit_fps.hip) ----------------------------------------
 * The reference's cloud model takes the cloud itself as its latent mesh (train_elasticity.py:46), so every processor block is a
 * dense n x n attention per sample.  Beyond the reference: pit_fps picks m << n points of every cloud by farthest-point sampling,
 * in ONE launch with one workgroup per sample, so that a captured step can sample the clouds it is fed.  A library built from
 * this header defines PIT_HAS_FPS; PIT_ABI_VERSION is unchanged (nothing that existed changed).
 *
 *   mesh       fp32: sample s holds n rows of space_dim contiguous floats at mesh + s * mesh_bstride (mesh_bstride in elements,
 *              >= n * space_dim)
 *   lengths    optional `batch` int32 on the device: the real points of every sample, read on the device and clamped into [1, n];
 *              NULL: n everywhere.  Rows at and beyond a sample's length are never read (they may hold NaN).
 *   start      optional `batch` int32 on the device: the first pick of every sample; NULL: start_all.  Clamped into [0, length).
 *   idx        (batch, m) int32; out_mesh (batch, m, space_dim) fp32; out_len optional `batch` int32
 * Sample s with L real points p_0 .. p_{L-1}: dist_i = +inf, cur = start; for t = 0 .. min(m, L) - 1:
 *   idx[t] = cur, out_mesh[t] = p_cur (the same bits);
 *   d_i = ((p_i0 - p_cur0)^2 + (p_i1 - p_cur1)^2) + ... in fp32, coordinates in ascending order, every operation rounded;
 *   dist_i = min(dist_i, d_i);  cur = the LOWEST index i < L with the largest dist_i.
 * Points already chosen have dist 0 and take part like any other: a cloud with fewer than m distinct points repeats points.
 * out_len[s] = min(m, L); slots t >= out_len[s] hold idx -1 and zero coordinates.  Precondition, not checked: the real
 * coordinates are finite; whatever they hold, every index is clamped before use and nothing is addressed out of bounds.
 * The points live in registers: space_dim 1..3 up to PIT_FPS_MAX_POINTS points, space_dim 4..8 up to PIT_FPS_MAX_POINTS_WIDE.
 * No atomics (the same input gives the same bits), no host synchronisation, no allocation, capturable.
 * PIT_ERR_NULL for a missing mesh, idx or out_mesh; PIT_ERR_SIZE for batch outside 1..65535, n < 1, m outside [1, n], space_dim
 * outside 1..PIT_MAX_SPACE_DIM, mesh_bstride < n * space_dim; PIT_ERR_UNSUPPORTED for n beyond the limit of its space_dim.  All
 * before any launch. */
#define PIT_HAS_FPS 1
#define PIT_FPS_MAX_POINTS 16384
#define PIT_FPS_MAX_POINTS_WIDE 4096
int pit_fps(const float* mesh, int batch, int n, int space_dim, long mesh_bstride, const int* lengths, const int* start,
            int start_all, int m, int* idx, float* out_mesh, int* out_len, void* stream);

/* ---- Farthest-point sampling of clouds of any size (an addition to ABI 31; csrc/pit_fps_large.hip) -------------------------------
 * pit_fps keeps a cloud in one workgroup's registers and refuses clouds beyond PIT_FPS_MAX_POINTS.  pit_fps_large is a second
 * sampler with the SAME semantics, bit for bit (the loop stated above: fp32 distances rounded operation by operation, the lowest
 * index among equals, lengths and start clamped, -1 / zero slots beyond the picks), for clouds up to PIT_FPS_LARGE_MAX_POINTS points
 * of 1..PIT_MAX_SPACE_DIM coordinates - one envelope for every space_dim.  The points stay in memory and the running distances in a
 * workspace; a cloud is cut into slices of slice_points points, one workgroup each, and the hand-off between two picks is a kernel
 * boundary: m dependent launches of one kernel on a grid of (slices, batch) workgroups, each of which reduces the previous launch's
 * per-slice candidates itself.  A library built from this header defines PIT_HAS_FPS_LARGE; PIT_ABI_VERSION is unchanged (nothing
 * that existed changed).
 *
 *   mesh .. out_len   as in pit_fps
 *   slice_points      0: the library's choice (1024 points up to 262144 points, beyond that the multiple of 256 that gives 256
 *                     slices: never more than 256 slices per cloud); otherwise a multiple of 256 in [256, 65536] - for tests that
 *                     want several slices at small n, and for tuning.  The result does not depend on it.
 *   workspace         pit_fps_large_workspace(batch, n, slice_points) bytes on the device, 8-byte aligned; needs no initial
 *                     contents and holds nothing between calls.  Calls that share a workspace must run one after the other.
 * The entry accepts small n too (there pit_fps is the single launch and the faster one).  No atomics (the same input gives the same
 * bits), no grid barrier, no host synchronisation, no allocation, capturable (m kernel nodes).
 * PIT_ERR_NULL for a missing mesh, idx, out_mesh or workspace; PIT_ERR_SIZE for batch outside 1..65535, n < 1, m outside [1, n],
 * space_dim outside 1..PIT_MAX_SPACE_DIM, mesh_bstride < n * space_dim, a slice_points that is neither 0 nor a multiple of 256 in
 * [256, 65536]; PIT_ERR_UNSUPPORTED for n > PIT_FPS_LARGE_MAX_POINTS or m > PIT_FPS_LARGE_MAX_SAMPLES.  In this order, all before
 * any launch.  pit_fps_large_workspace returns 0 for sizes the entry refuses. */
#define PIT_HAS_FPS_LARGE 1
#define PIT_FPS_LARGE_MAX_POINTS 4194304
#define PIT_FPS_LARGE_MAX_SAMPLES 16384
long pit_fps_large_workspace(int batch, int n, int slice_points);      /* bytes; 0 for sizes the entry refuses */
int  pit_fps_large(const float* mesh, int batch, int n, int space_dim, long mesh_bstride, const int* lengths,
                   const int* start, int start_all, int m, int* idx, float* out_mesh, int* out_len,
                   int slice_points, void* workspace, void* stream);

/* ---- The k nearest keys of every row, ascending (an addition to ABI 31; csrc/pit_knn.hip) -------------------------------------------
 * The candidate lists of the any-metric layers (pit_distlist_fwd) built on the device without a library sort and - for a box
 * metric - without the n_out x n_in matrix.  Two entries, one selection; a library built from this header defines PIT_HAS_KNN;
 * PIT_ABI_VERSION is unchanged (nothing that existed changed).
 *
 * Row i of sample s has the fp32 distances d_0 .. d_(J-1), J = n_in, to the keys.  Order the pairs (d_j, j) by the distance and then
 * by the key index (what a stable ascending sort of the row gives: the LOWEST index among equals, as in pit_fps):
 *   for t = 0 .. k-1:  idx[s][i][t] = the key of pair t,  dist[s][i][t] = its distance (the kernel's own value);
 *   next[s][i] = the distance of pair k (the (k+1)-th), or +inf when k == J.
 * pit_knn_box - the distances come from coordinates; no matrix is formed.  Per axis a < space_dim, every operation rounded to fp32:
 *     t = |x_a - y_a|;  u_a = min(t, p_a - t) where periods[a] = p_a > 0, u_a = t otherwise (periods NULL: no axis wraps);
 *     d = ((u_0*u_0 + u_1*u_1) + u_2*u_2) + ...   coordinates in ascending order
 *   mesh_out / mesh_in: (n_out, space_dim) / (n_in, space_dim) fp32 per sample; out_stride / in_stride: POINTS between two samples'
 *   meshes, 0 = one mesh shared by every sample and read in place, otherwise >= n_out / n_in (the *_strided convention above).
 *   periods: a HOST array of space_dim floats, read during the call, or NULL.  1 <= space_dim <= PIT_MAX_SPACE_DIM.
 * pit_knn_rows - the distances are rows of a matrix the caller formed: sample s, row i at m + s * m_bstride + i * ld_m, n_in floats
 *   (ld_m >= n_in; m_bstride 0 = one matrix for every sample, otherwise >= (n_out-1)*ld_m + n_in: pit_distmat_select_fwd's
 *   convention).  Precondition, not checked: the entries are finite and >= 0; -0.0 counts as 0 and comes out as +0.0.  Whatever the
 *   entries hold, every emitted index lies in [0, n_in), the indices of a row are distinct and nothing is addressed out of bounds;
 *   columns at or beyond n_in and rows at or beyond n_out are never read.
 * Outputs of both: idx (batch, n_out, k) int32, dist (batch, n_out, k) fp32, next (batch, n_out) fp32, contiguous.
 * One launch, a workgroup per row (any batch * n_out).  A row of up to PIT_KNN_REG_MAX_KEYS keys keeps its distances in registers
 * (form 1); a longer row is streamed and its distances are recomputed in every pass of the search (form 2).  No global atomics (the
 * same input gives the same bits), no workspace, no allocation, no host synchronisation, capturable.
 * 1 <= k <= min(n_in, PIT_KNN_MAX_K); batch * n_out * k < 2^31.  Refusals, all before any launch and in this order: PIT_ERR_NULL for
 * a missing mesh_out, mesh_in / m, idx, dist or next; PIT_ERR_SIZE for batch, n_out or n_in < 1, space_dim outside
 * 1..PIT_MAX_SPACE_DIM, a stride the conventions above refuse, k outside [1, n_in], batch * n_out * k >= 2^31;
 * PIT_ERR_UNSUPPORTED for k > PIT_KNN_MAX_K.
 * pit_knn_last_form - host-side and process-global: the form (1 or 2) of this process's latest pit_knn_box / pit_knn_rows launch,
 *   0 before the first. */
#define PIT_HAS_KNN 1
#define PIT_KNN_MAX_K 2048            /* the width the list layers accept (PIT_DISTLIST_MAX_CAP) */
#define PIT_KNN_REG_MAX_KEYS 1024     /* rows up to this many keys take form 1 */
int pit_knn_box(const float* mesh_out, const float* mesh_in, int batch, int n_out, int n_in, int space_dim, long out_stride,
                long in_stride, const float* periods, int k, int* idx, float* dist, float* next, void* stream);
int pit_knn_rows(const float* m, long ld_m, long m_bstride, int batch, int n_out, int n_in, int k, int* idx, float* dist,
                 float* next, void* stream);
int pit_knn_last_form(void);

/* ---- pit_knn_box on ragged batches (an addition to ABI 31; csrc/pit_knn.hip) --------------------------------------------------------
 * pit_knn_box_ragged - pit_knn_box plus len_out / len_in: int32 DEVICE arrays of `batch` entries, clamped into [1, n_out] /
 * [1, n_in] by the kernel, either NULL = the full width; no host synchronisation, capturable.  Sample s searches its first
 * L = len_in[s] keys only: keys beyond are never read (they may hold NaN).  A real row i < len_out[s] emits k' = min(k, L) pairs -
 * idx, dist and next equal pit_knn_box on the trimmed sample (n_out = len_out[s], n_in = L, k') bit for bit; its slots t >= k' hold
 * key -1 and distance 0, and next is the distance of pair k or +inf when k >= L.  A row i >= len_out[s] holds -1 / 0 / +inf and reads
 * nothing.  The form (pit_knn_last_form) is chosen from the padded n_in on the host; the refusals are pit_knn_box's, in its order,
 * with the padded sizes.  A library built from this header defines PIT_HAS_KNN_RAGGED; PIT_ABI_VERSION is unchanged. */
#define PIT_HAS_KNN_RAGGED 1
int pit_knn_box_ragged(const float* mesh_out, const float* mesh_in, int batch, int n_out, int n_in, int space_dim, long out_stride,
                       long in_stride, const float* periods, int k, const int* len_out, const int* len_in, int* idx, float* dist,
                       float* next, void* stream);

/* ---- The k nearest keys of every row under the path length of a graph (an addition to ABI 31; csrc/pit_geo.hip) ----------------------
 * The candidate lists of the any-metric layers where the metric is a geodesic: a truncated single-source shortest-path search per
 * row, in the list layers' own format (pit_knn_box_ragged's: key -1 / distance 0 in the slots a row does not fill).  A library
 * built from this header defines PIT_HAS_GEO; PIT_ABI_VERSION is unchanged (nothing that existed changed).
 *
 * The graph of sample s on n_vert vertices, padded adjacency: edge t of vertex u leads to adj[s][u][t] and has the length
 * w[s][u][t] (fp32, finite and >= 0: not checked - nothing is addressed out of bounds whatever adj and w hold); it is valid iff
 * 0 <= adj[s][u][t] < Vs, Vs = len_v[s] clamped into [1, n_vert] (len_v NULL: n_vert).  Directed; self edges and duplicate edges
 * are harmless.  adj_bstride: ELEMENTS between two samples' (n_vert, n_edge) arrays, of adj and w alike; 0 = one graph shared by
 * the batch, otherwise >= n_vert * n_edge.  Adjacency rows of vertices >= Vs are never read.
 * The path length D from a row's source is the least fixpoint of D(src) = 0, D(v) = min(D(v), fl32(D(u) + w(u, v))): one rounded
 * fp32 add per edge, which label-setting search reaches exactly (fp32 addition is monotone).
 * Row i of sample s starts at sources[s * src_bstride + i] (src_bstride 0 = one array for every sample, otherwise >= n_rows;
 * sources NULL: vertex i, which needs n_rows == n_vert and src_bstride 0); a source outside [0, Vs) is a padded row.  key_of (NULL:
 * the identity; key_bstride like src_bstride, >= n_vert) maps a vertex to its key index, < 0 = the vertex is no key.  The row's
 * candidates are the pairs (D(v), v) of the reachable key vertices; its list is the k smallest ascending by (D, v) - the lowest
 * VERTEX index among equal lengths:
 *   idx[s][i][t] = key_of[v_t],  dist[s][i][t] = D(v_t) (the length, not its square);  unfilled slots (fewer than k reachable
 *   keys, a truncated row, a padded row): -1 / 0;
 *   next[s][i]   = the smaller of candidate k's length (the (k+1)-th) where the search settled one and the least tentative length
 *                  of the frontier when the row was complete; +inf when neither exists.  Exact when every vertex is a key, a lower
 *                  bound otherwise.  A padded row and a truncated row: +inf;
 *   status[s][i] = 0 complete (or padded), 1 truncated.
 * A row is complete when its frontier is empty, or k candidates are settled and the frontier's least tentative length is strictly
 * greater than the k-th candidate's (a vertex discovered at a settled length may have the lower index).  `reach` bounds the
 * discovered vertices (settled or in the frontier) of a row: when relaxing a settled vertex's edges would make them more than
 * `reach`, the row stops as truncated and lists the key vertices settled so far (that vertex included) - a settled length is
 * final, so what a truncated row lists is exact.  No row takes more than `reach` steps.
 * Outputs contiguous: idx (batch, n_rows, k) int32, dist (batch, n_rows, k) fp32, next (batch, n_rows) fp32, status (batch, n_rows)
 * int32.  One launch, a wavefront per row, the row's state in LDS (8 bytes per discovered vertex and a 16-bit hash slot for two);
 * no workspace, no global atomics (the same input gives the same bits), no host synchronisation, capturable.
 * 1 <= k <= PIT_GEO_MAX_K, k <= reach <= PIT_GEO_MAX_REACH, n_vert * n_edge < 2^31, batch * n_rows * k < 2^31.  Refusals, all before
 * any launch and in this order: PIT_ERR_NULL for a missing adj, w, idx, dist, next or status; PIT_ERR_SIZE for batch, n_vert,
 * n_edge, n_rows or k < 1, reach < k, n_vert * n_edge >= 2^31, a stride the conventions above refuse, sources NULL with n_rows != n_vert, batch * n_rows * k >= 2^31;
 * PIT_ERR_UNSUPPORTED for k > PIT_GEO_MAX_K or reach > PIT_GEO_MAX_REACH. */
#define PIT_HAS_GEO 1
#define PIT_GEO_MAX_K 1024
#define PIT_GEO_MAX_REACH 4096
int pit_geo_knn(const int* adj, const float* w, long adj_bstride, int batch, int n_vert, int n_edge, const int* sources,
                long src_bstride, int n_rows, const int* key_of, long key_bstride, const int* len_v, int k, int reach, int* idx,
                float* dist, float* next, int* status, void* stream);

/* ---- The two slab forms of pit_block_fwd (additions to ABI 31; csrc/pit_block.hip) ------------------------------------------------
 * pit_block_fwd runs 16-row slabs, or - n_head = 2, n_pts = 256, the weights through LDS, and 8 * ceil(batch / 8) * n_pts / 8
 * workgroups no more than the device has CUs (batch <= 8 on MI355X) - 8-row slabs with the two heads stacked in the M dimension of
 * one MFMA (both heads contract the same value rows).  Every per-element sum keeps its order, so the two forms write the same
 * bits to xcat, z1, h, z2 and y.  A library built from this header defines PIT_HAS_BLOCK_ROWS8; PIT_ABI_VERSION is unchanged
 * (nothing that existed changed; pit_block_fwd keeps its signature).  The environment variable PIT_BLOCK_ROWS8=0 (read once)
 * keeps the automatic choice on the 16-row form.  Host-side and process-global, no device work, nothing read by a kernel:
 *
 * pit_block_fwd_set_form - 0: automatic (the rule above), 16: always the 16-row form, 8: the stacked form wherever the rule
 *   above admits it (PIT_BLOCK_ROWS8 notwithstanding), 16 rows elsewhere.  Returns the previous value, PIT_ERR_SIZE (nothing
 *   changed) for any other argument.  Meant for tests and A/B runs: a graph captured earlier keeps the form it was captured with.
 * pit_block_fwd_last_rows - the slab height (8 or 16) of the most recent pit_block_fwd launch of this process, 0 before the
 *   first. */
#define PIT_HAS_BLOCK_ROWS8 1
int pit_block_fwd_set_form(int form);
int pit_block_fwd_last_rows(void);

/* The weight-gradient riders of pit_block_bwd (`rider`, `rider2`; fp32 math mode) run in three forms: register-direct MFMA tiles
 * split over the rows, LDS-staged 64 x 64 tiles per row slab, and - a dW2 | db2 with n2 <= 4 and n1 in {32, 64, 128} - a vector-ALU
 * row reduction on at most 16 workgroups (one add per output element and workgroup).  When `rider` is the block's own MLP (rows =
 * batch * n_pts), both its reductions are 64 x 64 tiles and batch is a multiple of 8, a row slab's tiles run on the XCD that the
 * chain gives the slab's sample.  With d(scale) wanted and at most an eighth of the riders beyond the d(scale) slabs' count, the
 * d(scale) slabs take the launch's first workgroup ids and the chain slabs the second range: riders share the compute units of
 * the first range, and the chain is the longer of the two.  Only the summation order of the thin dW2 | db2 differs from the older
 * plan; the environment variable PIT_RIDER_TAIL=0 (read once) keeps that plan, the id-order tile map and the chain slabs first.  A library built from this header defines
 * PIT_HAS_RIDER_TAIL; PIT_ABI_VERSION is unchanged (nothing that existed changed).
 *
 * pit_block_bwd_last_riders - rider workgroups of the most recent pit_block_bwd launch of this process by form, whether the
 *   XCD-local map was used and which range came first: copies min(n, PIT_BLOCK_RIDER_SLOTS) values to out (host array), returns PIT_BLOCK_RIDER_SLOTS.
 *   Host-side and process-global, no device work, nothing read by a kernel. */
#define PIT_HAS_RIDER_TAIL 1
#define PIT_BLOCK_RIDER_RD    0   /* workgroups of register-direct reductions (gemm_rd_body)              */
#define PIT_BLOCK_RIDER_TILE  1   /* gemm_rr_tile tiles                                                  */
#define PIT_BLOCK_RIDER_THIN  2   /* thin_rider workgroups                                               */
#define PIT_BLOCK_RIDER_LOCAL 3   /* 1: `rider`'s tiles were dealt to their sample's XCD, 0: by id alone */
#define PIT_BLOCK_RIDER_DS_FIRST 4 /* 1: the d(scale) slabs had the launch's first workgroup ids, 0: the chain slabs */
#define PIT_BLOCK_RIDER_SLOTS 5
int pit_block_bwd_last_riders(int* out, int n);

/* The finishing launch carrying several postponed jobs (csrc/pit_posatt.hip: posatt_dhead_finish_tail).  A rider tile of
 * pit_block_bwd is latency - two cold round trips, 1.7 us of fp32 MFMA, the atomics' acknowledgement - and a launch pays for it
 * once however many run side by side; pit_posatt_dhead_finish pays that price already for its `rider` and leaves most compute
 * units idle.  So a caller may hand the jobs of its LAST block launches (which then pass rider = rider2 = NULL and shrink to
 * their chain) to the finishing launch.  A library built from this header defines PIT_HAS_FINISH_TAIL; PIT_ABI_VERSION is
 * unchanged (nothing that existed changed: a finish call with nothing staged makes the launches it always made).
 *
 * pit_posatt_dhead_finish_stage - host-only, no device work: COPIES the n job structs jobs[0..n) (the caller's may die at once)
 *   into a list of the calling thread; several calls append.  The thread's NEXT pit_posatt_dhead_finish consumes the list,
 *   whatever else it does: up to 8 staged jobs in the fp32 math mode that accumulate and have at most 2^28 MACs run inside its
 *   launch beside `rider` - as 64 x 64 LDS-staged tiles, the thin dW2 | db2 row reduction or register-direct tiles, 512 threads and
 *   64 KiB of LDS per workgroup; beyond two workgroups per compute unit the job with the most tiles takes more rows per tile.
 *   Every other staged job - and every staged job when n_layers <= 0 or the call's arguments are refused - runs as the
 *   pit_mlp_bwd_params launches of its own on `stream`, after the finishing launch.  d_head is what it is without staged jobs,
 *   bit for bit.  The staging call notes each job in pit_debug_rider_counts, under PIT_RIDER_DHEAD_FINISH when the finish call
 *   will carry it and PIT_RIDER_OWN otherwise; the finish call notes its `rider` only.  Returns 0, PIT_ERR_NULL (jobs or one of
 *   its entries NULL: nothing staged) or PIT_ERR_SIZE (n < 0).
 * pit_finish_last_tail - what the most recent pit_posatt_dhead_finish of this process did with staged jobs: copies
 *   min(n, PIT_FINISH_TAIL_SLOTS) values to out (host array), returns PIT_FINISH_TAIL_SLOTS.  All zero after a call that found
 *   nothing staged.  Host-side and process-global, no device work, nothing read by a kernel. */
#define PIT_HAS_FINISH_TAIL 1
#define PIT_FINISH_TAIL_STAGED  0   /* jobs the call found staged                                           */
#define PIT_FINISH_TAIL_CARRIED 1   /* ... of those, performed inside the finishing launch                  */
#define PIT_FINISH_TAIL_RD      2   /* their workgroups: register-direct reductions (gemm_rd_body)          */
#define PIT_FINISH_TAIL_TILE    3   /* gemm_rr_tile tiles                                                   */
#define PIT_FINISH_TAIL_THIN    4   /* thin_rider workgroups                                                */
#define PIT_FINISH_TAIL_OWN     5   /* staged jobs performed as launches of their own                       */
#define PIT_FINISH_TAIL_SLOTS   6
int pit_posatt_dhead_finish_stage(const pit_mlp_params_job* const* jobs, int n);
int pit_finish_last_tail(int* out, int n);

/* Layout probe used by the tests: D = A(32x8) * B(8x32) through the same
 * v_mfma_f32_32x32x2_f32 fragment maps the kernels use. */
int pit_debug_mfma_tile(const float* a, const float* b, float* d, void* stream);

/* Where the postponed weight-gradient jobs (pit_mlp_params_job, the `rider` arguments above) went: host-side counters of
 * the CALLING THREAD, one per kind below, incremented when a launch accepts a job (PIT_RIDER_OWN: every
 * pit_mlp_bwd_params call, which is also what a host that refuses a job makes).  Copies min(n, PIT_RIDER_KINDS) counters
 * to out (host array) and zeroes them all when reset != 0; returns PIT_RIDER_KINDS.  No device work. */
#define PIT_RIDER_OWN          0   /* pit_mlp_bwd_params: a launch of its own                                          */
#define PIT_RIDER_PAIR_DW      1   /* pit_posatt_bwd, dense: posatt_bwd_pair_dw_kernel (narrow tiles, plan_dw_pair)    */
#define PIT_RIDER_PAIR_WIDE    2   /* pit_posatt_bwd, dense: posatt_bwd_pair_wide_kernel (gemm_rr tiles, fp32 / bf16) */
#define PIT_RIDER_SPARSE_PAIR  3   /* pit_posatt_bwd, candidate lists: posatt_sparse_bwd_dw_kernel                     */
#define PIT_RIDER_SPARSE_ROWS  4   /* pit_posatt_bwd, candidate lists: posatt_sparse_rows_dw (d(scale) only)          */
#define PIT_RIDER_DHEAD_FINISH 5   /* pit_posatt_dhead_finish: posatt_dhead_finish_dw                                 */
#define PIT_RIDER_BLOCK        6   /* pit_block_bwd: `rider`                                                           */
#define PIT_RIDER_BLOCK2       7   /* pit_block_bwd: `rider2`                                                          */
#define PIT_RIDER_SATT         8   /* pit_satt_bwd: the merged d(values) + d(scale) launch                             */
#define PIT_RIDER_KINDS        9
int pit_debug_rider_counts(int* out, int n, int reset);

/* Which kernels the GEMM core (csrc/pit_mlp.hip, csrc/pit_mlp_slab.hip: pit_mlp_*, pit_linear_*) launched: host-side
 * counters of the CALLING THREAD, one per kind below, incremented by the host code at every launch site; one kind per kernel
 * and per template instance that differs in tile geometry.  The PIT_GEMM_LAST_* slots are not counters: they hold the template
 * arguments of the most recent fused launch.  Copies min(n, PIT_GEMM_KINDS) slots to out (host array) and zeroes them all when
 * reset != 0; returns PIT_GEMM_KINDS.  No device work, nothing read by a kernel. */
#define PIT_GEMM_RD_TN1            0   /* gemm_rd_kernel<1, *>: register-direct, one 32-column tile per wave               */
#define PIT_GEMM_RD_TN2            1   /* gemm_rd_kernel<2, *>: two column tiles per wave                                  */
#define PIT_GEMM_RD_PAIR           2   /* gemm_rd_pair_kernel<1, ATOMIC>: both weight-gradient reductions                  */
#define PIT_GEMM_RD_TRIPLE_TN1     3   /* gemm_rd_triple_kernel<1>: dX + both reductions                                   */
#define PIT_GEMM_RD_TRIPLE_TN2     4   /* gemm_rd_triple_kernel<2>                                                         */
#define PIT_GEMM_LDS_32            5   /* gemm_lds_kernel<32, ...>: fp32 math, LDS-staged (with or without AGZ)            */
#define PIT_GEMM_LDS_64            6   /* gemm_lds_kernel<64, ...>                                                         */
#define PIT_GEMM_LDS_128           7   /* gemm_lds_kernel<128, ...>                                                        */
#define PIT_GEMM_LDS_AGZ           8   /* ... of those, the launches with the trailing-gelu prologue (AGZ)                 */
#define PIT_GEMM_BFL_32            9   /* gemm_bfl_kernel<32, ..., IO16 = false>: bf16 math, fp32 storage                  */
#define PIT_GEMM_BFL_64           10   /* gemm_bfl_kernel<64, ..., false>                                                  */
#define PIT_GEMM_BFL_128          11   /* gemm_bfl_kernel<128, ..., false>                                                 */
#define PIT_GEMM_BFL_IO16         12   /* gemm_bfl_kernel<*, ..., IO16 = true>: bf16 storage (PIT_IO_*), any tile height   */
#define PIT_GEMM_RR               13   /* gemm_rr_kernel, one reduction                                                    */
#define PIT_GEMM_RR_PAIR          14   /* gemm_rr_kernel, the two reductions of one MLP                                    */
#define PIT_GEMM_MUL_GELU_GRAD    15   /* mul_gelu_grad_kernel: the trailing-gelu prologue as a pass of its own            */
#define PIT_GEMM_THIN_DZ1         16   /* thin_dz1_kernel                                                                  */
#define PIT_GEMM_THIN_FWD         17   /* thin_fwd_kernel, streamed = 0                                                    */
#define PIT_GEMM_THIN_FWD_STREAM  18   /* thin_fwd_kernel, streamed = 1                                                    */
#define PIT_GEMM_THIN_DW          19   /* thin_dw_kernel                                                                   */
#define PIT_GEMM_MLP_FWD16        20   /* mlp_fwd16_kernel<N1, KS>                                                         */
#define PIT_GEMM_MLP_BWD16        21   /* mlp_bwd16_kernel<N1, TPW>                                                        */
#define PIT_GEMM_MLP_FWD64        22   /* mlp_fwd64_kernel<KS, THIN = false>                                               */
#define PIT_GEMM_MLP_FWD64_THIN   23   /* mlp_fwd64_kernel<KS, true>                                                       */
#define PIT_GEMM_MLP_BWD64        24   /* mlp_bwd64_kernel<T, false>                                                       */
#define PIT_GEMM_MLP_BWD64_THIN   25   /* mlp_bwd64_kernel<T, true>                                                        */
#define PIT_GEMM_LAST_FWD16       26   /* last mlp_fwd16 instance: N1 * 100 + KS                                           */
#define PIT_GEMM_LAST_BWD16       27   /* last mlp_bwd16 instance: N1 * 100 + TPW                                          */
#define PIT_GEMM_LAST_FWD64       28   /* last mlp_fwd64 instance: KS                                                      */
#define PIT_GEMM_LAST_BWD64       29   /* last mlp_bwd64 instance: T                                                       */
#define PIT_GEMM_KINDS            30
int pit_debug_gemm_counts(int* out, int n, int reset);

/* Which kernels the masked-layer dispatcher of csrc/pit_posatt.hip (pit_posatt_fwd_job, pit_posatt_bwd: the candidate-list and
 * union-tile kernels) launched: host-side counters of the CALLING THREAD, one per kind below, incremented by the host code after
 * the launch call at every launch site.  The PIT_ATT_LAST_* slots are not counters: they hold the template arguments (and the
 * column blocks) of the most recent launch of their family.  PIT_ATT_DENSE is one coarse counter for every dense (MFMA) launcher.
 * Copies min(n, PIT_ATT_KINDS) slots to out (host array) and zeroes them all when reset != 0; returns PIT_ATT_KINDS.  No device
 * work, nothing read by a kernel.  A library built from this header defines PIT_HAS_ATT_COUNTS; PIT_ABI_VERSION is unchanged
 * (nothing that existed changed).  (PIT_ATT_UNION_FWD / _DSCALE / _DV / _ZERO below are SLOTS of this record; PIT_ATT_UNION
 * above, 0x2000, is the math_mode flag and no slot.) */
#define PIT_HAS_ATT_COUNTS 1
#define PIT_ATT_LIST_ROWS_FWD      0   /* posatt_sparse_rows<NH, CR, 0>: plain grid                                        */
#define PIT_ATT_LIST_ROWS_DSCALE   1   /* posatt_sparse_rows<NH, CR, 1>: plain grid                                        */
#define PIT_ATT_LIST_ROWS_X        2   /* posatt_sparse_rows_x<NH, CR, *>: XCD-remapped, either mode                       */
#define PIT_ATT_LIST_ROWS_W        3   /* posatt_sparse_rows_w<NH, CR>: forward carrying the block weights                 */
#define PIT_ATT_LIST_ROWS_DW       4   /* posatt_sparse_rows_dw<NH, CR>: d(scale) carrying a weight-gradient rider         */
#define PIT_ATT_LIST_COLS          5   /* posatt_sparse_cols<CR, false>: plain grid                                        */
#define PIT_ATT_LIST_COLS_X        6   /* posatt_sparse_cols_x<CR, *>: XCD-remapped                                        */
#define PIT_ATT_LIST_COLS_D16      7   /* posatt_sparse_cols<CR, true> / posatt_sparse_cols_x<CR, true>: bf16 d_out        */
#define PIT_ATT_LIST_PAIR          8   /* posatt_sparse_bwd_kernel<NH, CRR, CRC, false>                                    */
#define PIT_ATT_LIST_PAIR_DW       9   /* posatt_sparse_bwd_dw_kernel<NH, CRR, CRC>: the pair carrying a rider             */
#define PIT_ATT_LIST_PAIR_D16     10   /* posatt_sparse_bwd_kernel<NH, CRR, CRR, true>: bf16 d_out                         */
#define PIT_ATT_LIST_OVERFLOW     11   /* posatt_sparse_overflow_cols                                                      */
#define PIT_ATT_LIST_ROWS8        12   /* posatt_sparse_rows8<NH, MODE>: 4..8 coordinates                                  */
#define PIT_ATT_LIST_COLS8        13   /* posatt_sparse_cols8<*, *>                                                        */
#define PIT_ATT_LIST_OVERFLOW8    14   /* posatt_sparse_overflow_cols8                                                     */
#define PIT_ATT_UNION_FWD         15   /* posatt_union_kernel<NH, 0, EPL>                                                  */
#define PIT_ATT_UNION_DSCALE      16   /* posatt_union_kernel<NH, 1, EPL>                                                  */
#define PIT_ATT_UNION_DV          17   /* posatt_union_dv_kernel<NH, EPL>                                                  */
#define PIT_ATT_UNION_ZERO        18   /* zero_f32_kernel in front of posatt_union_dv_kernel                               */
#define PIT_ATT_DHEAD_FINISH      19   /* posatt_dhead_finish of a non-deferred pit_posatt_bwd                             */
#define PIT_ATT_HEAD_SCALE        20   /* pit_head_scale up front in pit_posatt_fwd_job (union tiles, rows > 8192)         */
#define PIT_ATT_DENSE             21   /* launch_rows, launch_cols, launch_bwd_pair: any dense kernel                      */
#define PIT_ATT_LAST_ROWS         22   /* last list rows launch (plain, _x, _w, _dw): NH * 100 + CR                        */
#define PIT_ATT_LAST_COLS         23   /* last posatt_sparse_cols* launch: CR                                              */
#define PIT_ATT_LAST_PAIR         24   /* last pair launch: NH * 10000 + CRR * 100 + CRC                                   */
#define PIT_ATT_LAST_UNION        25   /* last union launch (either kernel): NH * 100 + EPL                                */
#define PIT_ATT_LAST_UNION_PER    26   /* last posatt_union_kernel launch: column passes per wavefront                     */
#define PIT_ATT_LAST_GRID_Y       27   /* column blocks of the last list rows / cols launch (grid.y before any remap)      */
#define PIT_ATT_KINDS             28
int pit_debug_att_counts(int* out, int n, int reset);

/* Which DENSE (MFMA) position-attention kernel of csrc/pit_posatt.hip ran, and which instance of it: the same kind of record
 * for launch_rows / launch_cols / launch_rows8 / launch_cols8 / launch_rows_tiles / launch_cols_tiles / launch_bwd_pair, i.e. for
 * pit_posatt_fwd / pit_posatt_bwd without candidate lists (or where the list path declines) and pit_posatt_pre_fwd / _bwd.
 * Host-side counters of the CALLING THREAD, one per kernel template, incremented beside the launch call.  The PIT_DENSE_LAST_*
 * slots are not counters; they hold, in decimal digits, the template arguments of the most recent launch of their family:
 *   J-split rows / cols / pair (and rows8 / cols8, which are CT 1, IL 0):  CT * 10000 + WAVES * 1000 + IL * 100 + MASKED * 10 + BF
 *     (WAVES = wavefronts per workgroup, 1..8; BF = the instance contracts in bf16; the pair's rows half is exact fp32 whatever BF)
 *   tiles rows:  RT * 100000 + TPWG * 1000 + MASKED * 100 + BF * 10 + PRE   (TPWG = column tiles per workgroup = 8 * TPW: 8, 16, 32)
 *   tiles cols:                TPWG * 1000 + MASKED * 100 + BF * 10 + PRE
 * and PIT_DENSE_LAST_GRID_X / _Y / _Z the grid of the most recent dense launch of any family (riders' workgroups included).
 * Copies min(n, PIT_DENSE_KINDS) slots to out (host array) and zeroes them all when reset != 0; returns PIT_DENSE_KINDS.  No
 * device work, nothing read by a kernel.  A library built from this header defines PIT_HAS_DENSE_COUNTS; PIT_ABI_VERSION is
 * unchanged.  PIT_ATT_DENSE above still counts what it counted: the launches made through launch_rows, launch_cols and
 * launch_bwd_pair (not those of pit_posatt_pre_fwd / _bwd). */
#define PIT_HAS_DENSE_COUNTS 1
#define PIT_DENSE_ROWS_FWD           0   /* posatt_rows_kernel<CT, 0, M, BF, IL>                                            */
#define PIT_DENSE_ROWS_DSCALE        1   /* posatt_rows_kernel<CT, 1, M, false, IL>                                         */
#define PIT_DENSE_COLS               2   /* posatt_cols_kernel<CT, M, BF, IL>                                               */
#define PIT_DENSE_PAIR               3   /* posatt_bwd_pair_kernel<M, BF>: d(scale) + d(values), CT 1                       */
#define PIT_DENSE_PAIR_WIDE          4   /* posatt_bwd_pair_wide_kernel<CT, M, BF, IL>: CT 2 / 4, with or without its rider */
#define PIT_DENSE_PAIR_DW            5   /* posatt_bwd_pair_dw_kernel<M, BF>: the CT 1 pair carrying a weight-gradient rider */
#define PIT_DENSE_TILES_ROWS_FWD     6   /* posatt_rows_tiles<RT, TPW, 0, M, BF, PRE>                                       */
#define PIT_DENSE_TILES_ROWS_DSCALE  7   /* posatt_rows_tiles<RT, TPW, 1, M, false, PRE>                                    */
#define PIT_DENSE_TILES_COLS         8   /* posatt_cols_tiles<TPW, M, BF, PRE>                                              */
#define PIT_DENSE_ROWS8              9   /* posatt_rows_kernel8<MODE, M, BF>: 4..8 coordinates, either mode                 */
#define PIT_DENSE_COLS8             10   /* posatt_cols_kernel8<M, BF>                                                      */
#define PIT_DENSE_LAST_ROWS         11   /* last posatt_rows_kernel / _kernel8 launch (packing above)                       */
#define PIT_DENSE_LAST_COLS         12   /* last posatt_cols_kernel / _kernel8 launch                                       */
#define PIT_DENSE_LAST_PAIR         13   /* last pair launch (any of the three kernels)                                     */
#define PIT_DENSE_LAST_TILES_ROWS   14   /* last posatt_rows_tiles launch                                                   */
#define PIT_DENSE_LAST_TILES_COLS   15   /* last posatt_cols_tiles launch                                                   */
#define PIT_DENSE_LAST_GRID_X       16   /* grid of the last dense launch                                                   */
#define PIT_DENSE_LAST_GRID_Y       17
#define PIT_DENSE_LAST_GRID_Z       18
#define PIT_DENSE_KINDS             19
int pit_debug_dense_counts(int* out, int n, int reset);

#ifdef __cplusplus
}
#endif
#endif /* PIT_HIP_H */
