/* volt_hip.h -- C ABI of libvolt_hip.so: Volt's exact-GP hot path on MI355X (gfx950).
 *
 * This is the operator-level boundary of SURVEY.md 8(b).  The reference has no native layer:
 * its hot path is a sequence of ATen calls issued from Python (file:line under the g-benton/Volt
 * tree).  Each entry point below names the reference call site(s) it replaces.  A maintainer binds
 * them with ctypes (INTEGRATION.md shows the stub); volt_amd/_lib.py is that binding.
 *
 * Conventions (all entry points):
 *   - Plain pointers and sizes only.  Every pointer except `stream` is a DEVICE pointer owned by the
 *     caller (e.g. torch `tensor.data_ptr()`).  The library never allocates, frees or retains
 *     caller-visible memory; scratch comes from the caller via the *_workspace_bytes queries.
 *   - `stream` is a hipStream_t passed as void* (torch.cuda.current_stream().cuda_stream); work is
 *     enqueued asynchronously and the call returns immediately.  Re-entrant across streams.  Library state:
 *     one pool of auxiliary streams and fork/join events per device, created on first use and kept for the
 *     life of the process (the batched factorisation runs groups of matrices on them, forked from and joined
 *     back into `stream`); calls on one device serialise on the host while they ENQUEUE, never on the device.
 *     And HOST-side only: a cache of launch schedules per (batch size, block columns, inverse?) -- a few hundred KB of
 *     tables in pinned host memory (3 <= B <= 64, csrc/sched.h), a pure function of the shape.  The library owns NO
 *     device memory and keeps NO record of caller workspaces: volt_mll_workspace_init_f32 / volt_potrf_workspace_init_f32
 *     copy a table into the caller's scratch, and the caller states that it did so with the VOLT_WS_INITIALISED flag of
 *     the entry points that take a workspace.  Without the flag a call runs the table-free schedules; with it every
 *     table-driven launch checks the header in the scratch first, so a region that was never initialised, or was
 *     overwritten since, is reported (info = INT_MIN + 1), never followed.
 *   - Return value: 0 = enqueued; -k = argument k (1-based) is invalid; >0 = hipError_t of a
 *     failed launch.  A matrix that is not positive definite is NOT an error return: LAPACK-style
 *     `info[b]` (0, or the 1-based index of the first non-positive / NaN pivot) is written to a
 *     caller buffer and the jitter-retry policy (gpytorch psd_safe_cholesky, used at
 *     voltron/rollout_utils.py:35,46) stays in the host wrapper.  Where info[b] > 0 the failed pivot's own L[i,i] is NaN,
 *     and so are out[b,0] and (with VOLT_WANT_GRAD) all of alpha[b,:] of the fp32 step; the other matrices of the batch
 *     are not touched by it, and nothing in the call waits out a hand-off time-out for it (tests/test_gpu_failed_pivot.py,
 *     every dispatch path).
 *   - Matrices are row-major fp32 (the reference is fp32 throughout; voltron/means/EWMA.py:37 even
 *     forces FloatTensor) or fp64 where a *_f64 twin exists.  `ld` = leading dimension in
 *     elements, `bs` = batch stride in elements.
 *   - "Working" matrices (A, Y) have dimension Np = volt_padded_n(N) (next multiple of 128); the
 *     padding is an identity block written by volt_prepare_*, so it contributes nothing to
 *     log-determinants, solves or traces.
 */
#ifndef VOLT_HIP_H
#define VOLT_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VOLT_TILE 128
/* flag bits of the `flags` / `ws_flags` arguments below */
#define VOLT_WANT_GRAD 1          /* volt_mll_step_*: also produce the gradient outputs (the triangular inverse) */
#define VOLT_WS_INITIALISED 2     /* the workspace passed went through its *_workspace_init_f32 for this shape */
#define VOLT_REFINE_ALPHA 4       /* volt_mll_step_f32 with VOLT_WANT_GRAD: one step of iterative refinement of alpha */

/* ---- introspection ------------------------------------------------------------------------ */
int volt_abi_version(void);                 /* bumps when a signature changes */
const char* volt_source_hash(void);         /* hash of the sources this binary was built from (volt_amd/build.py) */
int volt_padded_n(int n);                   /* next multiple of VOLT_TILE */

/* ---- a1: CumTrapz  (voltron/kernels/VolKernel.py:4-10) -------------------------------------
 * V[b,i] = sum_{m<=i} w_m * y[b,m],  w = dx with first and last halved, dx = x[b,1]-x[b,0].
 * If `square` != 0, y = vol*vol is formed first, as VolatilityKernel.forward does (:28).
 * Bit-exact with the reference's CPU path: products in fp32, running sum in fp64, every prefix
 * rounded to fp32 (that is what torch.cumsum does on fp32 CPU tensors).
 * vol [B,N] (batch stride bs_vol), x [N] shared (bs_x = 0) or [B,N]; V [B,N] contiguous. */
int volt_cumtrapz_f32(const float* vol, int64_t bs_vol, const float* x, int64_t bs_x,
                      float* V, int B, int N, int square, void* stream);
int volt_cumtrapz_f64(const double* vol, int64_t bs_vol, const double* x, int64_t bs_x,
                      double* V, int B, int N, int square, void* stream);

/* ---- a2: VolatilityKernel.forward gather  (voltron/kernels/VolKernel.py:30-33) --------------
 * K[b,i,j] = V[b, min(i,j)], full square, row-major.  Replaces arange/meshgrid/minimum (int64
 * [N,N] index rebuilt on the CPU every call) + advanced-index gather.  HBM-write bound. */
int volt_fill_f32(const float* V, float* K, int B, int N, int64_t ldk, int64_t bsk, void* stream);
int volt_fill_f64(const double* V, double* K, int B, int N, int64_t ldk, int64_t bsk, void* stream);

/* ---- a4: EWMA  (voltron/means/EWMA.py:20-37) --------------------------------------------------
 * out[b,t] = sum_{j<k} w[j] * padded[b,t+j], padded = k copies of y[b,0] then y[b,:]; t = 0..N, so
 * out is [B,N+1]: out[:, :-1] is the train mean, out[:, -1] the one-step-ahead mean.  The k taps
 * `w` (device, fp32) are computed by the host exactly as the reference does (:21-24).  Replaces
 * conv1d + the forced .type(torch.FloatTensor) host round trip (:37). */
int volt_ewma_f32(const float* y, int64_t bs_y, const float* w, int k, float* out, int B, int N,
                  void* stream);

/* ---- a5: GaussianLikelihood "K + sigma^2 I"  (gpytorch, called from train_utils.py:249) ------
 * A[b] = tril-tiles(K[b]) + sigma2[b] I, padded to Np with an identity block.  sigma2 may be NULL
 * (adds nothing: rollouts factor raw K, rollout_utils.py:35) and `jitter` is added on top of it
 * (psd_safe_cholesky retry).  A [B,Np,Np] with ld = Np. */
int volt_prepare_f32(const float* K, int64_t ldk, int64_t bsk, const float* sigma2, float jitter,
                     float* A, int B, int N, void* stream);

/* ---- a5/a6: batched Cholesky  (torch.linalg.cholesky via gpytorch; psd_safe_cholesky at
 * rollout_utils.py:35, VoltronGP.py:83, VoltMagpie.py:87) ------------------------------------
 * In-place lower Cholesky of A [B,Np,Np] (left-looking, 128-wide panels, fp32 MFMA; ONE launch per block
 * column: diagonal tile, panel tiles (update + solve), look-ahead).  Winv [B, Np/128, 128, 128] receives the
 * inverses of the diagonal blocks (used by the solves; while the call runs, the first word of each block is also
 * the hand-off flag between the diagonal workgroup and the panel tiles of its launch).  info [B] int32: 0, the
 * 1-based index of the first non-positive / NaN pivot, or INT_MIN for an internal hand-off time-out (never
 * expected).  Diagonal tiles come back with their strict upper triangle zeroed; tiles above the diagonal are
 * never touched. */
int volt_potrf_f32(float* A, float* Winv, int* info, int B, int Np, void* stream);
/* The same with caller scratch (256-byte aligned, volt_potrf_workspace_bytes(B, Np) bytes; 0 for B >= 32): fewer than 32
 * matrices do not fill the chip with whole tiles, and with the scratch the long products of a launch are cut into
 * K-slices (csrc/chol.hip: split-K below 3 matrices, the balanced schedule of csrc/sched.h for the late block columns
 * of 3..31) -- one 4096^2 matrix 4.4 -> 1.3 ms.  ws == NULL is volt_potrf_f32. */
size_t volt_potrf_workspace_bytes(int B, int Np);
/* Once per scratch buffer (and again should the caller have overwritten it): copies the launch-schedule table for
 * (B, Np) into its table region, asynchronously on `stream`.  Optional: the factorisation follows the table only when
 * the caller passes ws_flags = VOLT_WS_INITIALISED (and then checks its header on the device: info = INT_MIN + 1 for
 * scratch that does not hold it); ws_flags = 0 runs the table-free schedules (3 .. 64 matrices: 2-25 % slower in the
 * late block columns). */
int volt_potrf_workspace_init_f32(void* ws, size_t ws_bytes, int B, int Np, void* stream);
int volt_potrf_ws_f32(float* A, float* Winv, int* info, int B, int Np, void* ws, size_t ws_bytes, int ws_flags, void* stream);
/* volt_prepare_f32 + volt_potrf_ws_f32 in one: the factor of K + (sigma2 + jitter) I (K [B,N,N], row stride ldk, batch
 * stride bsk, lower triangle read; sigma2 [B] or NULL) lands in A [B,Np,Np], Np = volt_padded_n(N), without a copy-in
 * pass -- the tiles are read from K by the workgroups that update them (what torch.linalg.cholesky(K + s2 I) is to the
 * reference: gpytorch's MLL, psd_safe_cholesky at rollout_utils.py:35).  ws as for volt_potrf_ws_f32 (may be NULL). */
int volt_potrf_k_f32(const float* K, int64_t ldk, int64_t bsk, const float* sigma2, float jitter, float* A, float* Winv,
                     int* info, int B, int N, void* ws, size_t ws_bytes, int ws_flags, void* stream);

/* fp64 twins on v_mfma_f64_16x16x4_f64 (the reference keeps the caller's dtype, VolKernel.py:28-33; the
 * noise-free train block of rollout_utils.py:35 has condition number 1e6 (N = 400) .. 1e8 (N = 4096), beyond
 * fp32).  Same layout and semantics as the fp32 pair; sigma2 [B] and jitter are doubles. */
int volt_prepare_f64(const double* K, int64_t ldk, int64_t bsk, const double* sigma2, double jitter,
                     double* A, int B, int N, void* stream);
int volt_potrf_f64(double* A, double* Winv, int* info, int B, int Np, void* stream);
/* The same with caller scratch (256-byte aligned, volt_potrf_workspace_bytes_f64(B, Np) bytes -- a few KB of progress words,
 * 0 where the shape does not use them; nothing to initialise): small batches of long series run the whole factorisation as
 * ONE launch (csrc/batch64_step.hip) instead of three launches per block column.  ws == NULL is volt_potrf_f64. */
size_t volt_potrf_workspace_bytes_f64(int B, int Np);
int volt_potrf_ws_f64(double* A, double* Winv, int* info, int B, int Np, void* ws, size_t ws_bytes, void* stream);
/* volt_prepare_f64 + volt_potrf_ws_f64 in one, the fp64 twin of volt_potrf_k_f32: the factor of K + (sigma2 + jitter) I with K
 * [B,N,N] read in place (row stride ldk, batch stride bsk; only the lower triangle) -- where the shape runs as one launch the
 * tiles come straight from K and A [B,Np,Np] only receives L (no copy-in pass; the strictly upper tiles of A are then not
 * written).  ws as for volt_potrf_ws_f64 (may be NULL: prepare + the launch-per-column schedule). */
int volt_potrf_k_f64(const double* K, int64_t ldk, int64_t bsk, const double* sigma2, double jitter, double* A, double* Winv,
                     int* info, int B, int N, void* ws, size_t ws_bytes, void* stream);

/* ---- a5/a6: triangular solves with one right-hand side  (torch.cholesky_solve at
 * rollout_utils.py:36,44; gpytorch inv_quad) ------------------------------------------------
 * rhs/out [B,Np] contiguous (pad with zeros).  `scratch` [B,Np] elements.  lower: out = L^-1 rhs;
 * lower_t: out = L^-T rhs.  rhs and out may alias.  ONE launch per solve: one workgroup per 128-block,
 * chained through release/acquire flags kept in `scratch`.  A hand-off that does not arrive within ~3 s of WALL CLOCK
 * (s_memrealtime; never expected -- only a bug or a wedged device gets there) turns the affected blocks into NaN
 * instead of hanging AND sets the error word: after the call, ((const int*)scratch)[1] != 0 says the solve timed out. */
int volt_trsv_lower_f32(const float* A, const float* Winv, const float* rhs, float* out,
                        float* scratch, int B, int Np, void* stream);
int volt_trsv_lower_t_f32(const float* A, const float* Winv, const float* rhs, float* out,
                          float* scratch, int B, int Np, void* stream);
int volt_trsv_lower_f64(const double* A, const double* Winv, const double* rhs, double* out,
                        double* scratch, int B, int Np, void* stream);
int volt_trsv_lower_t_f64(const double* A, const double* Winv, const double* rhs, double* out,
                          double* scratch, int B, int Np, void* stream);

/* ---- a5: triangular inverse for the noise gradient  (replaces autograd cholesky_backward) ---
 * Y = L^-T (upper triangular, row-major [B,Np,Np]); tr(K_s^-1) = ||Y||_F^2.  The fp64 twin uses the tiles BELOW the
 * diagonal of Y as scratch: only the upper triangle (diagonal included) is meaningful on return. */
int volt_trtri_f32(const float* A, const float* Winv, float* Y, int B, int Np, void* stream);
int volt_trtri_f64(const double* A, const double* Winv, double* Y, int B, int Np, void* stream);
/* The fp64 inverse with caller scratch (round 6): ws of volt_trtri_workspace_bytes_f64(B, Np) bytes (a few KB of progress words,
 * nothing to initialise; 0 = this shape has no one-launch schedule) lets the whole inverse run as ONE launch -- the rows' tiles
 * chase each other inside it (csrc/batch64_step.hip) instead of two launches per block row: 8 x 4096 4.8 -> 3.4 ms.  ws == NULL,
 * or a shape beyond the gate: exactly volt_trtri_f64.  Same result to rounding (different summation order of a tile's K blocks:
 * none -- the tiles' arithmetic is the launch-per-row kernels'). */
size_t volt_trtri_workspace_bytes_f64(int B, int Np);
int volt_trtri_ws_f64(const double* A, const double* Winv, double* Y, int B, int Np, void* ws, size_t ws_bytes, void* stream);

/* ---- a7/a8: sequential posterior rollouts  (voltron/rollout_utils.py:57-93 + :6-53) ----------
 * Bordered-Cholesky engine: the shared train block of every sample's matrix enters through two scalars per series,
 * rho = u'K^-1u and tau = u'K^-1 r_tr (the host gets them in closed form or from the fp64 factorisation,
 * volt_amd/rollout_engine.py); this launch walks all H horizon steps for every sample path: the sample's bordered
 * factor grown row by row, EWMA-family mean of the appended point (mean_mode 0 ewma / 1 dewma / 2 tewma /
 * 3 meanrevert, EWMA.py; 4 = a mean that depends on x alone -- constant, linear, log-linear, as in
 * experiments/weather/GPGenerator.py:68-82 --: hist_e1 then holds its values at the H test points, [G,H], hist_y is
 * ignored but must be valid with k = 1), optional mean reversion (:41-42), jitter ladder of psd_safe_cholesky(pred_cov, jitter) (:46).
 * G series x S samples x H steps, H <= VOLT_ROLLOUT_MAX_H.
 *   scratch == NULL  append-only solve: for the volatility kernel the right-hand side prefix and the stored rows
 *                    are step-invariant, so w_s only grows by one entry per step; nothing is stored or re-read.
 *   scratch != NULL  (volt_rollout_scratch_bytes(G,S,H) bytes) full forward substitution against the stored packed
 *                    rows at every step -- bitwise the same paths, H^3/6 * 4 B streamed per path; the cross-check.
 * hist_* [G,k] are the last k values of the (padded) train series / its EMA / EMA(EMA); acc0 [G] the CumTrapz running
 * sum through the last train point; rho, tau, acc0 are fp64 (the kernel works with acc - rho, which fp32 operands
 * would cancel away).  pred_vol, z, samples [G,S,H]; info [G,S]: 0; +step (1-based) of the first non-positive pivot
 * of the per-sample factor (a local jitter was applied); -step if the predictive variance stayed <= 0 after the
 * jitter ladder (the reference's psd_safe_cholesky raises NotPSDError there). */
#define VOLT_ROLLOUT_MAX_H 1024
size_t volt_rollout_scratch_bytes(int G, int S, int H);
int volt_rollout_bordered_f32(const double* rho, const double* tau, const double* acc0, const float* dx,
                              const float* hist_y, const float* hist_e1, const float* hist_e2,
                              const float* ema_prev, const float* mr_latent, const float* latent,
                              const float* w, const float* pred_vol, const float* z, float* samples,
                              float* scratch, int* info, int G, int S, int H, int k, int mean_mode,
                              int use_theta, float theta, float mr_theta, float jitter, void* stream);

/* nonvol_rollouts (voltron/rollout_utils.py:95-115): rollouts of a GP whose kernel is the same for every sample.
 * e [G,S,H] is the GP part of every path (posterior mean offset + correlated noise, computed by the caller from one
 * shared factorisation: e = c + M z, see volt_amd/rollout_engine.py); this adds the moving-average mean of the
 * sample's own stacked series, sequentially in the horizon: samples[.., idx] = mean_s(idx) + e[.., idx].
 * hist_* [G,k], ema_prev / mr_latent [G], w [k] and mean_mode as in volt_rollout_bordered_f32. */
int volt_rollout_shared_f32(const float* hist_y, const float* hist_e1, const float* hist_e2, const float* ema_prev,
                            const float* mr_latent, const float* w, const float* e, float* samples, int G, int S,
                            int H, int k, int mean_mode, float mr_theta, void* stream);

/* One-launch Adam step over a list of fp32 parameter tensors (train_utils.py:43,100,166,238,291 build
 * torch.optim.Adam(lr=0.1); same arithmetic, amsgrad off, no weight decay).  slots: DEVICE array of nslots records
 * {float* p; float* m; float* v; int64 end} (end = one past the tensor's last element in the flattened index space,
 * ascending); total = the last end; grad [total]: the gradients flattened in slot order.  state: 2 DEVICE ints {step
 * count t, arrival ticket}, zero before the first step; t is read and advanced on the device, so the launch can be
 * replayed from a graph. */
int volt_adam_step_f32(const void* slots, int nslots, long long total, const float* grad, float lr, float beta1, float beta2,
                       float eps, int* state, void* stream);

/* ---- a5: MLL + gradient  (ExactMarginalLogLikelihood + loss.backward(), train_utils.py:249-250)
 * One "step" of SURVEY 8(d) with K resident:
 *     A = K + sigma2 I -> potrf -> Y = L^-T -> z = Y'r, alpha = Y z
 *     out[b,0] = mll   = -1/2 (z'z + logdet + N log 2pi) / N
 *     out[b,1] = d mll / d sigma2 = 1/2 (alpha'alpha - tr K_s^-1) / N
 *     out[b,2] = z'z   out[b,3] = logdet   out[b,4] = tr K_s^-1   out[b,5] = alpha'alpha
 *     alpha[b,:] (= K_s^-1 r;  d mll / d mean = alpha / N)
 * resid [B,N] = y - mean(x).  `flags`: VOLT_WANT_GRAD -- without it the triangular inverse is skipped (forward
 * solve instead) and out[b,1], out[b,4], out[b,5] and alpha are not written; VOLT_WS_INITIALISED -- see below;
 * VOLT_REFINE_ALPHA (with VOLT_WANT_GRAD, opt-in) -- alpha <- alpha + K_s^-1 (r - K_s alpha) with the residual formed
 * against the caller's K in fp64 accumulation (BOTH triangles of K are read) and the correction solved through the
 * fp32 factor; out[b,0], out[b,1], out[b,2], out[b,5] are recomputed from the refined alpha and out[b,7] = 1.  Takes
 * alpha from the fp32 floor (cond * eps: 1e-5 .. 4e-5 of its max at sigma^2 = 1e-4, N = 4096, what the reference's own
 * fp32 path has) to < 1e-6 for one more pass over K and two triangular solves (+8 % of a step at 64 x 4096).
 * workspace: volt_mll_workspace_bytes(B,N,want_grad) bytes, 256-byte aligned. */
size_t volt_mll_workspace_bytes(int B, int N, int want_grad);
/* Once per workspace (and again should the caller have overwritten it), asynchronously on `stream`: copies the
 * launch-schedule table for this shape into the workspace (3 .. 31 series), and for short series (want_grad = 1, N <= 1024:
 * up to 40 series of N <= 512, 16 of N = 1024, 64 of N <= 256) writes the state of the ONE-LAUNCH step: a header, a step counter and the
 * flags its workgroups hand tiles on with (for ONE series of 1025 .. 4096 points also the list of its pieces, and the
 * workspace holds the slabs of their K-slices) -- volt_mll_step_f32 then enqueues one kernel for the whole step instead of
 * eleven (the counter lives on the device, so the launch replays from a hipGraph as it is).  Optional, like
 * volt_potrf_workspace_init_f32: the step uses what the init wrote only when the caller passes VOLT_WS_INITIALISED in
 * `flags` -- the library keeps no record of workspaces (rounds 2-3 recognised them by address) -- and every launch that
 * follows a table or the state checks the header there first: a region that does not hold what the init wrote (never
 * initialised, overwritten, or freed and handed out again) is reported (info = INT_MIN + 1), never followed.  Without the
 * flag the step runs the launch-per-column path.
 * (The workspace of volt_gpcv_step_f32 begins with an MLL workspace: same call, want_grad = 1.) */
int volt_mll_workspace_init_f32(void* workspace, int B, int N, int want_grad, void* stream);
int volt_mll_step_f32(const float* K, int64_t ldk, int64_t bsk, const float* resid,
                      const float* sigma2, float jitter, float* out /*[B,8]*/, float* alpha /*[B,N]*/,
                      int* info, void* workspace, int B, int N, int flags, void* stream);

/* The same step in double precision for double-precision models (the reference keeps the caller's dtype,
 * voltron/kernels/VolKernel.py:28-33; gpytorch computes log_prob in it): K, resid, sigma2, out [B,8], alpha [B,N] are
 * doubles; volt_potrf_f64 / volt_trsv_*_f64 / volt_trtri_f64 underneath.  Agreement with an fp64 LAPACK evaluation of
 * the same formulas: 1e-10 relative at N <= 1024, 1e-8 at N = 4096 (tests). */
size_t volt_mll_workspace_bytes_f64(int B, int N, int want_grad);
int volt_mll_step_f64(const double* K, int64_t ldk, int64_t bsk, const double* resid,
                      const double* sigma2, double jitter, double* out /*[B,8]*/, double* alpha /*[B,N]*/,
                      int* info, void* workspace, int B, int N, int want_grad, void* stream);

/* Dense gradient of the MLL wrt the covariance, for kernels whose parameters enter K elementwise (the fractional
 * Brownian-motion prior of the vol forecaster, voltron/models/BMGP.py:15-16 + kernels/FBMKernel.py:38-59):
 *     grad_K[b] = d mll_b / d K_b = 1/2 (alpha alpha' - K_s^-1) / N,   K_s^-1 = Y Y' on the structured GEMM.
 * Call after volt_mll_step_f32(want_grad = 1) on the same workspace; scratch [B, Np, Np] floats, 16-byte aligned. */
int volt_mll_grad_k_f32(void* mll_workspace, const float* alpha, float* scratch, float* grad_K, int B, int N,
                        void* stream);

/* ---- f4: GPCV volatility extraction (LearnGPCV, voltron/train_utils.py:15-67) --------------------
 * Structured batched GEMM on the fp32 MFMA core, C = alpha A B^T + beta C, row-major, K contiguous in
 * both operands.  uplo_* : 0 dense, 1 lower, 2 upper, at 128-tile granularity: for A (B) it restricts the
 * k-blocks read for a row-block, for C it selects the tiles written.  M, N, K multiples of 128;
 * lda/ldb multiples of 4, A and B 16-byte aligned. */
int volt_gemm_nt_f32(const float* A, int64_t lda, int64_t bsa, int uplo_a, const float* B, int64_t ldb,
                     int64_t bsb, int uplo_b, float* C, int64_t ldc, int64_t bsc, int uplo_c, float alpha,
                     float beta, int batch, int M, int N, int K, void* stream);

/* One ELBO + gradient evaluation of the variational GP whose inducing points are its inputs
 * (single_task_variational_gp.py:69-122 with use_whitened_var_strat=False; likelihood
 * volatility_likelihood.py:42-50, "exp" parameterisation; VariationalELBO call train_utils.py:44,51-54):
 *     q(u) = N(m, Lq Lq'),  prior N(mu, K + jitter I),
 *     ell = sum_i sum_k w_k log N(y_i; 0, max(exp(m_i + sqrt(2 var_i) x_k), min_scale)),  var_i = max(sum_j Lq_ij^2, min_var)
 *     KL  = 1/2 (tr(K^-1 S) + r'K^-1 r - N + logdet K - logdet S),   r = m - mu  (passed in as `resid`)
 * K [B,N,N] (ldk, bsk) without jitter; m, resid, y [B,N]; Lq [B,N,N] contiguous (upper triangle ignored);
 * gh_x, gh_w [Q] Gauss-Hermite nodes and weights / sqrt(pi).
 *     F   = w_ell ell - w_kl KL      (VariationalELBO: w_ell = 1/N, w_kl = beta/num_data)
 *     out[b,0..11] = ell, KL, r'K^-1 r, logdet K, logdet S, tr(K^-1 S), tr K^-1, |K^-1 Lq|_F^2, |K^-1 r|^2,
 *                    F, jitter, 0
 *     grad_m, grad_mu [B,N], grad_Lq [B,N,N]: gradients of F;  grad_K [B,N,N] (nullable) = dF/dK.
 * info[b] LAPACK-style for the factorisation of K + jitter I.  A series whose factorisation fails (info[b] > 0) is a
 * reported result, not an error return: its KL and F (out[b,1], out[b,9]) are not finite and grad_m[b,:], grad_mu[b,:] are
 * NaN throughout (the MLL step's contract for out[b,0] and alpha, carried on); its grad_Lq[b] and grad_K[b] have no meaning;
 * out[b,0] = ell and out[b,4] = logdet S, which do not involve K, are the series' own.  The other series of the batch are
 * not touched by it, and the workspace needs nothing before its next step (tests/test_gpu_gpcv_dense_edges.py).
 * workspace: volt_gpcv_workspace_bytes. */
size_t volt_gpcv_workspace_bytes(int B, int N, int want_dk);
int volt_gpcv_step_f32(const float* K, int64_t ldk, int64_t bsk, float jitter, const float* resid, const float* m,
                       const float* Lq, const float* y, const float* gh_x, const float* gh_w, int Q, float min_var,
                       float min_scale, float w_ell, float w_kl, float* out, float* grad_m, float* grad_mu,
                       float* grad_Lq, float* grad_K, int* info, void* workspace, int B, int N, int ws_flags, void* stream);

/* The same step for the copula-process ("cv") parameterisation of the likelihood -- the call site it replaces is
 * volatility_likelihood.py:43-51 under the quadrature of its expected_log_prob (:53-58):
 *     scale(f) = sum_k a_k log(1 + exp(b_k f + c_k)),  k < Kc,   y_i | f ~ N(0, max(scale(f), min_scale))
 * abc [B,3,Kc]: the TRANSFORMED a, b, c of every series (rows a, b, c; the constraints' chain rule is the caller's).
 * Everything else is volt_gpcv_step_f32's: the same arguments, out[b,0..11], gradients and info with the same meaning;
 *     grad_abc [B,3,Kc] = dF/d(a,b,c) = w_ell d ell / d(a,b,c)      (the KL does not see the likelihood).
 * The row sums behind grad_abc are reduced in a fixed order (per-workgroup partials, then one pass): no float atomics,
 * the step is bitwise repeatable.  1 <= Kc <= VOLT_GPCV_CV_K_MAX, otherwise a negative argument code (Kc is argument 10).
 * workspace: volt_gpcv_cv_workspace_bytes(B, N, want_dk, Kc) bytes (0 if Kc is out of range); it begins with the
 * workspace of volt_gpcv_step_f32 for the same (B, N, want_dk), initialised the same way. */
#define VOLT_GPCV_CV_K_MAX 8
size_t volt_gpcv_cv_workspace_bytes(int B, int N, int want_dk, int Kc);
int volt_gpcv_cv_step_f32(const float* K, int64_t ldk, int64_t bsk, float jitter, const float* resid, const float* m,
                          const float* Lq, const float* y, const float* abc, int Kc, const float* gh_x, const float* gh_w,
                          int Q, float min_var, float min_scale, float w_ell, float w_kl, float* out, float* grad_m,
                          float* grad_mu, float* grad_Lq, float* grad_K, float* grad_abc, int* info, void* workspace,
                          int B, int N, int ws_flags, void* stream);

/* ---- Multi-task GPCV  (MultitaskVariationalGP, voltron/models/multi_task_variational_gp.py:11-146; the trainer is this
 * library's: the reference has none) ------------------------------------------------------------------------------------
 * One ELBO + gradient evaluation of the Kronecker variational GP over T <= 64 series that share the N inducing points
 * (= the inputs).  Element (n,t) of vec F at n*T + t.
 *     q(F) = N(M, S_x (x) S_t),  S_x = Lx Lx', S_t = Lt Lt'  (Lx [N,N], Lt [T,T]: the parts above the diagonals are ignored)
 *     p(F) = N(mu, (K + jitter I) (x) K_t),  mu[n,t] = c[t],  K_t = f f' + diag(softplus(raw_var)),  f = covar_factor [T]
 *     ell  = sum_nt sum_k w_k log N(y_nt; 0, max(exp(M_nt + sqrt(2 var_nt) x_k), min_scale)),
 *            var_nt = max((sum_k Lx_nk^2)(sum_s Lt_ts^2), min_var)
 *     KL   = 1/2 [tau_x tau_t + q - N T + T logdet K + N logdet K_t - T logdet S_x - N logdet S_t],
 *            tau_x = tr(K^-1 S_x), tau_t = tr(K_t^-1 S_t), A = K^-1 (M - mu), q = tr(K_t^-1 (M - mu)'A)
 *     F    = w_ell ell - w_kl KL      (VariationalELBO over the [N,T] event: w_ell = 1/N, w_kl = beta/num_data)
 * K [N,N] (ldk) without jitter; M, y [N,T], Lx [N,N], Lt [T,T] contiguous; c, covar_factor, raw_var [T];
 * gh_x, gh_w [Q] Gauss-Hermite nodes and weights / sqrt(pi).
 *     out[0..15] = ell, KL, q, logdet K, logdet K_t, logdet S_x, logdet S_t, tau_x, tau_t, tr K^-1, |K^-1 Lx|_F^2,
 *                  tr(K_t^-1 A'A), F, jitter, 0, 0
 *     grad_M [N,T], grad_c [T], grad_Lx [N,N], grad_Lt [T,T], grad_covar_factor [T], grad_raw_var [T]: gradients of F;
 *     grad_K [N,N] (nullable) = dF/dK.
 * K + jitter I is factored ONCE (volt_mll_step_f32 at B = 1); the T solves are two NT products with the T rows in one
 * 128-row tile.  No host synchronisation, no allocation, every reduction in a fixed order (bitwise repeatable); the launch
 * sequence replays from a hipGraph on one stream.
 * info[0]: LAPACK-style for K + jitter I (or an internal error of the factorisation, as for volt_mll_step_f32);
 * info[1]: 0, or the 1-based index of the first non-positive pivot of K_t;  info[2]: 1 if F came out non-finite (NaN or
 * inf in the inputs, or a failed factorisation), else 0.  info holds 3 ints.
 * workspace: volt_gpcv_mt_workspace_bytes(N, T, want_dk) bytes (0 if T is out of range), 256-byte aligned; it begins with
 * an MLL workspace for (B = 1, N, want_grad = 1): volt_mll_workspace_init_f32 + VOLT_WS_INITIALISED in ws_flags as there. */
size_t volt_gpcv_mt_workspace_bytes(int N, int T, int want_dk);
int volt_gpcv_mt_step_f32(const float* K, int64_t ldk, float jitter, const float* M, const float* c, const float* Lx,
                          const float* Lt, const float* covar_factor, const float* raw_var, const float* y,
                          const float* gh_x, const float* gh_w, int Q, float min_var, float min_scale, float w_ell,
                          float w_kl, float* out, float* grad_M, float* grad_c, float* grad_Lx, float* grad_Lt,
                          float* grad_covar_factor, float* grad_raw_var, float* grad_K, int* info, void* workspace, int N,
                          int T, int ws_flags, void* stream);

/* The same step for the copula-process ("cv") likelihood with ONE WARP PER TASK -- the call sites it replaces are
 * multi_task_variational_gp.py:58-69 and the batched likelihood of volatility_likelihood.py:19-22,45-47 ([T,K] parameters):
 *     scale_t(f) = sum_k a_tk log(1 + exp(b_tk f + c_tk)),  k < Kc,   y_nt | f ~ N(0, max(scale_t(f), min_scale))
 * abc [T,3,Kc]: the TRANSFORMED a, b, c of every task (rows a, b, c; the constraints' chain rule is the caller's).
 * Everything else is volt_gpcv_mt_step_f32's: the same arguments, out[0..15], gradients and info[0..2] with the same meaning
 * (a NaN in abc shows as info[2] = 1), the same launches after the quadrature pass;
 *     grad_abc [T,3,Kc] = dF/d(a,b,c) = w_ell d ell / d(a,b,c)      (the KL does not see the likelihood).
 * The sums behind grad_abc are per-workgroup partials added in one fixed-order fp64 pass: no float atomics, bitwise
 * repeatable.  1 <= Kc <= VOLT_GPCV_CV_K_MAX (defined with volt_gpcv_cv_step_f32 above).
 * Argument codes (the negative return names the first offending argument, counted from 1 as for every entry):
 *     1 K, 2 ldk, 4 M, 5 c, 6 Lx, 7 Lt, 8 covar_factor, 9 raw_var, 10 y, 11 abc, 12 Kc, 13 gh_x, 14 gh_w, 15 Q,
 *     20 out, 21 grad_M, 22 grad_c, 23 grad_Lx, 24 grad_Lt, 25 grad_covar_factor, 26 grad_raw_var, (27 grad_K is nullable),
 *     28 grad_abc, 29 info, 30 workspace (null or not 256-byte aligned), 31 N, 32 T.  No launch is made before all pass.
 * workspace: volt_gpcv_mt_cv_workspace_bytes(N, T, want_dk, Kc) bytes (0 if T or Kc is out of range): the workspace of
 * volt_gpcv_mt_step_f32 for the same (N, T, want_dk), unchanged, with the partials [T, ceil(N/16), 3 Kc] appended;
 * initialised the same way. */
size_t volt_gpcv_mt_cv_workspace_bytes(int N, int T, int want_dk, int Kc);
int volt_gpcv_mt_cv_step_f32(const float* K, int64_t ldk, float jitter, const float* M, const float* c, const float* Lx,
                             const float* Lt, const float* covar_factor, const float* raw_var, const float* y,
                             const float* abc, int Kc, const float* gh_x, const float* gh_w, int Q, float min_var,
                             float min_scale, float w_ell, float w_kl, float* out, float* grad_M, float* grad_c,
                             float* grad_Lx, float* grad_Lt, float* grad_covar_factor, float* grad_raw_var, float* grad_K,
                             float* grad_abc, int* info, void* workspace, int N, int T, int ws_flags, void* stream);

/* ---- Kronecker multi-task vol forecaster  (MultitaskBMGP, voltron/models/BMGP.py:30-56: botorch KroneckerMultiTaskGP with
 * MultitaskKernel(BMKernel(), T) and MultitaskGaussianLikelihood(T); built by the batched constructors VoltMagpie.py:51-55,
 * VoltronGP.py:46-50, Volt.py:67-71, trained through ExactMarginalLogLikelihood + loss.backward()).
 * Sigma = K_x (x) K_t + I_N (x) D, element (n,t) of vec Y at n*T + t;  K_x = vol M, M = min(x_i,x_k), vol = sigmoid(raw_vol);
 * K_t = F F' + diag(softplus(raw_var)), F = covar_factor [T] (rank 1);  d_t = softplus(raw_task_noises_t) + 1e-4 +
 * softplus(raw_noise) + 1e-4;  mu[n,t] = -1/2 vol^2 x_n K_t[t,t];  mll = log N(vec Y; vec mu, Sigma) / (N T).
 * With S = D^-1/2 K_t D^-1/2 = Q Lambda Q', W = D^-1/2 Q, kappa_j = vol lambda_j, the MLL is T exact-GP steps over ONE M:
 *     volt_kron_prologue_*  ->  volt_mll_step_* (K = M for every j: ldk = N, bsk = 0 or M repeated; resid = r [T,N];
 *                               sigma2 = 1 / kappa [T]; B = T, VOLT_WANT_GRAD)  ->  volt_kron_epilogue_*
 * No host synchronisation in between: the three calls replay from a hipGraph.  T <= 64.  All parameters are device
 * pointers in the step's dtype; the eigendecomposition and the algebra around the step run in fp64 in either variant. */

/* Batched symmetric eigensolver, T <= 64: S [B,T,T] (batch stride bss >= T*T, contiguous rows) -> lam [B,T] ascending,
 * Q [B,T,T] row-major with the eigenvectors as columns (S Q = Q diag(lam)).  One workgroup per matrix, parallel cyclic
 * Jacobi in LDS; info[b] = sweeps used (>= 0), or -1 if 30 sweeps did not converge.  Replaces the torch.linalg.eigh that
 * gpytorch's KroneckerProductLinearOperator runs on the task covariance. */
int volt_syev_small_f64(const double* S, int64_t bss, double* lam, double* Q, int* info, int B, int T, void* stream);
/* Bytes of the caller's `state` of the prologue (doubles: vol, Lambda [T], d [T], W [T,T], Q [T,T]); 0 if T is out of range. */
size_t volt_kron_state_bytes(int T);
/* From the raw parameters (raw_vol [1], covar_factor [T], raw_var [T], raw_task_noises [T], raw_noise [1]), x [N] and Y [N,T]
 * (row stride ldy, contiguous rows): resid [T,N] = r_j = (R W)_j / sqrt(kappa_j), R = Y - mu; sigma2 [T] = 1 / kappa_j;
 * state (volt_kron_state_bytes(T)); info[0] = sweeps of the eigensolver or -1.  One launch. */
int volt_kron_prologue_f32(const float* raw_vol, const float* covar_factor, const float* raw_var, const float* raw_task_noises,
                           const float* raw_noise, const float* x, const float* Y, int64_t ldy, float* resid, float* sigma2,
                           double* state, int* info, int N, int T, void* stream);
int volt_kron_prologue_f64(const double* raw_vol, const double* covar_factor, const double* raw_var,
                           const double* raw_task_noises, const double* raw_noise, const double* x, const double* Y, int64_t ldy,
                           double* resid, double* sigma2, double* state, int* info, int N, int T, void* stream);
/* From the step's out [T,8] and alpha [T,N] (with the prologue's resid and state): res [3 + 3T] =
 *     mll, d mll / d raw_vol, d mll / d raw_noise, d mll / d covar_factor [T], d / d raw_var [T], d / d raw_task_noises [T].
 * One launch (one workgroup: the reductions over N, then T x T algebra). */
int volt_kron_epilogue_f32(const float* raw_vol, const float* covar_factor, const float* raw_var, const float* raw_task_noises,
                           const float* raw_noise, const float* x, const float* resid, const float* out, const float* alpha,
                           const double* state, float* res, int N, int T, void* stream);
int volt_kron_epilogue_f64(const double* raw_vol, const double* covar_factor, const double* raw_var,
                           const double* raw_task_noises, const double* raw_noise, const double* x, const double* resid,
                           const double* out, const double* alpha, const double* state, double* res, int N, int T,
                           void* stream);

/* The same step around the LINEAR-TIME chain solver (MultitaskBMGP(solver="linear"); no N x N matrix anywhere):
 *     volt_kron_prologue_warm_*  ->  volt_bm_step_* (x, vol = 1 [T], sigma2 = 1 / kappa [T], resid = r [T,N]; B = T,
 *                                    VOLT_WANT_GRAD)  ->  volt_kron_epilogue_ws_*
 * Stream order is the only synchronisation between and inside the calls: no atomics, no hand-off words, no workgroup waits
 * for another; every sum has a fixed order that does not depend on the device, results are bitwise repeatable, and the
 * sequence replays from a hipGraph.  T <= 64, N >= 1, 64-bit indices, fp64 arithmetic, I/O in the step's dtype.
 *
 * volt_kron_prologue_warm_*: the prologue's arguments, outputs and `state` layout (volt_kron_state_bytes), in TWO launches:
 * one workgroup decomposes S, then a grid over chunks of N writes resid.  The eigensolver starts from the Q the previous
 * call left in `state` (A0 = Q' S Q, same rotation criterion and sweep cap; Q is re-orthonormalised by one Newton-Schulz
 * step on entry, so it does not drift over a training run) when the stamp in the header's spare doubles says that Q is a
 * converged, finite decomposition for this T, and cold -- bitwise what volt_kron_prologue_* computes -- otherwise:
 *     state[1] = stamp (0: the next call starts cold; written by every call, cleared when the solve hit the sweep cap or
 *                produced a non-finite value);  state[2] = 1 if THIS call started warm, else 0;  state[3..7] unused.
 * The caller zeroes `state` once (or state[1]) before the first call; volt_kron_prologue_* does not touch state[1..7], so
 * the two prologues may share a state.  info[0] = sweeps used (>= 0), or -1.  If the decomposition holds a non-finite value
 * (NaN / inf in a parameter) sigma2 is NaN in every entry, so that the step reports all T directions in its info.
 * Argument errors (before any launch, in the order of their numbers; those of volt_kron_prologue_*): -1 raw_vol,
 * -2 covar_factor, -3 raw_var, -4 raw_task_noises, -5 raw_noise, -6 x, -7 Y NULL; -8 ldy < T; -9 resid, -10 sigma2, -11 state,
 * -12 info NULL; -13 N < 1; -14 T out of range.
 *
 * volt_kron_epilogue_ws_*: the epilogue's arguments and result, with the reductions over N spread over workgroups: launch 1,
 * one workgroup per slice of 256 columns of N (a compile-time constant), writes its partial sums (2 T^2 + T doubles) to
 * `workspace`; launch 2, one workgroup, adds them in slice order and runs the epilogue's T x T algebra (one device function
 * with volt_kron_epilogue_*).  workspace: volt_kron_epilogue_workspace_bytes(N, T) bytes (0 if N < 1 or T is out of range),
 * 256-byte aligned, caller-owned, no initialisation.
 * Argument errors (before any launch): -1 .. -11 the pointers raw_vol .. res in argument order; -12 workspace NULL or not
 * 256-byte aligned; -13 N < 1; -14 T out of range. */
int volt_kron_prologue_warm_f32(const float* raw_vol, const float* covar_factor, const float* raw_var,
                                const float* raw_task_noises, const float* raw_noise, const float* x, const float* Y, int64_t ldy,
                                float* resid, float* sigma2, double* state, int* info, int N, int T, void* stream);
int volt_kron_prologue_warm_f64(const double* raw_vol, const double* covar_factor, const double* raw_var,
                                const double* raw_task_noises, const double* raw_noise, const double* x, const double* Y,
                                int64_t ldy, double* resid, double* sigma2, double* state, int* info, int N, int T, void* stream);
size_t volt_kron_epilogue_workspace_bytes(int N, int T);
int volt_kron_epilogue_ws_f32(const float* raw_vol, const float* covar_factor, const float* raw_var, const float* raw_task_noises,
                              const float* raw_noise, const float* x, const float* resid, const float* out, const float* alpha,
                              const double* state, float* res, void* workspace, int N, int T, void* stream);
int volt_kron_epilogue_ws_f64(const double* raw_vol, const double* covar_factor, const double* raw_var,
                              const double* raw_task_noises, const double* raw_noise, const double* x, const double* resid,
                              const double* out, const double* alpha, const double* state, double* res, void* workspace, int N,
                              int T, void* stream);

/* ---- Path summaries  (voltron/option_utils.py:26-52 ECDF / Pricer; the weather calibration notebook's per-step ECDF, mean and
 * std) -- what every consumer of a rollout computes on the host after samples.cpu(), here on the device.
 * For every series g and horizon step h the S values samples[g*bs + s*ld + h] (ld >= H: any slice of the horizon is a view)
 * are sorted and reduced; G >= 1, 1 <= S <= VOLT_SUMMARY_MAX_S, H >= 1.  With VOLT_SUMMARY_EXP in `flags` every statistic is
 * that of v = exp(x), the exponential taken in fp64 from the fp32 sample; without it v = x.  All arithmetic after the sort is
 * fp64; the outputs are fp32 (counts int32) and keep H contiguous:
 *     moments [G,4,H]  mean, unbiased standard deviation (two-pass; NaN for S = 1), min, max
 *     quant   [G,Q,H]  for the levels q [Q] (DEVICE, fp64): pos = q (S-1), lo = floor(pos), v_(lo) + (v_(lo+1) - v_(lo)) (pos - lo)
 *                      over the sorted column (torch.quantile's default "linear" rule, in fp64).  Q may be 0.
 *     counts  [G,3,H]  n_nan = NaN samples;  n_lt = #{v < truth} (ECDF's numerator);  n_le = #{v <= truth}.  truth [G,H] is in
 *                      value units and may be NULL; where it is NaN or absent n_lt = n_le = -1.
 *     crps    [G,H]    mean |v_i - y| - S^-2 sum_i (2i - S - 1) v_(i), i 1-based over the sorted column
 *                      (= mean |v - y| - 1/2 mean |v_i - v_j|); NaN where truth is.
 *     call, put [G,M,H] for strikes [G,M]: mean max(v - K, 0), mean max(K - v, 0).  M may be 0.
 * A column with any NaN sample reports n_nan, NaN in every float output and n_lt = n_le = -1.  Infinities are ordinary values
 * of the ordering.  moments, counts and crps may be NULL (not written).
 * scratch: volt_path_summary_scratch_bytes(G,S,H) bytes (G H round_up(S, 64) floats: the transposed samples; 0 for a shape out
 * of range), 256-byte aligned, caller-owned.  Two launches, no host synchronisation, no allocation, no atomics: every
 * reduction has a fixed order, results are bitwise repeatable, and the call replays from a hipGraph.
 * Argument errors (before any launch): -1 samples NULL; -2 ld < H; -4 G < 1 (or G H beyond a grid); -5 S out of range;
 * -6 H < 1; -7 unknown flag bits; -8 Q > 0 and q NULL; -9 Q < 0; -11 M > 0 and strikes NULL; -12 M < 0; -14 Q > 0 and quant
 * NULL; -17 / -18 M > 0 and call / put NULL; -19 scratch NULL or not 256-byte aligned; -20 scratch_bytes too small. */
#define VOLT_SUMMARY_MAX_S 32768
#define VOLT_SUMMARY_EXP 1        /* flag bit of volt_path_summary_f32 */
size_t volt_path_summary_scratch_bytes(int G, int S, int H);
int volt_path_summary_f32(const float* samples, int64_t ld, int64_t bs, int G, int S, int H, int flags,
                          const double* q, int Q, const float* truth, const float* strikes, int M,
                          float* moments, float* quant, int* counts, float* crps, float* call, float* put,
                          void* scratch, size_t scratch_bytes, void* stream);

/* ---- Linear-time Brownian-motion solver  (BMGP, voltron/models/BMGP.py:9-28, with solver="linear": the vol forecaster's
 * MLL step and posterior solve without any N x N matrix).  K = v M, M = min(x_i, x_k) over a grid 0 <= x_0 < x_1 < ..
 * shared by the batch.  With D the first-difference operator D M D' = diag(delta) (delta_0 = x_0, delta_i = x_i - x_{i-1}),
 * so A = v M + s I = D^-1 T D^-T with T = v diag(delta) + s D D' tridiagonal and SPD whenever s > 0 (also at x_0 = 0,
 * where M itself is singular).  Two O(N) sweeps over T = L diag(d) L' give everything the dense step returns
 * (csrc/bm.hip has the recurrences); the arithmetic is fp64 whatever the I/O type.
 *     volt_bm_step_*:  x [N], vol [B] (v > 0), sigma2 [B] (s > 0), resid [B,N]  ->  out [B,8], alpha [B,N], info [B]
 *         out[b,0..5] exactly as volt_mll_step_*: mll, d mll / d sigma2, r'A^-1 r, logdet, tr A^-1, alpha'alpha;
 *         out[b,6] = sigma2[b], out[b,7] = vol[b] (the parameters the step used).  `flags`: VOLT_WANT_GRAD -- without it the backward sweep is skipped and
 *         out[b,1], out[b,4], out[b,5] and alpha are not written (workspace and alpha may then be NULL).
 *     volt_bm_solve_*: X [B,N,H] = A_b^-1 R_b for R [B,N,H], H contiguous (the posterior's solve: R = K_t*).
 * info[b]: 0, or i + 1 for the first pivot d_i that is not a positive finite number (s = 0 at x_0 = 0, a NaN parameter);
 * logdet and mll are then NaN.  A NaN in resid leaves info at 0 and comes out as NaN in out and alpha.
 * workspace: volt_bm_workspace_bytes(B,N,H) bytes (the step: H = 1), 256-byte aligned: (1 + H) B N doubles, the pivots'
 * reciprocals and the forward sweep's z.  Nothing is O(N^2).  The step is ONE launch, the solve two; no host
 * synchronisation, no allocation, no atomics: every sum has a fixed order, results are bitwise repeatable, and the calls
 * replay from a hipGraph.  Any B >= 1, N >= 1, H >= 1; indices are 64-bit.
 * Argument errors (before any launch, checked in the order of their numbers), step: -1 x, -2 vol, -3 sigma2, -4 resid, -5 out NULL; -6 alpha NULL with
 * VOLT_WANT_GRAD; -7 info NULL; -8 workspace NULL or not 256-byte aligned with VOLT_WANT_GRAD; -9 B < 1; -10 N < 1;
 * -11 unknown flag bits.  Solve: -1 x, -2 vol, -3 sigma2, -4 R, -5 X, -6 info NULL; -7 workspace NULL or misaligned;
 * -8 B < 1; -9 N < 1; -10 H < 1 (or B H beyond a grid). */
size_t volt_bm_workspace_bytes(int B, int N, int H);
int volt_bm_step_f32(const float* x, const float* vol, const float* sigma2, const float* resid, float* out /*[B,8]*/,
                     float* alpha /*[B,N]*/, int* info, void* workspace, int B, int N, int flags, void* stream);
int volt_bm_step_f64(const double* x, const double* vol, const double* sigma2, const double* resid, double* out /*[B,8]*/,
                     double* alpha /*[B,N]*/, int* info, void* workspace, int B, int N, int flags, void* stream);

/* The same step for the volatility-kernel data model (VoltronGP / VoltMagpie / Volt with data_solver="linear"):
 * K_b[i,k] = V_b[min(i,k)], every series on its OWN grid V_b = CumTrapz(vol_b^2, x), scale 1.  V [B,N] with batch stride
 * `bsv` in elements (bsv >= N, or bsv = 0: one grid [N] shared by the batch); each row non-decreasing with V_0 >= 0 (the
 * caller's contract, not checked per step; an increment of 0 is legal, T stays SPD through sigma2 > 0).  delta_i =
 * V_i - V_{i-1} is formed in fp64 from the values as stored, so the step factors exactly the matrix a dense step on
 * volt_fill_*(V) factors.  out[b,0..6], alpha, info, flags and the workspace (volt_bm_workspace_bytes(B, N, 1)) mean what
 * they mean for volt_bm_step_*; out[b,7] = 1.  One launch, fp64 arithmetic, no atomics, bitwise repeatable, replays from
 * a hipGraph, 64-bit indices, nothing O(N^2).
 * Argument errors: -1 V NULL; -2 bsv < 0 or 0 < bsv < N; -3 sigma2, -4 resid, -5 out NULL; -6 alpha NULL with VOLT_WANT_GRAD;
 * -7 info NULL; -8 workspace NULL or not 256-byte aligned with VOLT_WANT_GRAD; -9 B < 1; -10 N < 1; -11 unknown flag bits. */
int volt_vk_step_f32(const float* V, int64_t bsv, const float* sigma2, const float* resid, float* out /*[B,8]*/,
                     float* alpha /*[B,N]*/, int* info, void* workspace, int B, int N, int flags, void* stream);
int volt_vk_step_f64(const double* V, int64_t bsv, const double* sigma2, const double* resid, double* out /*[B,8]*/,
                     double* alpha /*[B,N]*/, int* info, void* workspace, int B, int N, int flags, void* stream);
/* The conditioning of a FORECAST from that data model in O(N) (predict_solver="linear").  The reference factors the train block
 * of the stacked kernel per sample and solves twice (voltron/rollout_utils.py:35-36, and :44 for the covariance); every
 * appended point has the same cross-covariance with the train block, u = V (its last column), so all a forecast needs from
 * the train block are scalars.  Per series, with A_b = V_b[min(i,k)] + jitter_b I:
 *     out[b,0] = V'A^-1 V (rho),  out[b,1] = V'A^-1 r (tau),  out[b,2] = r'A^-1 r,  out[b,3] = logdet A
 * -- the forward sweep of volt_vk_step_* with a second z chain over D V next to the one over D r:  rho = sum (z^V_i)^2 / d_i,
 * tau = sum z^V_i z^r_i / d_i.  No backward sweep, no workspace.  V, bsv: as for volt_vk_step_*.  jitter [B] doubles, >= 0
 * (a rung of the jitter ladder; 0 is legal: the forms are then V_{N-1}, r_{N-1}, ...) -- doubles for BOTH entries, as is
 * `out` [B,4]: rho is subtracted from running sums of its own size to leave increments ~dx vol^2.  out[b,2] and out[b,3] are
 * the r'A^-1 r and logdet volt_vk_step_* returns for sigma2 = jitter.
 * info[b]: 0, or i + 1 for the first pivot d_i that is not a positive finite number (jitter = 0 and a flat step V_i = V_{i-1},
 * a NaN in V); out[b,0..3] are then NaN.  One launch, fp64 arithmetic, no atomics, bitwise repeatable, replays from a
 * hipGraph, 64-bit indices, nothing O(N^2).
 * Argument errors: -1 V NULL; -2 bsv < 0 or 0 < bsv < N; -3 jitter, -4 resid, -5 out, -6 info NULL; -7 B < 1; -8 N < 1. */
int volt_vk_forms_f32(const float* V, int64_t bsv, const double* jitter, const float* resid, double* out /*[B,4]*/, int* info,
                      int B, int N, void* stream);
int volt_vk_forms_f64(const double* V, int64_t bsv, const double* jitter, const double* resid, double* out /*[B,4]*/, int* info,
                      int B, int N, void* stream);
/* The POSTERIOR of the Brownian-motion vol forecaster at H test points in O(N H) time and O(H) memory (BMGP / MultitaskBMGP
 * with posterior="sweep").  For a test point xi >= 0 the cross-covariance column k = v min(x, xi) has the first difference
 * (D k)_i = v clamp(xi - x_{i-1}, 0, delta_i), so its chain z(xi) is formed on the fly; over xs [H] sorted ascending (shared by
 * the batch), per series
 *     out[b,0,h] = m_h = k_h'A^-1 r,   out[b,1,h] = p_h = k_h'A^-1 k_h,   out[b,2,h] = q_h = k_h'A^-1 k_{h+1}  (q_{H-1} = p_{H-1})
 * -- doubles for BOTH entries.  The posterior mean at xi_h is m(xi_h) + m_h, its variance v xi_h - p_h, the covariance of
 * neighbours v xi_h - q_h; the posterior is Markov, so these fix the whole H x H covariance.  Test points beyond the grid give
 * p = q bitwise.  x [N] (bsx = 0: one grid for the batch) or [B,N] with batch stride bsx >= N in elements; vol, sigma2 [B];
 * resid [B,N].  One wave per (series, 64 test points), the forward sweep alone: ONE launch, no workspace, fp64 arithmetic, no
 * atomics, bitwise repeatable, replays from a hipGraph, 64-bit indices.
 * info[b]: 0; i + 1 for the first pivot d_i that is not a positive finite number; or -(h + 1) for the first test point that
 * is NaN / inf, negative or smaller than its predecessor (no sweep runs then).  The series' rows of out are NaN in both cases.
 * Argument errors: -1 x NULL; -2 bsx < 0 or 0 < bsx < N; -3 xs, -4 vol, -5 sigma2, -6 resid, -7 out, -8 info NULL; -9 B < 1;
 * -10 N < 1; -11 H < 1 (or beyond 65535 blocks of 64). */
int volt_bm_post_f32(const float* x, int64_t bsx, const float* xs, const float* vol, const float* sigma2, const float* resid,
                     double* out /*[B,3,H]*/, int* info, int B, int N, int H, void* stream);
int volt_bm_post_f64(const double* x, int64_t bsx, const double* xs, const double* vol, const double* sigma2, const double* resid,
                     double* out /*[B,3,H]*/, int* info, int B, int N, int H, void* stream);
int volt_bm_solve_f32(const float* x, const float* vol, const float* sigma2, const float* R /*[B,N,H]*/,
                      float* X /*[B,N,H]*/, int* info, void* workspace, int B, int N, int H, void* stream);
int volt_bm_solve_f64(const double* x, const double* vol, const double* sigma2, const double* R /*[B,N,H]*/,
                      double* X /*[B,N,H]*/, int* info, void* workspace, int B, int N, int H, void* stream);

/* ---- Joint draws in O(S H) from the two covariances of the forecast that are semiseparable plus a diagonal (DESIGN 4.17;
 * csrc/chain_draw.hip has the recursion).  For cov(i,i) = c_i, cov(i+1,j) = g_i cov(i,j) (j <= i) and a jitter j on the
 * diagonal, out = mean + chol(C + j I) z without C: two running scalars per path.  One lane per path, H unbounded and streamed
 * through LDS in chunks, fp64 arithmetic (z and out carry the entry's type), ONE launch, no workspace, no atomics, bitwise
 * repeatable, replays from a hipGraph, 64-bit indices.  jitter [G] doubles, >= 0 (a rung of the ladder; 0 is legal).
 *
 * volt_markov_draw_*: the Markov posterior of the vol forecaster (BMGP / MultitaskBMGP(posterior="chain")): c = max(diag, 0),
 * g_i = max(off_i / diag_i, 0), 0 where diag_i <= 0 (off[., H-1] is not read) -- the matrix gp._markov_cov builds.  mean, diag,
 * off [G,H] doubles; z, out [G,S,H].  flags: VOLT_DRAW_EXP writes exp(out), computed in double and rounded once.
 * info[g]: 0, or i + 1 for the first step whose e_i + j is not a positive finite number; ALL S x H outputs of the series are
 * then NaN.
 * Argument errors: -1 mean, -2 diag, -3 off, -4 z, -5 jitter, -6 out, -7 info NULL; -8 G < 1; -9 S < 1 (or beyond 65535 blocks
 * of 1024 paths); -10 H < 1; -11 an unknown flag.
 *
 * volt_vk_draw_*: the predictive block of the volatility-kernel data model, C = W[min(s,t)] (g = 1), with
 * W_h = (V_last - rho) + sum_{k <= h} w_k pred_vol_k^2 formed on the fly in fp64: CumTrapz's weights over the H + 1 points
 * [vol_last, pred_vol] on one uniform step dx (dx / 2 on the first and the last point, dx between) less its first entry.
 * pred_vol [G,S,H]; vol_last, vlr = V_last - rho, dx [G] doubles; mean [G,H] doubles (tau, m(x_t) and the theta pull folded in
 * by the caller); z, out [G,S*reps,H]: `reps` >= 1 consecutive paths share a row of pred_vol.
 * info [G,S]: 0, or i + 1 as above, per pred_vol row; all H outputs of its `reps` paths are then NaN, other paths unchanged.
 * Argument errors: -1 pred_vol, -2 vol_last, -3 vlr, -4 dx, -5 mean, -6 z, -7 jitter, -8 out, -9 info NULL; -10 G < 1;
 * -11 S < 1; -12 H < 1; -13 reps < 1 (or more than 2^31 - 1 blocks of 64 paths). */
#define VOLT_DRAW_EXP 1           /* flag bit of volt_markov_draw_* */
/* volt_markov_mix_f32: the draws of T eigen-directions carried to the T tasks of MultitaskBMGP(posterior="chain"):
 * out[s,h,t] = mean[h,t] + sum_j V[t,j] lz[j,s,h], lz [T,S,n] doubles (volt_markov_draw_f64 with G = T), V [T,T] doubles
 * (row t: task t), mean [n,T], out [S,n,T].  The sum is fp64 in the fixed order j = 0 .. T-1, rounded once.  One launch.
 * Argument errors: -1 lz, -2 V, -3 mean, -4 out NULL; -5 T < 1 or T > 64; -6 S < 1 (or more than 2^31 - 1 blocks of 64 points); -7 n < 1. */
int volt_markov_mix_f32(const double* lz /*[T,S,n]*/, const double* V /*[T,T]*/, const float* mean /*[n,T]*/, float* out /*[S,n,T]*/,
                        int T, int S, int n, void* stream);
int volt_markov_draw_f32(const double* mean, const double* diag, const double* off, const float* z, const double* jitter,
                         float* out, int* info, int G, int S, int H, int flags, void* stream);
int volt_markov_draw_f64(const double* mean, const double* diag, const double* off, const double* z, const double* jitter,
                         double* out, int* info, int G, int S, int H, int flags, void* stream);
int volt_vk_draw_f32(const float* pred_vol, const double* vol_last, const double* vlr, const double* dx, const double* mean,
                     const float* z, const double* jitter, float* out, int* info, int G, int S, int H, int reps, void* stream);
int volt_vk_draw_f64(const double* pred_vol, const double* vol_last, const double* vlr, const double* dx, const double* mean,
                     const double* z, const double* jitter, double* out, int* info, int G, int S, int H, int reps, void* stream);

/* ---- GPCV ELBO step for the Brownian-motion prior in O(N^2)  (SingleTaskVariationalGP(prior_solver="linear"): LearnGPCV's
 * default prior, K = vol min(x, x'), without the N x N factorisation).  The step of volt_gpcv_step_f32 / volt_gpcv_cv_step_f32
 * with K given as (x [N], vol [B]) over a grid 0 <= x_0 < x_1 < .. shared by the batch:  A = K + jitter I = D^-1 T D^-T with T
 * tridiagonal (volt_bm_*, above), so G = A^-1 Lq is one O(N) chain solve per column of Lq and every scalar of the KL follows
 * from the same sweeps (csrc/gpcv_bm.hip has the recurrences).  Chain arithmetic fp64, I/O fp32.
 *     abc == NULL (and Kc == 0): the "exp" likelihood;  abc [B,3,Kc], 1 <= Kc <= VOLT_GPCV_CV_K_MAX: the "cv" one.
 *     out[b,0..11], grad_m, grad_mu [B,N], grad_Lq [B,N,N] (zero above the diagonal), grad_abc [B,3,Kc]: exactly as
 *     volt_gpcv_step_f32 / volt_gpcv_cv_step_f32 document them.  There is no grad_K: the prior's only parameter is vol, and
 *     dF/dvol follows from out[b,2..8] in closed form.  Elements of Lq above the diagonal are never read.
 * info[b]: 0, or i + 1 for the first pivot d_i that is not a positive finite number (as volt_bm_step_*: jitter = 0 at
 * x_0 = 0, a NaN vol); the outputs of that series are then NaN.
 * workspace: volt_gpcv_bm_workspace_bytes(B, N, Kc) bytes (0 for a shape out of range), 256-byte aligned: one row-packed fp64
 * lower triangle per series for the forward sweep's z (4 B N (N + 1) bytes) plus O(B N).  It needs no initialisation call.
 * No host synchronisation, no allocation, no atomics: every reduction has a fixed order, results are bitwise repeatable, and
 * the launch sequence replays from a hipGraph.  1 <= B <= 65535, N >= 1; indices are 64-bit.
 * Argument errors (before any launch, checked in the order of their numbers): -1 x, -2 vol, -4 resid, -5 m, -6 Lq, -7 y NULL;
 * -9 Kc out of range with abc, or Kc != 0 without; -10 gh_x, -11 gh_w NULL; -12 Q outside 1 .. 1024; -17 out, -18 grad_m,
 * -19 grad_mu, -20 grad_Lq NULL; -21 grad_abc NULL with abc; -22 info NULL; -23 workspace NULL or not 256-byte aligned;
 * -24 B outside 1 .. 65535; -25 N < 1. */
size_t volt_gpcv_bm_workspace_bytes(int B, int N, int Kc);
int volt_gpcv_bm_step_f32(const float* x, const float* vol, float jitter, const float* resid, const float* m, const float* Lq,
                          const float* y, const float* abc, int Kc, const float* gh_x, const float* gh_w, int Q, float min_var,
                          float min_scale, float w_ell, float w_kl, float* out, float* grad_m, float* grad_mu, float* grad_Lq,
                          float* grad_abc, int* info, void* workspace, int B, int N, void* stream);

/* ---- GPCV ELBO step in O(N) for the Brownian-motion prior with a Markov variational family
 * (SingleTaskVariationalGP(prior_solver="markov"); csrc/gpcv_markov.hip has the recurrences).
 * Prior: f - mu is Brownian motion started from an N(0, jitter) level over the grid x [N] (0 <= x_0 < x_1 < .., shared by the
 * batch): K_M = vol min(x, x') + jitter 1 1', increments of variance q_0 = vol x_0 + jitter, q_i = vol (x_i - x_{i-1}).  This is
 * NOT the other steps' K + jitter I: a jitter on the starting level keeps K_M^-1 exactly tridiagonal (and x_0 = 0 valid).
 * Family: q = N(m, P^-1), P = Lp Lp', Lp lower bidiagonal: diagonal exp(rho_i), entry (i+1, i) gamma_i exp(rho_i).
 * rho, gamma [B,N]; gamma[., N-1] is never read.  resid = m - mu.  abc == NULL (and Kc == 0): the "exp" likelihood;
 * abc [B,3,Kc], 1 <= Kc <= VOLT_GPCV_CV_K_MAX: the "cv" one.  Arithmetic of the recurrences fp64, quadrature and I/O fp32.
 *     out[b,0..11] = ell, KL, quad, logdet K_M, logdet S, tr(K_M^-1 S), dF/dvol, 0, 0, F = w_ell ell - w_kl KL, jitter, 0
 *     grad_m, grad_mu, grad_rho, grad_gamma [B,N] (grad_gamma[., N-1] = 0), grad_abc [B,3,Kc] = dF/d(a,b,c)
 * info[b]: 0, or 1 where F is not finite (there is no pivot that can fail).
 * workspace: volt_gpcv_markov_workspace_bytes(B, N, Kc) bytes (0 for a shape out of range), 256-byte aligned, O(B N); it needs
 * no initialisation call and is fully written before it is read.  On return its first 8 B N bytes hold diag S [B,N] in fp64.
 * ONE launch, one workgroup per series; no host synchronisation, no allocation, no atomics: every reduction has a fixed
 * order, results are bitwise repeatable, and the launch replays from a hipGraph.  1 <= B <= 65535, N >= 1; 64-bit indices.
 * Argument errors (before the launch, in the order of their numbers): -1 x, -2 vol, -4 resid, -5 m, -6 rho, -7 gamma, -8 y
 * NULL; -10 Kc out of range with abc, or Kc != 0 without; -11 gh_x, -12 gh_w NULL; -13 Q outside 1 .. 1024; -18 out,
 * -19 grad_m, -20 grad_mu, -21 grad_rho, -22 grad_gamma NULL; -23 grad_abc NULL with abc; -24 info NULL; -25 workspace NULL
 * or not 256-byte aligned; -26 B outside 1 .. 65535; -27 N < 1.
 *
 * volt_markov_root_draw_f32: out[b,r,:] = m[b] + Lp[b]^-T eps[b,r,:] (u_{N-1} = eps_{N-1} e^{-rho_{N-1}},
 * u_i = eps_i e^{-rho_i} - gamma_i u_{i+1}): `reps` draws per series, eps, out [B,reps,N]; fp64 arithmetic, rounded once.
 * One launch, one workgroup per draw.  Argument errors: -1 m, -2 rho, -3 gamma, -4 eps, -5 out NULL; -6 B < 1; -7 reps < 1 (or
 * B reps >= 2^24 draws: a launch of 256-thread workgroups holds fewer than 2^32 threads); -8 N < 1.
 * volt_markov_root_var_f32: var [B,N] (fp64) = diag (Lp Lp')^-1, the step's s.  Argument errors: -1 rho, -2 gamma, -3 var
 * NULL; -4 B < 1; -5 N < 1. */
size_t volt_gpcv_markov_workspace_bytes(int B, int N, int Kc);
int volt_gpcv_markov_step_f32(const float* x, const float* vol, float jitter, const float* resid, const float* m, const float* rho,
                              const float* gamma, const float* y, const float* abc, int Kc, const float* gh_x, const float* gh_w,
                              int Q, float min_var, float min_scale, float w_ell, float w_kl, float* out, float* grad_m,
                              float* grad_mu, float* grad_rho, float* grad_gamma, float* grad_abc, int* info, void* workspace,
                              int B, int N, void* stream);
int volt_markov_root_draw_f32(const float* m, const float* rho, const float* gamma, const float* eps, float* out, int B, int reps,
                              int N, void* stream);
int volt_markov_root_var_f32(const float* rho, const float* gamma, double* var, int B, int N, void* stream);

/* ---- Natural-gradient update of the Markov GPCV's q in O(N), ONE launch (csrc/gpcv_markov_ng.hip has the
 * recurrences).  Prior, family and likelihood arguments as volt_gpcv_markov_step_f32, with mu [B,N] the prior mean in place of
 * resid.  The optimum of F over q has precision K_M^-1 + diag(lam2) and mean mu + P^-1 lam1, which lies in the family; one call
 * moves the sites lam1, lam2 [B,N] (fp64, updated IN PLACE; zeros stand for q = prior) a step in (0, 1] towards the targets the
 * current q = (m, rho, gamma) asks for, with r = w_ell / w_kl, d = m - mu, gm = dE/dm, gv = dE/ds at the current q,
 *     t2_i = max(-2 r gv_i, 0),  t1_i = r gm_i + t2_i d_i,  lam <- (1 - step) lam + step t,
 * and writes the q of the new sites: (rho_out, gamma_out) the bidiagonal root of K_M^-1 + diag(lam2) (gamma_out[., N-1] = 0;
 * gamma[., N-1] is never read), m_out = mu + P^-1 lam1.  m_out / rho_out / gamma_out may be the buffers m / rho / gamma.
 *     out[b,0..3] (fp64) = the number of sites clamped at 0 (gv_i > 0), max |m_out - m|, max |rho_out - rho|,
 *                          max |gamma_out - gamma| (over i < N - 1)
 * info[b]: 0, or 1 where a site, a pivot or an output of series b is not finite (only a non-finite input can do that: every
 * pivot of K_M^-1 + diag(lam2 >= 0) is positive); m_out, rho_out, gamma_out, lam1, lam2 and out of that series are then NaN,
 * the other series are not affected.
 * workspace: volt_gpcv_markov_ng_workspace_bytes(B, N, Kc) bytes (0 for a shape out of range), 256-byte aligned, 32 B N bytes;
 * it needs no initialisation call and is fully written before it is read.  On return its first 8 B N bytes hold
 * diag P^-1 [B,N] of the INPUT q in fp64: volt_gpcv_markov_step_f32's s bit for bit.
 * One workgroup per series; no host synchronisation, no allocation, no atomics: every reduction has a fixed order, results are
 * bitwise repeatable, and the launch replays from a hipGraph.  1 <= B <= 65535, N >= 1; 64-bit indices.
 * Argument errors (before the launch, in the order of their numbers): -1 x, -2 vol, -4 mu, -5 m, -6 rho, -7 gamma, -8 y NULL;
 * -10 Kc out of range with abc, or Kc != 0 without; -11 gh_x, -12 gh_w NULL; -13 Q outside 1 .. 1024; -17 w_kl not > 0;
 * -18 step outside (0, 1]; -19 lam1, -20 lam2, -21 m_out, -22 rho_out, -23 gamma_out, -24 out, -25 info NULL; -26 workspace NULL
 * or not 256-byte aligned; -27 B outside 1 .. 65535; -28 N < 1. */
size_t volt_gpcv_markov_ng_workspace_bytes(int B, int N, int Kc);
int volt_gpcv_markov_ng_f32(const float* x, const float* vol, float jitter, const float* mu, const float* m, const float* rho,
                            const float* gamma, const float* y, const float* abc, int Kc, const float* gh_x, const float* gh_w,
                            int Q, float min_var, float min_scale, float w_ell, float w_kl, double step, double* lam1,
                            double* lam2, float* m_out, float* rho_out, float* gamma_out, double* out, int* info,
                            void* workspace, int B, int N, void* stream);

/* ---- The Markov GPCV away from its grid in O(N + S H): mean, variance and joint path draws of f at H test points
 * (SingleTaskVariationalGP / MultitaskVariationalGP(prior_solver="markov")(x); csrc/markov_predict.hip has the
 * formulas and the plan's steps).  Given u ~ q, f(xi) is a Brownian bridge between the neighbouring knots of the grid x [N],
 * free Brownian motion beyond x_{N-1}, and a bridge from (-jitter / vol, level mu, variance 0) before x_0.
 *
 * volt_markov_predict_plan_f32: x [N] and xs [H] (ascending, >= 0, finite; duplicates allowed) are shared by the B series;
 * vol, mu [B]; m, rho, gamma [B,N] (gamma[., N-1] is never read).  Outputs, all fp64: mean, var_q (the q part A P^-1 A'),
 * var_p (the bridge part K** - A K_uu A') [B,H]; the draw plan coef [B,3H+1,3] and code [B,3H+1] (8 h + op), of which
 * steps[b] <= 3 H + 1 entries are steps (the rest no-ops); steps depends on (x, xs) alone.  var_q at a test point ON a knot is
 * volt_markov_root_var_f32's s there bit for bit, and mean is m there.
 * info[b]: 0; -(h + 1) for the first xs_h that is NaN, infinite, negative or below its predecessor -- the series' outputs are
 * then NaN and steps[b] = 0; 1 where a variance (or s_0) is not finite.
 * workspace: volt_markov_predict_workspace_bytes(B, N, H) bytes (0 for a shape out of range), 256-byte aligned, O(B (N + H)),
 * no initialisation call, fully written before it is read.  ONE launch, one workgroup per series; no atomics, bitwise
 * repeatable, replays from a hipGraph.  1 <= B <= 65535, N >= 1, 1 <= H <= 2^24; 64-bit indices.
 * Argument errors: -1 x, -2 xs, -3 vol, -5 mu, -6 m, -7 rho, -8 gamma, -9 mean, -10 var_q, -11 var_p, -12 coef, -13 code,
 * -14 steps, -15 info NULL; -16 workspace NULL or not 256-byte aligned; -17 B, -18 N, -19 H out of range.
 *
 * volt_markov_predict_draw_f32: out[b,s,:] = the plan run on eps[b,s,:]: eps [B,S,E] with E >= steps[b] base samples per
 * path (N(0,1) for a joint draw; the first steps[b] of a row are read), out [B,S,H] fp32, fp64 arithmetic rounded once.
 * flags: VOLT_DRAW_EXP writes exp(out); VOLT_PREDICT_NO_CHAIN / VOLT_PREDICT_NO_BRIDGE zero the noise of the chain steps
 * (the q part) / of the bridge steps, the mean is added either way.  A series whose steps[b] is 0 (a failed plan) or exceeds
 * E gets NaN.  One lane per path, one wave per 64 paths of one series, eps and out staged through LDS; ONE launch, no workspace.
 * Argument errors: -1 mean, -2 coef, -3 code, -4 steps, -5 eps, -6 out NULL; -7 B outside 1 .. 65535; -8 S < 1; -9 H out of
 * range; -10 E < 1; -11 an unknown flag. */
#define VOLT_PREDICT_NO_CHAIN 2   /* flag bits of volt_markov_predict_draw_f32 (beside VOLT_DRAW_EXP) */
#define VOLT_PREDICT_NO_BRIDGE 4
size_t volt_markov_predict_workspace_bytes(int B, int N, int H);
int volt_markov_predict_plan_f32(const float* x, const float* xs, const float* vol, float jitter, const float* mu, const float* m,
                                 const float* rho, const float* gamma, double* mean, double* var_q, double* var_p, double* coef,
                                 int* code, int* steps, int* info, void* workspace, int B, int N, int H, void* stream);
int volt_markov_predict_draw_f32(const double* mean, const double* coef, const int* code, const int* steps, const float* eps,
                                 float* out, int B, int S, int H, int E, int flags, void* stream);

/* ---- Multi-task GPCV ELBO step in O(N T (Q + T) + T^3): the Markov variational family under the Kronecker prior
 * (MultitaskVariationalGP(prior_solver="markov"); csrc/gpcv_mt_markov.hip has the closed forms).
 * Prior: p(F) = N(mu, K_M (x) K_t) over the grid x [N] (0 <= x_0 < x_1 < ..), K_M = vol min(x, x') + jitter 1 1' as in
 * volt_gpcv_markov_step_f32 (vol [1]; NOT the dense multi-task step's K + jitter I), K_t = f f' + diag softplus(raw_var)
 * (covar_factor f [T], raw_var [T]), mu[n,t] = c_t.
 * Family: q(F) = N(M, P^-1 (x) S_t), P = Lp Lp' with Lp lower bidiagonal (diagonal exp(rho_i), entry (i+1, i)
 * gamma_i exp(rho_i); rho, gamma [N], gamma[N-1] is never read), S_t = Lt Lt' (Lt [T,T]; what lies above its diagonal is
 * ignored), M [N,T].  y [N,T].  abc == NULL (and Kc == 0): the "exp" likelihood; abc [T,3,Kc], 1 <= Kc <=
 * VOLT_GPCV_CV_K_MAX: the "cv" one with one warp per task (the TRANSFORMED a, b, c).  Recurrences and sums fp64, the
 * quadrature nodes and all I/O fp32.
 *     out[0..11] = ell, KL, quad = tr(K_t^-1 G), logdet K_M, logdet K_t, logdet S_x = -2 sum rho, logdet S_t,
 *                  tau_x = tr(K_M^-1 P^-1), tau_t = tr(K_t^-1 S_t), dF/dvol, F = w_ell ell - w_kl KL, jitter
 *     grad_M [N,T], grad_c [T], grad_rho, grad_gamma [N] (grad_gamma[N-1] = 0), grad_Lt [T,T] (zero above the diagonal),
 *     grad_covar_factor, grad_raw_var [T], grad_abc [T,3,Kc] = dF/d(a,b,c)
 * info[0]: 1 where F is not finite, else 0;  info[1]: 0, or j + 1 for the first pivot j of K_t that is not positive (the
 * outputs are then NaN).  A NaN input arrives in info; there is no data-dependent loop.
 * workspace: volt_gpcv_mt_markov_workspace_bytes(N, T, Kc) bytes (0 for a shape out of range), 256-byte aligned,
 * O(N T + T^2 ceil(N / 128)); it needs no initialisation call and is fully written before it is read.  On return its first
 * 8 N bytes hold diag P^-1 [N] in fp64.
 * Four launches (five with abc); no host synchronisation, no allocation, no atomics: every reduction has a fixed order that
 * depends on (N, T) alone, results are bitwise repeatable, and the launch sequence replays from a hipGraph.
 * N >= 1, 1 <= T <= 64; 64-bit indices.
 * Argument errors (before any launch, in the order of their numbers): -1 x, -2 vol, -4 M, -5 c, -6 rho, -7 gamma, -8 Lt,
 * -9 covar_factor, -10 raw_var, -11 y NULL; -13 Kc out of range with abc, or Kc != 0 without; -14 gh_x, -15 gh_w NULL;
 * -16 Q outside 1 .. 1024; -21 out, -22 grad_M, -23 grad_c, -24 grad_rho, -25 grad_gamma, -26 grad_Lt, -27 grad_covar_factor,
 * -28 grad_raw_var NULL; -29 grad_abc NULL with abc; -30 info NULL; -31 workspace NULL or not 256-byte aligned; -32 N < 1;
 * -33 T outside 1 .. 64. */
size_t volt_gpcv_mt_markov_workspace_bytes(int N, int T, int Kc);
int volt_gpcv_mt_markov_step_f32(const float* x, const float* vol, float jitter, const float* M, const float* c, const float* rho,
                                 const float* gamma, const float* Lt, const float* covar_factor, const float* raw_var,
                                 const float* y, const float* abc, int Kc, const float* gh_x, const float* gh_w, int Q,
                                 float min_var, float min_scale, float w_ell, float w_kl, float* out, float* grad_M,
                                 float* grad_c, float* grad_rho, float* grad_gamma, float* grad_Lt, float* grad_covar_factor,
                                 float* grad_raw_var, float* grad_abc, int* info, void* workspace, int N, int T, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* VOLT_HIP_H */
