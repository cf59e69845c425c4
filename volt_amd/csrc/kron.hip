// Kronecker multi-task exact GP of the batched vol forecaster (voltron/models/BMGP.py:30-56, MultitaskBMGP:
// Sigma = K_x (x) K_t + I_N (x) D with K_x = vol M, M = min(x_i, x_k), K_t = F F' + diag(var), D = diag(d)).
//
// After S = D^-1/2 K_t D^-1/2 = Q Lambda Q' the exact MLL is T independent N x N exact-GP steps over the ONE matrix M:
//     lambda_j K_x + I = kappa_j (M + sigma_j^2 I),  kappa_j = vol lambda_j,  sigma_j^2 = 1 / kappa_j,
//     r_j = (R W)_j / sqrt(kappa_j),  W = D^-1/2 Q,  R = Y - mu
// so one iteration is  prologue (here) -> volt_mll_step_* with B = T -> epilogue (here); no NT x NT matrix exists.
//   * kron_jacobi: parallel cyclic Jacobi (Brent-Luk round-robin ordering) on a T x T symmetric matrix held in LDS, one
//     workgroup per matrix, T <= 64; the eigenvalues / vectors are then sorted ascending (as LAPACK's syev returns them).
//   * prologue: K_t, d, S and its eigenpairs from the raw parameters, then r and sigma^2 for the step.  EVERY workgroup
//     computes the same (deterministic) eigendecomposition and then its own slice of rows of R W -- no hand-off between
//     workgroups; workgroup 0 also writes the small state (vol, Lambda, d, W, Q) the epilogue and the posterior read.
//   * epilogue: one workgroup.  The reductions over N (alpha' r, alpha' alpha, alpha' x: 2 T^2 N + T N multiply-adds in
//     fp64), then T x T algebra for the MLL and the gradients of the five raw parameters.
// The device code (Jacobi, sort, S, the epilogue's body) lives in kron_shared.h: csrc/kron_chain.hip, the same step around the
// linear-time chain solver, is built from it too.
#include "kron_shared.h"
#include "../../include/volt_hip.h"

namespace volt {

__global__ __launch_bounds__(KNT) void syev_small_kernel(const double* __restrict__ S, int64_t bss, double* __restrict__ lam,
                                                         double* __restrict__ Q, int* __restrict__ info, int T) {
    __shared__ double sA[KT_MAX * KLD], sV[KT_MAX * KLD], sQ[KT_MAX * KLD];
    __shared__ JacobiLds s;
    const int b = blockIdx.x, tid = threadIdx.x;
    const double* Sb = S + (int64_t)b * bss;
    for (int e = tid; e < T * T; e += blockDim.x) {
        const int i = e / T, j = e - (e / T) * T;
        sA[i * KLD + j] = Sb[(int64_t)i * T + j];
    }
    __syncthreads();
    const int sw = kron_jacobi(sA, sV, T, s);
    kron_sort(sA, sV, sQ, T, s);
    for (int e = tid; e < T * T; e += blockDim.x) {
        const int i = e / T, j = e - (e / T) * T;
        Q[(int64_t)b * T * T + e] = sQ[i * KLD + j];
    }
    if (tid < T) lam[(int64_t)b * T + tid] = s.lam[tid];
    if (tid == 0) info[b] = sw;
}

template <typename R>
__global__ __launch_bounds__(KNT) void kron_prologue_kernel(const R* __restrict__ raw_vol, const R* __restrict__ cf,
                                                            const R* __restrict__ raw_var, const R* __restrict__ rtn,
                                                            const R* __restrict__ rn, const R* __restrict__ x,
                                                            const R* __restrict__ Y, int64_t ldy, R* __restrict__ resid,
                                                            R* __restrict__ sigma2, double* __restrict__ state,
                                                            int* __restrict__ info, int N, int T) {
    __shared__ double sA[KT_MAX * KLD], sV[KT_MAX * KLD], sR[KRB * KLD];
    __shared__ double sd[KT_MAX], sdiag[KT_MAX], srk[KT_MAX];
    __shared__ JacobiLds s;
    const int tid = threadIdx.x;
    const double vol = ksigmoid((double)raw_vol[0]);
    const double gnoise = ksoftplus((double)rn[0]) + KNOISE_FLOOR;
    kron_form_s(cf, raw_var, rtn, gnoise, sd, sdiag, sA, T);
    const int sw = kron_jacobi(sA, sV, T, s);
    kron_sort(sA, sV, sR, T, s);                                        // Q -> sR (free until the row passes)
    for (int e = tid; e < T * T; e += blockDim.x) {                     // W = D^-1/2 Q -> sV
        const int t = e / T, j = e - (e / T) * T;
        sV[t * KLD + j] = sR[t * KLD + j] / sqrt(sd[t]);
    }
    if (tid < T) srk[tid] = 1.0 / sqrt(vol * s.lam[tid]);
    if (blockIdx.x == 0) {
        for (int e = tid; e < T * T; e += blockDim.x) {
            const int t = e / T, j = e - (e / T) * T;
            state[kst_w(T) + e] = sR[t * KLD + j] / sqrt(sd[t]);
            state[kst_q(T) + e] = sR[t * KLD + j];
        }
        if (tid < T) {
            state[kst_lam(T) + tid] = s.lam[tid];
            state[kst_d(T) + tid] = sd[tid];
            sigma2[tid] = (R)(1.0 / (vol * s.lam[tid]));
        }
        if (tid == 0) {
            state[0] = vol;
            info[0] = sw;
        }
    }
    const double mscale = -0.5 * vol * vol;
    for (int n0 = blockIdx.x * KRB; n0 < N; n0 += gridDim.x * KRB) {
        __syncthreads();                                                // sR free (Q copied / last pass consumed)
        for (int e = tid; e < KRB * T; e += blockDim.x) {               // R = Y - mu, mu[n,t] = -1/2 vol^2 x_n K_t[t,t]
            const int nn = e / T, t = e - (e / T) * T, n = n0 + nn;
            if (n < N) sR[nn * KLD + t] = (double)Y[(int64_t)n * ldy + t] - mscale * (double)x[n] * sdiag[t];
        }
        __syncthreads();
        for (int e = tid; e < KRB * T; e += blockDim.x) {               // r_j = (R W)_j / sqrt(kappa_j), n fastest
            const int j = e / KRB, nn = e - (e / KRB) * KRB, n = n0 + nn;
            if (n >= N) continue;
            double acc = 0.0;
            for (int t = 0; t < T; ++t) acc = fma(sR[nn * KLD + t], sV[t * KLD + j], acc);
            resid[(int64_t)j * N + n] = (R)(acc * srk[j]);
        }
    }
}

template <typename R>
__global__ __launch_bounds__(KNT) void kron_epilogue_kernel(const R* __restrict__ raw_vol, const R* __restrict__ cf,
                                                            const R* __restrict__ raw_var, const R* __restrict__ rtn,
                                                            const R* __restrict__ rn, const R* __restrict__ x,
                                                            const R* __restrict__ resid, const R* __restrict__ out,
                                                            const R* __restrict__ alpha, const double* __restrict__ state,
                                                            R* __restrict__ res, int N, int T) {
    kron_epilogue_body<R, KRON_EPI_WHOLE>(raw_vol, cf, raw_var, rtn, rn, x, resid, out, alpha, state, res, nullptr, 0, N, T);
}

template <typename R>
int kron_prologue(const R* raw_vol, const R* cf, const R* raw_var, const R* rtn, const R* rn, const R* x, const R* Y,
                  int64_t ldy, R* resid, R* sigma2, double* state, int* info, int N, int T, void* stream) {
    const int bad = kron_prologue_check(raw_vol, cf, raw_var, rtn, rn, x, Y, ldy, resid, sigma2, state, info, N, T);
    if (bad) return bad;
    const int chunks = (N + KRB - 1) / KRB;
    const int grid = chunks < 64 ? chunks : 64;
    hipLaunchKernelGGL(kron_prologue_kernel<R>, dim3(grid), dim3(KNT), 0, (hipStream_t)stream, raw_vol, cf, raw_var, rtn, rn,
                       x, Y, ldy, resid, sigma2, state, info, N, T);
    VOLT_LAUNCH_CHECK();
    return 0;
}

template <typename R>
int kron_epilogue(const R* raw_vol, const R* cf, const R* raw_var, const R* rtn, const R* rn, const R* x, const R* resid,
                  const R* out, const R* alpha, const double* state, R* res, int N, int T, void* stream) {
    if (!raw_vol) return -1;
    if (!cf) return -2;
    if (!raw_var) return -3;
    if (!rtn) return -4;
    if (!rn) return -5;
    if (!x) return -6;
    if (!resid) return -7;
    if (!out) return -8;
    if (!alpha) return -9;
    if (!state) return -10;
    if (!res) return -11;
    if (N < 1) return -12;
    if (T < 1 || T > KT_MAX) return -13;
    hipLaunchKernelGGL(kron_epilogue_kernel<R>, dim3(1), dim3(KNT), 0, (hipStream_t)stream, raw_vol, cf, raw_var, rtn, rn, x,
                       resid, out, alpha, state, res, N, T);
    VOLT_LAUNCH_CHECK();
    return 0;
}

}  // namespace volt

using namespace volt;

extern "C" {

int volt_syev_small_f64(const double* S, int64_t bss, double* lam, double* Q, int* info, int B, int T, void* stream) {
    if (!S) return -1;
    if (bss < (int64_t)T * T) return -2;
    if (!lam) return -3;
    if (!Q) return -4;
    if (!info) return -5;
    if (B < 0 || B > 65535) return -6;
    if (T < 1 || T > KT_MAX) return -7;
    if (B == 0) return 0;
    hipLaunchKernelGGL(syev_small_kernel, dim3(B), dim3(KNT), 0, (hipStream_t)stream, S, bss, lam, Q, info, T);
    VOLT_LAUNCH_CHECK();
    return 0;
}

size_t volt_kron_state_bytes(int T) {
    if (T < 1 || T > KT_MAX) return 0;
    return (size_t)kst_len(T) * sizeof(double);
}

int volt_kron_prologue_f32(const float* raw_vol, const float* covar_factor, const float* raw_var, const float* raw_task_noises,
                           const float* raw_noise, const float* x, const float* Y, int64_t ldy, float* resid, float* sigma2,
                           double* state, int* info, int N, int T, void* stream) {
    return kron_prologue<float>(raw_vol, covar_factor, raw_var, raw_task_noises, raw_noise, x, Y, ldy, resid, sigma2, state,
                                info, N, T, stream);
}

int volt_kron_prologue_f64(const double* raw_vol, const double* covar_factor, const double* raw_var,
                           const double* raw_task_noises, const double* raw_noise, const double* x, const double* Y, int64_t ldy,
                           double* resid, double* sigma2, double* state, int* info, int N, int T, void* stream) {
    return kron_prologue<double>(raw_vol, covar_factor, raw_var, raw_task_noises, raw_noise, x, Y, ldy, resid, sigma2, state,
                                 info, N, T, stream);
}

int volt_kron_epilogue_f32(const float* raw_vol, const float* covar_factor, const float* raw_var, const float* raw_task_noises,
                           const float* raw_noise, const float* x, const float* resid, const float* out, const float* alpha,
                           const double* state, float* res, int N, int T, void* stream) {
    return kron_epilogue<float>(raw_vol, covar_factor, raw_var, raw_task_noises, raw_noise, x, resid, out, alpha, state, res,
                                N, T, stream);
}

int volt_kron_epilogue_f64(const double* raw_vol, const double* covar_factor, const double* raw_var,
                           const double* raw_task_noises, const double* raw_noise, const double* x, const double* resid,
                           const double* out, const double* alpha, const double* state, double* res, int N, int T,
                           void* stream) {
    return kron_epilogue<double>(raw_vol, covar_factor, raw_var, raw_task_noises, raw_noise, x, resid, out, alpha, state, res,
                                 N, T, stream);
}

}  // extern "C"
