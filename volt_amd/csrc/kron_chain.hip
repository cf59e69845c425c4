// The Kronecker multi-task step around the LINEAR-TIME chain step (MultitaskBMGP(solver="linear")):
//     volt_kron_prologue_warm_*  ->  volt_bm_step_* (x, vol = 1, sigma2 = 1 / kappa, resid = r; B = T)  ->  volt_kron_epilogue_ws_*
// Once the step costs O(T N) the two things around it that csrc/kron.hip does in a way that was free beside an O(T N^3) step
// are not free any more, and are done differently here (the mathematics, the state and the result are those of kron.hip; the
// device code both share is csrc/kron_shared.h):
//   * prologue, two launches in stream order.  kron_eigen_warm_kernel, ONE workgroup: S, then its eigenpairs by the same
//     Jacobi sweeps, started from the previous call's Q when `state` carries a valid stamp (A0 = Q0' S Q0, V0 = Q0: a
//     training step moves S by O(lr), so A0 is nearly diagonal and a few sweeps finish it) and cold otherwise; it writes the
//     state, sigma2, info and the stamp.  kron_rows_kernel, a grid over chunks of N: reads W, Lambda and vol from the state
//     and writes r.  (kron.hip's one launch repeats the decomposition in every workgroup and lets workgroup 0 write the state;
//     a warm start that READ the state in that launch would race with that write -- hence two launches.)
//   * epilogue, two launches in stream order.  kron_gram_kernel, one workgroup per slice of KSL columns of N: the partial sums
//     over its slice, to the caller's workspace.  kron_epilogue_ws_kernel, one workgroup: adds the partials in slice order and
//     runs the T x T algebra.
// Stream order is the only synchronisation: no atomics, no hand-off words, no workgroup waits on another.
#include "kron_shared.h"
#include "../../include/volt_hip.h"

namespace volt {

constexpr double KWARM_STAMP = 1447512148.0;    // state[1] = KWARM_STAMP + T: Q in the state is a decomposition for this T
constexpr double KWARM_ORTH = 1e-6;             // max |Q0' Q0 - I| above this: whatever is in the state is no previous Q
constexpr int KROWS_GRID = 256;                 // workgroups of the rows kernel (each strides over the chunks of KRB rows)

// Eigenpairs of S for the warm prologue.  LDS: three [T][KLD] arrays, 100 KB.
//   warm: Q0 (state) -> sV;  G = Q0' Q0 -> sB;  Q1 = Q0 (3 I - G) / 2 -> sA  (one Newton-Schulz step: Q0 carries the rounding
//         of every solve since the last cold start, |G - I| = e becomes O(e^2), so Q stays orthogonal to rounding however long
//         the run);  S -> sV;  S Q1 -> sB;  A0 = Q1' (S Q1) -> sV;  sweeps on (A = sV, V = sA);  sorted Q -> sB.
//   cold: S -> sA;  kron_jacobi (V = I in sV) exactly as kron_prologue_kernel;  sorted Q -> sB.
template <typename R>
__global__ __launch_bounds__(KNT) void kron_eigen_warm_kernel(const R* __restrict__ raw_vol, const R* __restrict__ cf,
                                                              const R* __restrict__ raw_var, const R* __restrict__ rtn,
                                                              const R* __restrict__ rn, R* __restrict__ sigma2,
                                                              double* __restrict__ state, int* __restrict__ info, int T) {
    __shared__ double sA[KT_MAX * KLD], sV[KT_MAX * KLD], sB[KT_MAX * KLD];
    __shared__ double sd[KT_MAX], sdiag[KT_MAX];
    __shared__ JacobiLds s;
    __shared__ int cold;
    const int tid = threadIdx.x;
    const double vol = ksigmoid((double)raw_vol[0]);
    const double gnoise = ksoftplus((double)rn[0]) + KNOISE_FLOOR;
    const bool stamped = state[1] == KWARM_STAMP + (double)T;          // the same for every thread
    if (tid == 0) cold = stamped ? 0 : 1;
    __syncthreads();
    if (stamped) {
        for (int e = tid; e < T * T; e += blockDim.x) {
            const double q = state[kst_q(T) + e];
            sV[(e / T) * KLD + e - (e / T) * T] = q;
            if (!isfinite(q)) cold = 1;
        }
        __syncthreads();
        for (int e = tid; e < T * T; e += blockDim.x) {                 // G = Q0' Q0
            const int i = e / T, j = e - (e / T) * T;
            double acc = 0.0;
            for (int k = 0; k < T; ++k) acc = fma(sV[k * KLD + i], sV[k * KLD + j], acc);
            sB[i * KLD + j] = acc;
            if (!(fabs(acc - (i == j ? 1.0 : 0.0)) <= KWARM_ORTH)) cold = 1;
        }
        __syncthreads();
        for (int e = tid; e < T * T; e += blockDim.x) {                 // Q1 = 3/2 Q0 - 1/2 Q0 G
            const int i = e / T, j = e - (e / T) * T;
            double acc = 1.5 * sV[i * KLD + j];
            for (int k = 0; k < T; ++k) acc = fma(-0.5 * sV[i * KLD + k], sB[k * KLD + j], acc);
            sA[i * KLD + j] = acc;
        }
        __syncthreads();
    }
    const bool warm = cold == 0;                                        // read after a barrier: the same for every thread
    double* A = warm ? sV : sA;                                         // what the sweeps diagonalise ...
    double* V = warm ? sA : sV;                                         // ... and where they keep the eigenvectors
    int sw;
    if (warm) {
        kron_form_s(cf, raw_var, rtn, gnoise, sd, sdiag, sV, T);
        for (int e = tid; e < T * T; e += blockDim.x) {                 // S Q1
            const int i = e / T, j = e - (e / T) * T;
            double acc = 0.0;
            for (int k = 0; k < T; ++k) acc = fma(sV[i * KLD + k], sA[k * KLD + j], acc);
            sB[i * KLD + j] = acc;
        }
        __syncthreads();
        for (int e = tid; e < T * T; e += blockDim.x) {                 // A0 = Q1' (S Q1); (i,j) and (j,i) take the same sum
            const int i = e / T, j = e - (e / T) * T;
            const int lo = i < j ? i : j, hi = i < j ? j : i;
            double acc = 0.0;
            for (int k = 0; k < T; ++k) acc = fma(sA[k * KLD + lo], sB[k * KLD + hi], acc);
            sV[i * KLD + j] = acc;
        }
        sw = kron_jacobi_sweeps(A, V, T, s);
    } else {
        kron_form_s(cf, raw_var, rtn, gnoise, sd, sdiag, sA, T);
        sw = kron_jacobi(A, V, T, s);
    }
    kron_sort(A, V, sB, T, s);
    if (tid == 0) s.flag = 0;                                           // from here: "the result holds a non-finite value"
    __syncthreads();
    for (int e = tid; e < T * T; e += blockDim.x) {
        const int t = e / T, j = e - (e / T) * T;
        const double q = sB[t * KLD + j];
        state[kst_w(T) + e] = q / sqrt(sd[t]);
        state[kst_q(T) + e] = q;
        if (!isfinite(q)) s.flag = 1;
    }
    if (tid < T) {
        state[kst_lam(T) + tid] = s.lam[tid];
        state[kst_d(T) + tid] = sd[tid];
        // (the sort ranks by comparisons, which a NaN eigenvalue fails: judge the diagonal itself, not only its sorted copy)
        if (!isfinite(s.lam[tid]) || !isfinite(A[tid * KLD + tid]) || !isfinite(sd[tid])) s.flag = 1;
    }
    __syncthreads();
    const bool finite = s.flag == 0;
    // a non-finite decomposition (NaN / inf in a parameter) must not pass as T healthy directions: sigma2 = NaN makes the
    // step report every one of them in its info
    if (tid < T) sigma2[tid] = finite ? (R)(1.0 / (vol * s.lam[tid])) : (R)NAN;
    if (tid == 0) {
        state[0] = vol;
        state[1] = sw >= 0 && finite ? KWARM_STAMP + (double)T : 0.0;   // the next call may start from this Q, or may not
        state[2] = warm ? 1.0 : 0.0;                                    // how THIS call started (for tests and profiles)
        info[0] = sw;
    }
}

// r_j = (R W)_j / sqrt(kappa_j) for the rows of this workgroup's chunks, with W, Lambda and vol as the eigen kernel left them
// in the state: kron_prologue_kernel's row passes.
template <typename R>
__global__ __launch_bounds__(KNT) void kron_rows_kernel(const R* __restrict__ cf, const R* __restrict__ raw_var,
                                                        const R* __restrict__ x, const R* __restrict__ Y, int64_t ldy,
                                                        R* __restrict__ resid, const double* __restrict__ state, int N, int T) {
    __shared__ double sW[KT_MAX * KLD], sR[KRB * KLD];
    __shared__ double sdiag[KT_MAX], srk[KT_MAX];
    const int tid = threadIdx.x;
    const double vol = state[0];
    if (tid < T) {
        const double f = (double)cf[tid];
        sdiag[tid] = f * f + ksoftplus((double)raw_var[tid]);          // K_t[t,t]
        srk[tid] = 1.0 / sqrt(vol * state[kst_lam(T) + tid]);
    }
    for (int e = tid; e < T * T; e += blockDim.x) sW[(e / T) * KLD + e - (e / T) * T] = state[kst_w(T) + e];
    const double mscale = -0.5 * vol * vol;
    for (int n0 = blockIdx.x * KRB; n0 < N; n0 += gridDim.x * KRB) {
        __syncthreads();                                                // sW, sdiag, srk written / last pass consumed
        for (int e = tid; e < KRB * T; e += blockDim.x) {               // R = Y - mu, mu[n,t] = -1/2 vol^2 x_n K_t[t,t]
            const int nn = e / T, t = e - (e / T) * T, n = n0 + nn;
            if (n < N) sR[nn * KLD + t] = (double)Y[(int64_t)n * ldy + t] - mscale * (double)x[n] * sdiag[t];
        }
        __syncthreads();
        for (int e = tid; e < KRB * T; e += blockDim.x) {               // n fastest
            const int j = e / KRB, nn = e - (e / KRB) * KRB, n = n0 + nn;
            if (n >= N) continue;
            double acc = 0.0;
            for (int t = 0; t < T; ++t) acc = fma(sR[nn * KLD + t], sW[t * KLD + j], acc);
            resid[(int64_t)j * N + n] = (R)(acc * srk[j]);
        }
    }
}

template <typename R>
__global__ __launch_bounds__(KNT) void kron_gram_kernel(const R* __restrict__ x, const R* __restrict__ resid,
                                                        const R* __restrict__ alpha, double* __restrict__ partial, int N, int T) {
    kron_epilogue_body<R, KRON_EPI_GRAM>(nullptr, nullptr, nullptr, nullptr, nullptr, x, resid, nullptr, alpha, nullptr, nullptr,
                                         partial, 0, N, T);
}

template <typename R>
__global__ __launch_bounds__(KNT) void kron_epilogue_ws_kernel(const R* __restrict__ raw_vol, const R* __restrict__ cf,
                                                               const R* __restrict__ raw_var, const R* __restrict__ rtn,
                                                               const R* __restrict__ rn, const R* __restrict__ out,
                                                               const double* __restrict__ state, R* __restrict__ res,
                                                               double* __restrict__ partial, int nslices, int N, int T) {
    kron_epilogue_body<R, KRON_EPI_SUMMED>(raw_vol, cf, raw_var, rtn, rn, nullptr, nullptr, out, nullptr, state, res, partial,
                                           nslices, N, T);
}

template <typename R>
int kron_prologue_warm(const R* raw_vol, const R* cf, const R* raw_var, const R* rtn, const R* rn, const R* x, const R* Y,
                       int64_t ldy, R* resid, R* sigma2, double* state, int* info, int N, int T, void* stream) {
    const int bad = kron_prologue_check(raw_vol, cf, raw_var, rtn, rn, x, Y, ldy, resid, sigma2, state, info, N, T);
    if (bad) return bad;
    hipLaunchKernelGGL(kron_eigen_warm_kernel<R>, dim3(1), dim3(KNT), 0, (hipStream_t)stream, raw_vol, cf, raw_var, rtn, rn,
                       sigma2, state, info, T);
    VOLT_LAUNCH_CHECK();
    const int chunks = (N + KRB - 1) / KRB;
    hipLaunchKernelGGL(kron_rows_kernel<R>, dim3(chunks < KROWS_GRID ? chunks : KROWS_GRID), dim3(KNT), 0, (hipStream_t)stream, cf,
                       raw_var, x, Y, ldy, resid, (const double*)state, N, T);
    VOLT_LAUNCH_CHECK();
    return 0;
}

template <typename R>
int kron_epilogue_ws(const R* raw_vol, const R* cf, const R* raw_var, const R* rtn, const R* rn, const R* x, const R* resid,
                     const R* out, const R* alpha, const double* state, R* res, void* workspace, int N, int T, void* stream) {
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
    if (!workspace || ((uintptr_t)workspace & 255)) return -12;
    if (N < 1) return -13;
    if (T < 1 || T > KT_MAX) return -14;
    const int nslices = kws_slices(N);
    double* partial = (double*)workspace;
    hipLaunchKernelGGL(kron_gram_kernel<R>, dim3(nslices), dim3(KNT), 0, (hipStream_t)stream, x, resid, alpha, partial, N, T);
    VOLT_LAUNCH_CHECK();
    hipLaunchKernelGGL(kron_epilogue_ws_kernel<R>, dim3(1), dim3(KNT), 0, (hipStream_t)stream, raw_vol, cf, raw_var, rtn, rn, out,
                       state, res, partial, nslices, N, T);
    VOLT_LAUNCH_CHECK();
    return 0;
}

}  // namespace volt

using namespace volt;

extern "C" {

size_t volt_kron_epilogue_workspace_bytes(int N, int T) {
    if (N < 1 || T < 1 || T > KT_MAX) return 0;
    const size_t bytes = (size_t)kws_slices(N) * (size_t)kws_stride(T) * sizeof(double);
    return (bytes + 255) / 256 * 256;
}

int volt_kron_prologue_warm_f32(const float* raw_vol, const float* covar_factor, const float* raw_var,
                                const float* raw_task_noises, const float* raw_noise, const float* x, const float* Y, int64_t ldy,
                                float* resid, float* sigma2, double* state, int* info, int N, int T, void* stream) {
    return kron_prologue_warm<float>(raw_vol, covar_factor, raw_var, raw_task_noises, raw_noise, x, Y, ldy, resid, sigma2, state,
                                     info, N, T, stream);
}

int volt_kron_prologue_warm_f64(const double* raw_vol, const double* covar_factor, const double* raw_var,
                                const double* raw_task_noises, const double* raw_noise, const double* x, const double* Y,
                                int64_t ldy, double* resid, double* sigma2, double* state, int* info, int N, int T, void* stream) {
    return kron_prologue_warm<double>(raw_vol, covar_factor, raw_var, raw_task_noises, raw_noise, x, Y, ldy, resid, sigma2, state,
                                      info, N, T, stream);
}

int volt_kron_epilogue_ws_f32(const float* raw_vol, const float* covar_factor, const float* raw_var, const float* raw_task_noises,
                              const float* raw_noise, const float* x, const float* resid, const float* out, const float* alpha,
                              const double* state, float* res, void* workspace, int N, int T, void* stream) {
    return kron_epilogue_ws<float>(raw_vol, covar_factor, raw_var, raw_task_noises, raw_noise, x, resid, out, alpha, state, res,
                                   workspace, N, T, stream);
}

int volt_kron_epilogue_ws_f64(const double* raw_vol, const double* covar_factor, const double* raw_var,
                              const double* raw_task_noises, const double* raw_noise, const double* x, const double* resid,
                              const double* out, const double* alpha, const double* state, double* res, void* workspace, int N,
                              int T, void* stream) {
    return kron_epilogue_ws<double>(raw_vol, covar_factor, raw_var, raw_task_noises, raw_noise, x, resid, out, alpha, state, res,
                                    workspace, N, T, stream);
}

}  // extern "C"
