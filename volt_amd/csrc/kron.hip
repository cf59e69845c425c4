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
#include <math.h>

#include "common.h"
#include "../../include/volt_hip.h"

namespace volt {

constexpr int KT_MAX = 64;          // largest T (tasks) the LDS-resident solver takes
constexpr int KLD = KT_MAX + 1;     // LDS row stride in doubles (odd: column walks spread over the banks)
constexpr int KNT = 1024;           // threads per workgroup
constexpr int KRB = 64;             // rows of R staged per prologue pass
constexpr int KCH = 32;             // columns of alpha / r staged per epilogue pass
constexpr int KCLD = KCH + 1;
constexpr int KSWEEPS = 30;         // sweep cap of the Jacobi solver
constexpr double KTOL = 1e-14;      // rotate (p,q) while |a_pq| > KTOL sqrt(|a_pp a_qq|)
constexpr double KNOISE_FLOOR = 1e-4;   // gpytorch's GreaterThan(1e-4) on both noise terms

// state written by the prologue (doubles): [0] vol, then Lambda [T], d [T], W [T,T], Q [T,T]
__host__ __device__ inline int kst_lam(int) { return 8; }
__host__ __device__ inline int kst_d(int T) { return 8 + T; }
__host__ __device__ inline int kst_w(int T) { return 8 + 2 * T; }
__host__ __device__ inline int kst_q(int T) { return 8 + 2 * T + T * T; }
__host__ __device__ inline int kst_len(int T) { return 8 + 2 * T + 2 * T * T; }

__device__ __forceinline__ double ksoftplus(double v) { return v > 20.0 ? v : log1p(exp(v)); }
__device__ __forceinline__ double ksigmoid(double v) { return 1.0 / (1.0 + exp(-v)); }

struct JacobiLds {
    double cs[KT_MAX];              // (c, s) of the pairs of one round
    int pq[KT_MAX];                 // (p, q) of the pairs of one round; p = -1: no rotation
    int flag;                       // a rotation happened in this sweep
    int rank[KT_MAX];
    double lam[KT_MAX];
};

// A, V: [T][KLD] in LDS.  A symmetric on entry; on return V holds the eigenvectors as columns and diag(A) the
// eigenvalues (unsorted).  Returns the sweeps used (the last one rotated nothing), or -1 if KSWEEPS were not enough.
__device__ int kron_jacobi(double* A, double* V, int T, JacobiLds& s) {
    const int tid = threadIdx.x;
    for (int e = tid; e < T * T; e += blockDim.x) {
        const int i = e / T, j = e - (e / T) * T;
        V[i * KLD + j] = i == j ? 1.0 : 0.0;
    }
    if (T == 1) {
        __syncthreads();
        return 0;
    }
    const int Tp = (T + 1) & ~1, m = Tp - 1, np = Tp / 2;    // odd T: one dummy index (= T) sits out a round
    int sweeps = 0;
    for (;;) {
        __syncthreads();                                      // everyone has read the last sweep's flag
        if (tid == 0) s.flag = 0;
        __syncthreads();
        for (int k = 0; k < m; ++k) {
            if (tid < np) {
                int p = tid == 0 ? k : (k + tid) % m;
                int q = tid == 0 ? m : (k - tid + m) % m;
                if (p > q) { const int t = p; p = q; q = t; }
                double c = 1.0, sn = 0.0;
                bool on = false;
                if (q < T) {
                    const double apq = A[p * KLD + q], app = A[p * KLD + p], aqq = A[q * KLD + q];
                    if (fabs(apq) > 1e-300 && fabs(apq) > KTOL * sqrt(fabs(app * aqq))) {
                        const double th = (aqq - app) / (2.0 * apq);
                        const double t = fabs(th) > 1e150 ? 0.5 / th : copysign(1.0, th) / (fabs(th) + sqrt(1.0 + th * th));
                        c = 1.0 / sqrt(1.0 + t * t);
                        sn = t * c;
                        on = true;
                    }
                }
                s.cs[2 * tid] = c;
                s.cs[2 * tid + 1] = sn;
                s.pq[2 * tid] = on ? p : -1;
                s.pq[2 * tid + 1] = q;
                if (on) s.flag = 1;
            }
            __syncthreads();
            for (int e = tid; e < np * T; e += blockDim.x) {    // rows p, q:  A <- J' A
                const int i = e / T, col = e - (e / T) * T;
                const int p = s.pq[2 * i];
                if (p < 0) continue;
                const int q = s.pq[2 * i + 1];
                const double c = s.cs[2 * i], sn = s.cs[2 * i + 1];
                const double ap = A[p * KLD + col], aq = A[q * KLD + col];
                A[p * KLD + col] = c * ap - sn * aq;
                A[q * KLD + col] = sn * ap + c * aq;
            }
            __syncthreads();
            for (int e = tid; e < np * T; e += blockDim.x) {    // columns p, q:  A <- A J,  V <- V J
                const int i = e / T, row = e - (e / T) * T;
                const int p = s.pq[2 * i];
                if (p < 0) continue;
                const int q = s.pq[2 * i + 1];
                const double c = s.cs[2 * i], sn = s.cs[2 * i + 1];
                const double bp = A[row * KLD + p], bq = A[row * KLD + q];
                A[row * KLD + p] = row == q ? 0.0 : c * bp - sn * bq;      // the annihilated pair is exactly zero
                A[row * KLD + q] = row == p ? 0.0 : sn * bp + c * bq;
                const double vp = V[row * KLD + p], vq = V[row * KLD + q];
                V[row * KLD + p] = c * vp - sn * vq;
                V[row * KLD + q] = sn * vp + c * vq;
            }
            __syncthreads();
        }
        ++sweeps;
        if (!s.flag) return sweeps;
        if (sweeps >= KSWEEPS) return -1;
    }
}

// After kron_jacobi: eigenvalues ascending into s.lam, the matching eigenvectors as the columns of Qout [T][KLD]
// (ties keep their index order).
__device__ void kron_sort(const double* A, const double* V, double* Qout, int T, JacobiLds& s) {
    const int tid = threadIdx.x;
    __syncthreads();
    if (tid < T) {
        const double li = A[tid * KLD + tid];
        int r = 0;
        for (int k = 0; k < T; ++k) {
            const double lk = A[k * KLD + k];
            r += (lk < li) || (lk == li && k < tid);
        }
        s.rank[tid] = r;
        s.lam[r] = li;
    }
    __syncthreads();
    for (int e = tid; e < T * T; e += blockDim.x) {
        const int t = e / T, i = e - (e / T) * T;
        Qout[t * KLD + s.rank[i]] = V[t * KLD + i];
    }
    __syncthreads();
}

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
    if (tid < T) {
        const double f = (double)cf[tid];
        sd[tid] = ksoftplus((double)rtn[tid]) + KNOISE_FLOOR + gnoise;
        sdiag[tid] = f * f + ksoftplus((double)raw_var[tid]);          // K_t[t,t]
    }
    __syncthreads();
    for (int e = tid; e < T * T; e += blockDim.x) {                     // S = D^-1/2 (F F' + diag(var)) D^-1/2
        const int i = e / T, j = e - (e / T) * T;
        const double kt = i == j ? sdiag[i] : (double)cf[i] * (double)cf[j];
        sA[i * KLD + j] = kt / sqrt(sd[i] * sd[j]);
    }
    __syncthreads();
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
    __shared__ double sX[2 * KT_MAX * KCLD];   // staged alpha | r chunks, then H, then G ([T][KLD] fits: 64 x 65 < 2 x 64 x 33)
    __shared__ double sP[KT_MAX * KLD];      // sum_n a_i r_j, then H W', then Q2 W'
    __shared__ double sQ[KT_MAX * KLD];      // sum_n a_i a_j, then Q2 = A~' A~
    __shared__ double sW[KT_MAX * KLD];
    __shared__ double sxc[KCH], su[KT_MAX], ssk[KT_MAX], slam[KT_MAX], stau[KT_MAX], sgd[KT_MAX], sax[KT_MAX];
    __shared__ double sard[KT_MAX], saad[KT_MAX];
    const int tid = threadIdx.x, TT = T * T;
    double* sa = sX;                          // [T][KCLD]
    double* sr = sX + KT_MAX * KCLD;          // [T][KCLD]
    constexpr int PPT = (KT_MAX * KT_MAX + KNT - 1) / KNT;
    double accr[PPT], acca[PPT], accu = 0.0;
#pragma unroll
    for (int k = 0; k < PPT; ++k) accr[k] = acca[k] = 0.0;
    for (int n0 = 0; n0 < N; n0 += KCH) {
        __syncthreads();
        for (int e = tid; e < T * KCH; e += blockDim.x) {
            const int i = e / KCH, c = e - (e / KCH) * KCH, n = n0 + c;
            sa[i * KCLD + c] = n < N ? (double)alpha[(int64_t)i * N + n] : 0.0;
            sr[i * KCLD + c] = n < N ? (double)resid[(int64_t)i * N + n] : 0.0;
        }
        if (tid < KCH) sxc[tid] = n0 + tid < N ? (double)x[n0 + tid] : 0.0;
        __syncthreads();
#pragma unroll
        for (int k = 0; k < PPT; ++k) {
            const int p = tid + k * KNT;
            if (p < TT) {
                const int i = p / T, j = p - (p / T) * T;
                double ar = accr[k], aa = acca[k];
#pragma unroll 4
                for (int c = 0; c < KCH; ++c) {
                    const double ai = sa[i * KCLD + c];
                    ar = fma(ai, sr[j * KCLD + c], ar);
                    aa = fma(ai, sa[j * KCLD + c], aa);
                }
                accr[k] = ar;
                acca[k] = aa;
            }
        }
        if (tid < T)
            for (int c = 0; c < KCH; ++c) accu = fma(sa[tid * KCLD + c], sxc[c], accu);
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < PPT; ++k) {
        const int p = tid + k * KNT;
        if (p < TT) {
            const int i = p / T, j = p - (p / T) * T;
            sP[i * KLD + j] = accr[k];
            sQ[i * KLD + j] = acca[k];
        }
    }
    const double vol = state[0];
    if (tid < T) {
        const double lam = state[kst_lam(T) + tid], kap = vol * lam;
        slam[tid] = lam;
        ssk[tid] = sqrt(kap);
        stau[tid] = (double)out[tid * 8 + 4] / kap;                     // tr (lambda K_x + I)^-1
        su[tid] = accu;                                                 // sum_n alpha_j[n] x_n (step scale)
    }
    for (int e = tid; e < TT; e += blockDim.x) sW[(e / T) * KLD + e - (e / T) * T] = state[kst_w(T) + e];
    __syncthreads();
    if (tid < T) {
        sard[tid] = sP[tid * KLD + tid];                                // a~_j' y~_j = a_j' r_j
        saad[tid] = sQ[tid * KLD + tid] / (ssk[tid] * ssk[tid]);        // a~_j' a~_j
    }
    // H = 1/2 [ sym(A~'(Y~ - A~) Lambda^-1) - diag(c) ],  A~'(Y~ - A~)[i,j] = ar_ij sk_j / sk_i - aa_ij / (sk_i sk_j)
    for (int e = tid; e < TT; e += blockDim.x) {
        const int i = e / T, j = e - (e / T) * T;
        const double pij = sP[i * KLD + j] * ssk[j] / ssk[i] - sQ[i * KLD + j] / (ssk[i] * ssk[j]);
        const double pji = sP[j * KLD + i] * ssk[i] / ssk[j] - sQ[j * KLD + i] / (ssk[i] * ssk[j]);
        double h = 0.25 * (pij / slam[j] + pji / slam[i]);
        if (i == j) h -= 0.5 * ((double)N - stau[i]) / slam[i];
        sX[i * KLD + j] = h;
    }
    __syncthreads();
    for (int e = tid; e < TT; e += blockDim.x) {                       // Q2 = A~' A~
        const int i = e / T, j = e - (e / T) * T;
        sQ[i * KLD + j] = sQ[i * KLD + j] / (ssk[i] * ssk[j]);
    }
    for (int e = tid; e < TT; e += blockDim.x) {                       // H W'
        const int i = e / T, t = e - (e / T) * T;
        double acc = 0.0;
        for (int j = 0; j < T; ++j) acc = fma(sX[i * KLD + j], sW[t * KLD + j], acc);
        sP[i * KLD + t] = acc;
    }
    __syncthreads();
    for (int e = tid; e < TT; e += blockDim.x) {                       // G = W H W'  (d log p / d K_t, covariance part)
        const int s_ = e / T, t = e - (e / T) * T;
        double acc = 0.0;
        for (int i = 0; i < T; ++i) acc = fma(sW[s_ * KLD + i], sP[i * KLD + t], acc);
        sX[s_ * KLD + t] = acc;
    }
    __syncthreads();
    for (int e = tid; e < TT; e += blockDim.x) {                       // Q2 W'
        const int i = e / T, t = e - (e / T) * T;
        double acc = 0.0;
        for (int j = 0; j < T; ++j) acc = fma(sQ[i * KLD + j], sW[t * KLD + j], acc);
        sP[i * KLD + t] = acc;
    }
    __syncthreads();
    if (tid < T) {
        const int t = tid;
        double q = 0.0, tw = 0.0, ax = 0.0;
        for (int i = 0; i < T; ++i) {
            const double w = sW[t * KLD + i];
            q = fma(w, sP[i * KLD + t], q);
            tw = fma(stau[i] * w, w, tw);
            ax = fma(w, su[i] / ssk[i], ax);                            // sum_n A[n,t] x_n,  A = A~ W'
        }
        sgd[t] = 0.5 * q - 0.5 * tw;                                    // d log p / d d_t
        sax[t] = ax;
        sX[t * KLD + t] += -0.5 * vol * vol * ax;                       // mean term of d log p / d K_t[t,t]
    }
    __syncthreads();
    const double scale = 1.0 / ((double)N * (double)T);
    if (tid < T) {
        const int t = tid;
        double gf = 0.0;
        for (int s_ = 0; s_ < T; ++s_) gf = fma(sX[t * KLD + s_], (double)cf[s_], gf);
        res[3 + t] = (R)(2.0 * gf * scale);
        res[3 + T + t] = (R)(sX[t * KLD + t] * ksigmoid((double)raw_var[t]) * scale);
        res[3 + 2 * T + t] = (R)(sgd[t] * ksigmoid((double)rtn[t]) * scale);
    }
    if (tid == 0) {
        double logp = 0.0, quad = 0.0, tr = 0.0, mterm = 0.0, gdsum = 0.0;
        for (int j = 0; j < T; ++j) {
            const double kap = ssk[j] * ssk[j];
            const double d = state[kst_d(T) + j];
            const double f = (double)cf[j];
            logp += (double)N * (double)out[j * 8] - 0.5 * (double)N * log(kap) - 0.5 * (double)N * log(d);
            quad += sard[j] - saad[j];
            tr += (double)N - stau[j];
            mterm += sax[j] * (f * f + ksoftplus((double)raw_var[j]));
            gdsum += sgd[j];
        }
        const double gvol = (0.5 * quad - 0.5 * tr) / vol - vol * mterm;
        res[0] = (R)(logp * scale);
        res[1] = (R)(gvol * vol * (1.0 - vol) * scale);
        res[2] = (R)(gdsum * ksigmoid((double)rn[0]) * scale);
    }
}

template <typename R>
int kron_prologue(const R* raw_vol, const R* cf, const R* raw_var, const R* rtn, const R* rn, const R* x, const R* Y,
                  int64_t ldy, R* resid, R* sigma2, double* state, int* info, int N, int T, void* stream) {
    if (!raw_vol) return -1;
    if (!cf) return -2;
    if (!raw_var) return -3;
    if (!rtn) return -4;
    if (!rn) return -5;
    if (!x) return -6;
    if (!Y) return -7;
    if (ldy < T) return -8;
    if (!resid) return -9;
    if (!sigma2) return -10;
    if (!state) return -11;
    if (!info) return -12;
    if (N < 1) return -13;
    if (T < 1 || T > KT_MAX) return -14;
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
