// Device code shared by the two translation units of the Kronecker multi-task step: csrc/kron.hip (the one-launch prologue
// and the one-workgroup epilogue around the dense batched step) and csrc/kron_chain.hip (the warm-started prologue and the
// epilogue with its N-reductions spread over workgroups, around the linear-time chain step).  Everything here is
// __forceinline__ into its callers: the kernels of kron.hip compile to the instructions they had when this code lived there.
#pragma once
#include <math.h>

#include "common.h"

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

// state written by the prologue (doubles): [0] vol, [1..7] spare (the warm prologue's stamp), then Lambda [T], d [T],
// W [T,T], Q [T,T]
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

// A, V: [T][KLD] in LDS, A symmetric and V orthogonal on entry (the barrier that publishes them is the first thing here).
// Cyclic Jacobi sweeps A <- J' A J, V <- V J until a sweep rotates nothing: with V = I on entry V holds the eigenvectors of A
// as columns and diag(A) the eigenvalues (unsorted); with A = V0' S V0, V = V0 on entry, those of S.  Returns the sweeps used
// (the last one rotated nothing), or -1 if KSWEEPS were not enough.
__device__ __forceinline__ int kron_jacobi_sweeps(double* A, double* V, int T, JacobiLds& s) {
    const int tid = threadIdx.x;
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

// The cold start: V = I, then the sweeps.  A symmetric on entry; on return V holds the eigenvectors as columns and diag(A)
// the eigenvalues (unsorted).
__device__ __forceinline__ int kron_jacobi(double* A, double* V, int T, JacobiLds& s) {
    const int tid = threadIdx.x;
    for (int e = tid; e < T * T; e += blockDim.x) {
        const int i = e / T, j = e - (e / T) * T;
        V[i * KLD + j] = i == j ? 1.0 : 0.0;
    }
    return kron_jacobi_sweeps(A, V, T, s);
}

// After kron_jacobi: eigenvalues ascending into s.lam, the matching eigenvectors as the columns of Qout [T][KLD]
// (ties keep their index order).  A NaN eigenvalue (a NaN parameter) ranks above every number, NaNs among themselves in
// index order: the ranks are a permutation whatever the diagonal holds, so every slot of s.lam and every column of Qout is
// written exactly once -- comparisons alone would rank every NaN 0, beside the smallest number, and leave the top slots
// holding whatever the LDS held before.
__device__ __forceinline__ void kron_sort(const double* A, const double* V, double* Qout, int T, JacobiLds& s) {
    const int tid = threadIdx.x;
    __syncthreads();
    if (tid < T) {
        const double li = A[tid * KLD + tid];
        const bool nan_i = li != li;
        int r = 0;
        for (int k = 0; k < T; ++k) {
            const double lk = A[k * KLD + k];
            r += nan_i ? (lk == lk || k < tid) : ((lk < li) || (lk == li && k < tid));
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

// d [T] and diag(K_t) [T] from the raw parameters, then S = D^-1/2 (F F' + diag(var)) D^-1/2 into A [T][KLD] (all in LDS);
// ends with a barrier.
template <typename R>
__device__ __forceinline__ void kron_form_s(const R* __restrict__ cf, const R* __restrict__ raw_var, const R* __restrict__ rtn,
                                            double gnoise, double* sd, double* sdiag, double* A, int T) {
    const int tid = threadIdx.x;
    if (tid < T) {
        const double f = (double)cf[tid];
        sd[tid] = ksoftplus((double)rtn[tid]) + KNOISE_FLOOR + gnoise;
        sdiag[tid] = f * f + ksoftplus((double)raw_var[tid]);          // K_t[t,t]
    }
    __syncthreads();
    for (int e = tid; e < T * T; e += blockDim.x) {                     // S = D^-1/2 (F F' + diag(var)) D^-1/2
        const int i = e / T, j = e - (e / T) * T;
        const double kt = i == j ? sdiag[i] : (double)cf[i] * (double)cf[j];
        A[i * KLD + j] = kt / sqrt(sd[i] * sd[j]);
    }
    __syncthreads();
}

// The epilogue's partial sums (csrc/kron_chain.hip): per slice of KSL columns of N, sum_n a_i r_j [T,T], sum_n a_i a_j [T,T],
// sum_n a_j x_n [T].  KSL is a compile-time constant, so the order of every sum is the same on every device.
constexpr int KSL = 256;
__host__ __device__ inline int64_t kws_stride(int T) { return 2 * (int64_t)T * T + T; }
__host__ __device__ inline int kws_slices(int N) { return (N + KSL - 1) / KSL; }

// The epilogue, in the three forms its kernels take (one code, so that the sums and the algebra cannot drift apart):
//   KRON_EPI_WHOLE  one workgroup: the sums over all of N reduced here out of LDS, then the T x T algebra for the MLL and the
//                   gradients of the five raw parameters -- kron_epilogue_kernel;
//   KRON_EPI_GRAM   workgroup b: the same sums over the columns [b KSL, (b + 1) KSL) of N only, written to block b of
//                   `partial`; no algebra -- kron_gram_kernel;
//   KRON_EPI_SUMMED one workgroup: the `nslices` blocks of `partial` added in slice order, then the algebra --
//                   kron_epilogue_ws_kernel.
enum { KRON_EPI_WHOLE = 0, KRON_EPI_GRAM = 1, KRON_EPI_SUMMED = 2 };

template <typename R, int MODE>
__device__ __forceinline__ void kron_epilogue_body(const R* raw_vol, const R* cf, const R* raw_var, const R* rtn, const R* rn,
                                                   const R* x, const R* resid, const R* out, const R* alpha, const double* state,
                                                   R* res, double* partial, int nslices, int N, int T) {
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
    const int64_t stride = kws_stride(T);
    if constexpr (MODE == KRON_EPI_SUMMED) {
#pragma unroll
        for (int k = 0; k < PPT; ++k) {
            const int p = tid + k * KNT;
            if (p < TT)
                for (int sl = 0; sl < nslices; ++sl) {
                    accr[k] += partial[sl * stride + p];
                    acca[k] += partial[sl * stride + TT + p];
                }
        }
        if (tid < T)
            for (int sl = 0; sl < nslices; ++sl) accu += partial[sl * stride + 2 * TT + tid];
    } else {
        const int n_lo = MODE == KRON_EPI_GRAM ? (int)blockIdx.x * KSL : 0;
        const int n_hi = MODE == KRON_EPI_GRAM ? (N - n_lo < KSL ? N : n_lo + KSL) : N;
        for (int n0 = n_lo; n0 < n_hi; n0 += KCH) {
            __syncthreads();
            for (int e = tid; e < T * KCH; e += blockDim.x) {
                const int i = e / KCH, c = e - (e / KCH) * KCH, n = n0 + c;
                sa[i * KCLD + c] = n < n_hi ? (double)alpha[(int64_t)i * N + n] : 0.0;
                sr[i * KCLD + c] = n < n_hi ? (double)resid[(int64_t)i * N + n] : 0.0;
            }
            if (tid < KCH) sxc[tid] = n0 + tid < n_hi ? (double)x[n0 + tid] : 0.0;
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
    }
    if constexpr (MODE == KRON_EPI_GRAM) {
        double* mine = partial + (int64_t)blockIdx.x * stride;
#pragma unroll
        for (int k = 0; k < PPT; ++k) {
            const int p = tid + k * KNT;
            if (p < TT) {
                mine[p] = accr[k];
                mine[TT + p] = acca[k];
            }
        }
        if (tid < T) mine[2 * TT + tid] = accu;
        return;
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

// The argument checks of the prologue entries (include/volt_hip.h), before any launch: 0, or the code of the first bad one.
inline int kron_prologue_check(const void* raw_vol, const void* cf, const void* raw_var, const void* rtn, const void* rn,
                               const void* x, const void* Y, int64_t ldy, const void* resid, const void* sigma2,
                               const void* state, const void* info, int N, int T) {
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
    return 0;
}

}  // namespace volt
