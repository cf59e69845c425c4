// The T x T task algebra of the multi-task GPCV steps, ONE text for mt_task_kernel (gpcv_mt.hip: dense prior, fp32 partial
// sums) and mtm::task_kernel (gpcv_mt_markov.hip: Markov family, fp64 partial sums).  One workgroup of nt threads, fp64 in
// LDS: T x T matrices with row stride MLD.  Each kernel keeps its prologue (where tau_x, ell, colpart and R'A or G come
// from, in which type) and its epilogue (the out layout, kti / cinv / tsc); the steps between are these functions, in this
// order.  Device code only, all __forceinline__; every sum has a fixed order.
#pragma once
#include "gpcv_shared.h"
#include <math.h>

namespace volt {

constexpr int TASK_NT = 1024;         // threads of the task-algebra workgroup at most (sred, sgrp are sized by it)

__device__ __forceinline__ double msoftplus(double v) { return v > 20.0 ? v : log1p(exp(v)); }
__device__ __forceinline__ double msigmoid(double v) { return 1.0 / (1.0 + exp(-v)); }

// v[0..3] <- their sums over the workgroup: wsum inside each wave, then the waves in order (two barriers).  The two steps
// sum a wave with different butterflies, which round differently: the caller says which.  sred: 4 (TASK_NT / 64) doubles.
template <class WaveSum>
__device__ __forceinline__ void task_block_sum4(double (&v)[4], double* sred, WaveSum wsum) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const double w = wsum(v[k]);
        if (lane == 0) sred[k * (TASK_NT / 64) + wave] = w;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        double s = 0.0;
        for (int w = 0; w < nw; ++w) s += sred[k * (TASK_NT / 64) + w];
        v[k] = s;
    }
    __syncthreads();
}

// sC <- K_t = f f' + diag softplus(raw_var)
__device__ __forceinline__ void task_build_kt(double* sC, const double* sf, const float* raw_var, int T) {
    const int tid = threadIdx.x, nt = blockDim.x;
    for (int e = tid; e < T * T; e += nt) {
        const int i = e / T, j = e - i * T;
        sC[i * MLD + j] = sf[i] * sf[j] + (i == j ? msoftplus((double)raw_var[i]) : 0.0);
    }
}

// scol[t] = sum_blk colpart[blk, t]: nw strided partial sums per task (U rows in flight), added in order.  One barrier; scol
// is published by the caller's next one.  sgrp: TASK_NT doubles.
template <int U, class CT>
__device__ __forceinline__ void task_colsum(const CT* colpart, int ngh, int T, double* sgrp, double* scol) {
    const int tid = threadIdx.x, nw = blockDim.x >> 6;
    {
        const int t = tid & 63, g = tid >> 6;
        double acc = 0.0;
        if (t < T) {
#pragma unroll U
            for (int b = g; b < ngh; b += nw) acc += (double)colpart[(int64_t)b * T + t];
        }
        sgrp[g * 64 + t] = acc;
    }
    __syncthreads();
    if (tid < T) {
        double s = 0.0;
        for (int g = 0; g < nw; ++g) s += sgrp[g * 64 + tid];
        scol[tid] = s;
    }
}

// C = chol(K_t) right-looking in place (strictly lower part of sC; the pivots go to spiv) and, in the same sweep, sI = C^-1
// by right-looking forward substitution (row j is final once divided by its pivot, then leaves every row below it): two
// barriers per column.  Every thread takes the pivot's root itself, so no thread waits for thread 0.  *sbad (0 on entry)
// becomes j + 1 for the first pivot that is <= 0 or NaN; everything downstream of it is NaN.
__device__ __forceinline__ void task_chol_inverse(double* sC, double* sI, double* spiv, int* sbad, int T) {
    const int tid = threadIdx.x, nt = blockDim.x, TT = T * T;
    for (int e = tid; e < TT; e += nt) sI[(e / T) * MLD + e % T] = e / T == e % T ? 1.0 : 0.0;
    __syncthreads();
    for (int j = 0; j < T; ++j) {
        double d = sC[j * MLD + j];
        const bool bad = !(d > 0.0);
        d = bad ? __builtin_nan("") : sqrt(d);
        if (tid == 0) {
            if (bad && !*sbad) *sbad = j + 1;
            spiv[j] = d;
        }
        for (int i = j + 1 + tid; i < T; i += nt) sC[i * MLD + j] /= d;
        for (int c = nt - 1 - tid; c <= j; c += nt) sI[j * MLD + c] /= d;        // (the last threads: the first scale C)
        __syncthreads();
        const int m = T - j - 1, cnt = m * T;
        for (int e = tid; e < cnt; e += nt) {
            const int i = j + 1 + e / T, c = e % T;
            if (c > j) {
                if (c <= i) sC[i * MLD + c] -= sC[i * MLD + j] * sC[c * MLD + j];
            } else {
                sI[i * MLD + c] -= sC[i * MLD + j] * sI[j * MLD + c];
            }
        }
        __syncthreads();
    }
}

// sK <- K_t^-1 = C^-T C^-1 (keep(e, s, t, value) stores what the kernel hands on), sC <- tril(Lt), sA <- U = K_t^-1 Lt;
// r[0..2] <- this thread's share of tau_t = tr(Lt' K_t^-1 Lt), logdet K_t, logdet S_t (r[3] untouched): the caller sums them
template <class Keep>
__device__ __forceinline__ void task_inverse_and_u(double* sC, const double* sI, double* sK, double* sA, const double* spiv,
                                                   const float* Lt, int T, double (&r)[4], Keep keep) {
    const int tid = threadIdx.x, nt = blockDim.x, TT = T * T;
    for (int e = tid; e < TT; e += nt) {
        const int s = e / T, t = e - s * T;
        double acc = 0.0;
        for (int k = s > t ? s : t; k < T; ++k) acc = fma(sI[k * MLD + s], sI[k * MLD + t], acc);
        sK[s * MLD + t] = acc;
        keep(e, s, t, acc);
    }
    for (int e = tid; e < TT; e += nt) {                  // (C itself is no longer needed)
        const int t = e / T, s = e - t * T;
        sC[t * MLD + s] = s <= t ? (double)Lt[e] : 0.0;
    }
    __syncthreads();
    for (int e = tid; e < TT; e += nt) {
        const int s = e / T, k = e - s * T;
        double acc = 0.0;
        for (int t = k; t < T; ++t) acc = fma(sK[s * MLD + t], sC[t * MLD + k], acc);
        sA[s * MLD + k] = acc;
    }
    __syncthreads();
    for (int e = tid; e < TT; e += nt) r[0] += sA[(e / T) * MLD + e % T] * sC[(e / T) * MLD + e % T];
    if (tid < T) {
        const double d = sC[tid * MLD + tid];
        r[1] = 2.0 * log(spiv[tid]);
        r[2] = log(d * d);
    }
}

// dF/dLt = we 2 colred_t Lt - wk (tau_x tril(U) - N diag(1 / Lt_tt))   (sC = tril(Lt), sA = U)
__device__ __forceinline__ void task_grad_lt(const double* sC, const double* sA, const double* scol, double tau_x, int N,
                                             double we, double wk, float* grad_Lt, int T) {
    const int tid = threadIdx.x, nt = blockDim.x;
    for (int e = tid; e < T * T; e += nt) {
        const int t = e / T, s = e - t * T;
        double g = 0.0;
        if (s <= t) {
            const double l = sC[t * MLD + s];
            double kl = tau_x * sA[t * MLD + s];
            if (s == t) kl -= (double)N / l;
            g = we * 2.0 * scol[t] * l - wk * kl;
        }
        grad_Lt[e] = (float)g;
    }
}

// With sC = R'A (or G) and scs = colsum A published:  sI <- Z = K_t^-1 sC,  sC <- H = dKL/dK_t = 1/2 (N K_t^-1 - tau_x U U'
// - Z K_t^-1), pushed through K_t = f f' + diag softplus(raw_var) to covar_factor and raw_var;  grad_c = wk colsum(A) K_t^-1
__device__ __forceinline__ void task_push_through(double* sC, double* sI, const double* sK, const double* sA, const double* sf,
                                                  const double* scs, double tau_x, int N, double wk, const float* raw_var,
                                                  float* grad_cf, float* grad_rv, float* grad_c, int T) {
    const int tid = threadIdx.x, nt = blockDim.x, TT = T * T;
    for (int e = tid; e < TT; e += nt) {
        const int s = e / T, k = e - s * T;
        double acc = 0.0;
        for (int t = 0; t < T; ++t) acc = fma(sK[s * MLD + t], sC[t * MLD + k], acc);
        sI[s * MLD + k] = acc;
    }
    __syncthreads();
    for (int e = tid; e < TT; e += nt) {
        const int s = e / T, t = e - s * T;
        double uu = 0.0, zk = 0.0;
        for (int k = 0; k < T; ++k) {
            uu = fma(sA[s * MLD + k], sA[t * MLD + k], uu);
            zk = fma(sI[s * MLD + k], sK[k * MLD + t], zk);
        }
        sC[s * MLD + t] = 0.5 * ((double)N * sK[s * MLD + t] - tau_x * uu - zk);
    }
    __syncthreads();
    if (tid < T) {
        const int t = tid;
        double hf = 0.0, gc = 0.0;
        for (int s = 0; s < T; ++s) {
            hf = fma(sC[t * MLD + s] + sC[s * MLD + t], sf[s], hf);       // K_t = f f' + diag: dKL/df = (H + H') f
            gc = fma(scs[s], sK[s * MLD + t], gc);
        }
        grad_cf[t] = (float)(-wk * hf);
        grad_rv[t] = (float)(-wk * sC[t * MLD + t] * msigmoid((double)raw_var[t]));
        grad_c[t] = (float)(wk * gc);                                      // dKL/dc_t = - sum_n (A K_t^-1)_nt
    }
}

}  // namespace volt
