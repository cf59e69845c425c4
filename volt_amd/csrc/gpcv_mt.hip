// Multi-task GPCV: one ELBO + gradient step of the Kronecker variational GP over T series that share the time grid
//   reference: voltron/models/multi_task_variational_gp.py (MultitaskVariationalGP, :11-146); the ELBO arithmetic is
//   gpytorch's VariationalELBO over a MultitaskMultivariateNormal, as in gpcv.hip for one series.
//     q(F) = N(M, S_x (x) S_t),  S_x = Lx Lx',  S_t = Lt Lt'        p(F) = N(mu, (K_x + j I) (x) K_t),  mu[n,t] = c_t
//     K_t  = f f' + diag(softplus(raw_var))                          (IndexKernel, rank 1)
//     ell  = sum_nt GH_Q[ log N(y_nt; 0, max(exp f, min_scale)) ],  f ~ N(M_nt, max(vx_n vt_t, min_var))
//     KL   = 1/2 [ tau_x tau_t + q - N T + T logdet K + N logdet K_t - T logdet S_x - N logdet S_t ]
//            tau_x = |L^-1 Lx|_F^2,  tau_t = tr(K_t^-1 S_t),  A = K^-1 R,  R = M - mu,  q = tr(K_t^-1 R'A)
// Every N^3 piece is the single-series step's at B = 1: ONE factorisation of K_x + jI (volt_mll_step_f32: L, Y = L^-T,
// logdet, tr K^-1), T' = Lx' L^-T and G = K^-1 Lx on the structured GEMM (gpcv.hip).  The T right-hand sides ride on the
// same MFMA core as one 128-row tile: V = R' L^-T, A' = V Y'.  New here: the N x T quadrature pass, the deterministic
// partial sums of R'A / A'A, ONE fp64 workgroup for everything T x T, and the gradient kernels.
// The copula-process ("cv") likelihood with one warp per task (volt_gpcv_mt_cv_step_f32) is the same launch sequence with
// the quadrature pass of gpcv_mt_cv.hip in place of mt_gh_kernel.
#include "common.h"
#include "gpcv_task.h"
#include "../../include/volt_hip.h"
#include <math.h>

namespace volt {

// (MT_MAX, MLD and GH_ROWS are in gpcv_shared.h: the "cv" quadrature pass of gpcv_mt_cv.hip has the same layout; the task
// algebra and its workgroup size TASK_NT are in gpcv_task.h)
constexpr int RT_CH = 64;             // columns n staged per pass of the partial sums of R'A / A'A
constexpr int RT_PASSES = 1;          // passes per workgroup: RT_CH * RT_PASSES columns per partial

// Rt [128, Np] = (M - c)' zero padded: the T right-hand sides as rows of one MFMA tile (row 0 doubles as the exact-GP
// step's residual).
__global__ __launch_bounds__(256) void mt_resid_kernel(const float* __restrict__ M, const float* __restrict__ c,
                                                       float* __restrict__ Rt, int N, int Np, int T) {
    const int t = blockIdx.y, n = blockIdx.x * 256 + threadIdx.x;
    if (n >= Np) return;
    float v = 0.f;
    if (t < T && n < N) v = M[(int64_t)n * T + t] - c[t];
    Rt[(int64_t)t * Np + n] = v;
}

// vx[i] = sum_{j<=i} Lx_ij^2 and log Lx_ii^2, one wave per row (coalesced row read).
__global__ __launch_bounds__(256) void mt_rowsq_kernel(const float* __restrict__ Lx, float* __restrict__ vx,
                                                       float* __restrict__ logd, int N) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int i = blockIdx.x * 4 + wave;
    if (i >= N) return;
    const float* row = Lx + (int64_t)i * N;
    float s2 = 0.f;
    for (int j = lane; j <= i; j += 64) {
        const float v = row[j];
        s2 += v * v;
    }
    s2 = wave_sum_f(s2);
    if (lane == 0) {
        const float d = row[i];
        vx[i] = s2;
        logd[i] = logf(d * d);
    }
}

// The N x T Gauss-Hermite pass.  One thread per (n, t), GH_ROWS rows per workgroup: f = M_nt + sqrt(2 var) x_k,
// s = max(exp f, min_scale), logp = -y^2 / (2 s^2) - log s - log sqrt(2 pi), dlogp/df = (y^2/s^2 - 1) [exp f > min_scale].
//   gm [N,T] = dE/dM;  rowred[n] = sum_t gv_nt vt_t;  colpart[blk, t] = sum_{n in blk} gv_nt vx_n;  ellpart[blk].
// gv = dE/dvar (0 where the variance is floored).  The sums run in a fixed order: no atomics.
__global__ __launch_bounds__(256) void mt_gh_kernel(const float* __restrict__ M, const float* __restrict__ Lt,
                                                    const float* __restrict__ y, const float* __restrict__ vx,
                                                    const float* __restrict__ ghx, const float* __restrict__ ghw, int Q,
                                                    float min_var, float min_scale, float* __restrict__ gm,
                                                    float* __restrict__ rowred, float* __restrict__ colpart,
                                                    float* __restrict__ ellpart, int N, int T) {
    __shared__ float svt[MT_MAX], sx[GH_ROWS], sre[GH_ROWS];
    __shared__ float sgv[GH_ROWS][MLD], sel[GH_ROWS][MLD];
    const int tid = threadIdx.x, r0 = blockIdx.x * GH_ROWS;
    if (tid < T) {
        float s2 = 0.f;
        for (int s = 0; s <= tid; ++s) {
            const float v = Lt[tid * T + s];
            s2 += v * v;
        }
        svt[tid] = s2;
    }
    if (tid >= 64 && tid < 64 + GH_ROWS) sx[tid - 64] = r0 + tid - 64 < N ? vx[r0 + tid - 64] : 0.f;
    __syncthreads();
    const float lms = logf(min_scale);
    for (int e = tid; e < GH_ROWS * T; e += 256) {
        const int rr = e / T, t = e - rr * T, n = r0 + rr;
        float el = 0.f, g1 = 0.f, g2 = 0.f;
        if (n < N) {
            float var = sx[rr] * svt[t];
            const bool floored = var < min_var;
            if (floored) var = min_var;
            const float mi = M[(int64_t)n * T + t], yi = y[(int64_t)n * T + t];
            const float sd2 = sqrtf(2.f * var);
            for (int k = 0; k < Q; ++k) {
                const float xk = ghx[k], wk = ghw[k];
                const ExpNode nd = exp_node(mi + sd2 * xk, yi, min_scale, lms);
                el += wk * nd.logp;
                g1 += wk * nd.g;
                g2 += wk * nd.g * xk;
            }
            g2 = floored ? 0.f : g2 / sd2;               // df/dvar = x_k / sqrt(2 var)
            gm[(int64_t)n * T + t] = g1;
        }
        sgv[rr][t] = g2;
        sel[rr][t] = el;
    }
    __syncthreads();
    if (tid < GH_ROWS) {
        float a = 0.f, b = 0.f;
        for (int t = 0; t < T; ++t) {
            a += sgv[tid][t] * svt[t];
            b += sel[tid][t];
        }
        if (r0 + tid < N) rowred[r0 + tid] = a;
        sre[tid] = b;
    }
    if (tid >= 64 && tid < 64 + T) {
        const int t = tid - 64;
        float a = 0.f;
        for (int rr = 0; rr < GH_ROWS; ++rr) a += sgv[rr][t] * sx[rr];
        colpart[(int64_t)blockIdx.x * T + t] = a;
    }
    __syncthreads();
    if (tid == 0) {
        float a = 0.f;
        for (int rr = 0; rr < GH_ROWS; ++rr) a += sre[rr];
        ellpart[blockIdx.x] = a;
    }
}

// Partial sums over a chunk of RT_CH * RT_PASSES columns n:  part[blk] = { (R'A)[s,t], (A'A)[s,t], sum_n A[n,s] }  ([2 T^2 + T] floats),
// from Rt and At ([128, Np], the T rows used).  The task kernel adds the chunks in order.
__global__ __launch_bounds__(256) void mt_rta_kernel(const float* __restrict__ Rt, const float* __restrict__ At,
                                                     float* __restrict__ part, int N, int Np, int T) {
    __shared__ float sr[MT_MAX][RT_CH + 1], sa[MT_MAX][RT_CH + 1];
    const int tid = threadIdx.x, TT = T * T;
    constexpr int PPT = MT_MAX * MT_MAX / 256;
    float ra[PPT], aa[PPT], cs = 0.f;
#pragma unroll
    for (int k = 0; k < PPT; ++k) ra[k] = aa[k] = 0.f;
    for (int pass = 0; pass < RT_PASSES; ++pass) {
        const int c0 = (blockIdx.x * RT_PASSES + pass) * RT_CH;
        if (c0 >= N) break;
        __syncthreads();
        for (int e = tid; e < T * RT_CH; e += 256) {
            const int s = e / RT_CH, c = e - s * RT_CH, n = c0 + c;
            sr[s][c] = n < N ? Rt[(int64_t)s * Np + n] : 0.f;
            sa[s][c] = n < N ? At[(int64_t)s * Np + n] : 0.f;
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < PPT; ++k) {
            const int p = tid + k * 256;
            if (p < TT) {
                const int s = p / T, t = p - s * T;
                float r = ra[k], a = aa[k];
#pragma unroll 8
                for (int c = 0; c < RT_CH; ++c) {
                    const float at = sa[t][c];
                    r = fmaf(sr[s][c], at, r);
                    a = fmaf(sa[s][c], at, a);
                }
                ra[k] = r;
                aa[k] = a;
            }
        }
        if (tid < T)
            for (int c = 0; c < RT_CH; ++c) cs += sa[tid][c];
    }
    float* o = part + (int64_t)blockIdx.x * (2 * TT + T);
#pragma unroll
    for (int k = 0; k < PPT; ++k) {
        const int p = tid + k * 256;
        if (p < TT) {
            o[p] = ra[k];
            o[TT + p] = aa[k];
        }
    }
    if (tid < T) o[2 * TT + tid] = cs;
}

struct MtTaskArgs {
    const float *cf, *raw_var, *Lt;
    const float* part;        // [nch, 2 T^2 + T]
    const float* colpart;     // [ngh, T]
    const float* ellpart;     // [ngh]
    const float *logd, *frobT, *frobG, *mllout;
    float *out, *grad_c, *grad_Lt, *grad_cf, *grad_rv, *kti, *cinv, *tsc;
    int* info_t;
    int nch, ngh, ntiles, N, T;
    float jitter, we, wk;
};

// the DESCENDING butterfly (offsets 32 .. 1); markov_scan.h's wave_sum_d is the ascending one, which rounds differently
__device__ __forceinline__ double wave_sum_d_desc(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// Everything T x T, one workgroup (256 threads up to T = 16, 1024 above), fp64 in LDS: K_t from the raw parameters,
// C = chol(K_t), C^-1, K_t^-1, U = K_t^-1 Lt, tau_t, the chunk sums of R'A / A'A / colsum A, q, both task log-determinants,
// H = dKL/dK_t pushed through to covar_factor and raw_var, grad_Lt, grad_c, and the step's scalars.  Sums over lists are
// per-thread strided sums, a butterfly inside each wave, then the waves in order: a fixed order, three block reductions in
// all.  Leaves K_t^-1 and C^-1 (fp32) and {tau_t, tau_x} for the kernels that follow.
__global__ __launch_bounds__(TASK_NT) void mt_task_kernel(MtTaskArgs a) {
    __shared__ double sC[MT_MAX * MLD], sI[MT_MAX * MLD], sK[MT_MAX * MLD], sA[MT_MAX * MLD];
    __shared__ double sgrp[TASK_NT], sred[4 * (TASK_NT / 64)];
    __shared__ double sf[MT_MAX], scs[MT_MAX], scol[MT_MAX], spiv[MT_MAX];
    __shared__ int sbad;
    const int tid = threadIdx.x, nt = blockDim.x, T = a.T, TT = T * T, N = a.N;
    auto block_sum4 = [&](double (&v)[4]) { task_block_sum4(v, sred, [](double x) { return wave_sum_d_desc(x); }); };
    if (tid < T) sf[tid] = (double)a.cf[tid];
    if (tid == 0) sbad = 0;
    // the sums that need nothing of the T x T algebra: tau_x = |T'|_F^2, |G|_F^2, ell, logdet S_x
    double r0[4] = {0.0, 0.0, 0.0, 0.0};
    for (int i = tid; i < a.ntiles; i += nt) {
        r0[0] += (double)a.frobT[i];
        r0[1] += (double)a.frobG[i];
    }
#pragma unroll 4
    for (int i = tid; i < a.ngh; i += nt) r0[2] += (double)a.ellpart[i];
#pragma unroll 8
    for (int i = tid; i < N; i += nt) r0[3] += (double)a.logd[i];
    block_sum4(r0);                                       // (its barriers publish sf and sbad)
    const double tau_x = r0[0], gg = r0[1], ell = r0[2], ld_sx = r0[3];
    task_build_kt(sC, sf, a.raw_var, T);
    task_colsum<8>(a.colpart, a.ngh, T, sgrp, scol);
    task_chol_inverse(sC, sI, spiv, &sbad, T);
    double r1[4] = {0.0, 0.0, 0.0, 0.0};
    task_inverse_and_u(sC, sI, sK, sA, spiv, a.Lt, T, r1, [&](int e, int s, int t, double v) {
        a.kti[e] = (float)v;
        a.cinv[e] = (float)sI[s * MLD + t];
    });
    block_sum4(r1);
    const double tau_t = r1[0], ld_kt = r1[1], ld_st = r1[2];
    task_grad_lt(sC, sA, scol, tau_x, N, (double)a.we, (double)a.wk, a.grad_Lt, T);
    __syncthreads();
    // sC <- R'A (chunks in order);  tr(K_t^-1 A'A);  colsum A
    const int pstride = 2 * TT + T;
    double r2[4] = {0.0, 0.0, 0.0, 0.0};
    for (int e = tid; e < TT; e += nt) {
        const int s = e / T, t = e - s * T;
        double ra = 0.0, aa = 0.0;
#pragma unroll 8
        for (int c = 0; c < a.nch; ++c) {
            ra += (double)a.part[(int64_t)c * pstride + e];
            aa += (double)a.part[(int64_t)c * pstride + TT + e];
        }
        sC[s * MLD + t] = ra;
        r2[0] += aa * sK[t * MLD + s];
        r2[1] += ra * sK[t * MLD + s];                    // q = tr(K_t^-1 R'A)
    }
    if (tid < T) {
        double cs = 0.0;
#pragma unroll 8
        for (int c = 0; c < a.nch; ++c) cs += (double)a.part[(int64_t)c * pstride + 2 * TT + tid];
        scs[tid] = cs;
    }
    block_sum4(r2);                                       // (its barriers publish sC and scs)
    const double tr_aa = r2[0], q = r2[1];
    task_push_through(sC, sI, sK, sA, sf, scs, tau_x, N, (double)a.wk, a.raw_var, a.grad_cf, a.grad_rv, a.grad_c, T);
    if (tid == 0) {
        const double ld_k = (double)a.mllout[3];
        const double kl = 0.5 * (tau_x * tau_t + q - (double)N * T + T * ld_k + N * ld_kt - T * ld_sx - N * ld_st);
        float* o = a.out;
        o[0] = (float)ell;
        o[1] = (float)kl;
        o[2] = (float)q;
        o[3] = (float)ld_k;
        o[4] = (float)ld_kt;
        o[5] = (float)ld_sx;
        o[6] = (float)ld_st;
        o[7] = (float)tau_x;
        o[8] = (float)tau_t;
        o[9] = a.mllout[4];
        o[10] = (float)gg;
        o[11] = (float)tr_aa;
        o[12] = (float)((double)a.we * ell - (double)a.wk * kl);
        o[13] = a.jitter;
        o[14] = 0.f;
        o[15] = 0.f;
        a.tsc[0] = (float)tau_t;
        a.tsc[1] = (float)tau_x;
        a.info_t[0] = sbad;
        a.info_t[1] = (o[12] - o[12] == 0.f) ? 0 : 1;     // F is not finite (NaN / inf somewhere in the inputs)
    }
}

// Gradient of F = we ell - wk KL:
//   dF/dLx[i,j] = we 2 rowred_i Lx_ij - wk (tau_t G_ij - [i == j] T / Lx_ii)   (j <= i, zero above),
//   dF/dM[n,t]  = we gm_nt - wk (A K_t^-1)_nt.
__global__ __launch_bounds__(256) void mt_grad_kernel(const float* __restrict__ Lx, const float* __restrict__ G,
                                                      const float* __restrict__ rowred, const float* __restrict__ gm,
                                                      const float* __restrict__ At, const float* __restrict__ kti,
                                                      const float* __restrict__ tsc, float* __restrict__ gLx,
                                                      float* __restrict__ gM, int N, int Np, int T, float we, float wk) {
    const int i = blockIdx.y;                             // grid.y = max(N, T)
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j < N && i < N) {
        const int64_t e = (int64_t)i * N + j;
        float v = 0.f;
        if (j <= i) {
            const float l = Lx[e];
            float kl = tsc[0] * G[(int64_t)i * Np + j];
            if (j == i) kl -= (float)T / l;
            v = we * 2.f * rowred[i] * l - wk * kl;
        }
        gLx[e] = v;
    }
    if (i < T && j < N) {                                 // rows 0 .. T-1 of the grid double as the tasks: (n, t) = (j, i)
        float acc = 0.f;
        for (int s = 0; s < T; ++s) acc = fmaf(At[(int64_t)s * Np + j], kti[s * T + i], acc);
        gM[(int64_t)j * T + i] = we * gm[(int64_t)j * T + i] - wk * acc;
    }
}

// Bm [Np, 128] = A C^-T zero padded (C = chol(K_t)), so that A K_t^-1 A' = Bm Bm' is one NT product with K = 128.
__global__ __launch_bounds__(256) void mt_bmat_kernel(const float* __restrict__ At, const float* __restrict__ cinv,
                                                      float* __restrict__ Bm, int N, int Np, int T) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int i = (int)(idx >> 7), t = (int)(idx & 127);
    if (i >= Np) return;
    float acc = 0.f;
    if (i < N && t < T)
        for (int s = 0; s <= t; ++s) acc = fmaf(At[(int64_t)s * Np + i], cinv[t * T + s], acc);
    Bm[idx] = acc;
}

// dF/dK = -wk/2 (T K^-1 - tau_t G G' - A K_t^-1 A')  from P1 = T K^-1 - Bm Bm' and P2 = G G' (padded).
__global__ __launch_bounds__(256) void mt_dk_kernel(const float* __restrict__ P1, const float* __restrict__ P2,
                                                    const float* __restrict__ tsc, float* __restrict__ gK, int N, int Np,
                                                    float wk) {
    const int i = blockIdx.y;
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= N) return;
    const int64_t p = (int64_t)i * Np + j;
    gK[(int64_t)i * N + j] = -0.5f * wk * (P1[p] - tsc[0] * P2[p]);
}


struct MtWs {
    float *LxT, *W, *Tt, *G, *P1, *P2, *Bm, *Rt, *V, *At, *mllout, *beta, *vx, *logd, *rowred, *gm, *colpart, *ellpart,
        *part, *frobT, *frobG, *kti, *cinv, *tsc, *cvpart;
    void* mll;
    int ngh, nch;
    size_t bytes;
};

// Kc > 0: the "cv" step's layout, the "exp" one with the parameter partials [T, ngh, 3 Kc] appended.
static MtWs carve_mt(void* base, int N, int T, int want_dk, int Kc = 0) {
    const size_t Np = (size_t)volt_padded_n(N), n = Np / TS;
    Carver c{base};
    MtWs w;
    w.mll = base;
    c.skip(volt_mll_workspace_bytes(1, N, 1));
    w.ngh = (N + GH_ROWS - 1) / GH_ROWS;
    w.nch = (N + RT_CH * RT_PASSES - 1) / (RT_CH * RT_PASSES);
    w.LxT = c.take<float>(Np * Np);
    w.W = c.take<float>(Np * Np);
    w.Tt = c.take<float>(Np * Np);
    w.G = c.take<float>(Np * Np);
    w.P1 = c.take<float>(want_dk ? Np * Np : 0);
    w.P2 = c.take<float>(want_dk ? Np * Np : 0);
    w.Bm = c.take<float>(want_dk ? Np * TS : 0);
    w.Rt = c.take<float>(TS * Np);
    w.V = c.take<float>(TS * Np);
    w.At = c.take<float>(TS * Np);
    w.mllout = c.take<float>(8);
    w.beta = c.take<float>(N);
    w.vx = c.take<float>(N);
    w.logd = c.take<float>(N);
    w.rowred = c.take<float>(N);
    w.gm = c.take<float>((size_t)N * T);
    w.colpart = c.take<float>((size_t)w.ngh * T);
    w.ellpart = c.take<float>(w.ngh);
    w.part = c.take<float>((size_t)w.nch * (2 * (size_t)T * T + T));
    w.frobT = c.take<float>(n * n);
    w.frobG = c.take<float>(n * n);
    w.kti = c.take<float>((size_t)T * T);
    w.cinv = c.take<float>((size_t)T * T);
    w.tsc = c.take<float>(8);
    w.cvpart = c.take<float>(Kc > 0 ? (size_t)T * w.ngh * 3 * Kc : 0);
    w.bytes = c.off;
    return w;
}

// Both multi-task steps: abc == nullptr is the "exp" likelihood (volt_gpcv_mt_step_f32, whose launch sequence this is),
// otherwise the "cv" one -- only the quadrature pass differs.
static int mt_step_impl(const float* K, int64_t ldk, float jitter, const float* M, const float* c, const float* Lx,
                        const float* Lt, const float* covar_factor, const float* raw_var, const float* y, const float* abc,
                        int Kc, const float* gh_x, const float* gh_w, int Q, float min_var, float min_scale, float w_ell,
                        float w_kl, float* out, float* grad_M, float* grad_c, float* grad_Lx, float* grad_Lt,
                        float* grad_covar_factor, float* grad_raw_var, float* grad_K, float* grad_abc, int* info,
                        void* workspace, int N, int T, int ws_flags, void* stream) {
    hipStream_t s = (hipStream_t)stream;
    const int Np = volt_padded_n(N), n = Np / TS;
    const int64_t mat = (int64_t)Np * Np;
    const int want_dk = grad_K != nullptr;
    MtWs w = carve_mt(workspace, N, T, want_dk, abc ? Kc : 0);
    int rc;

    // what does not depend on the factorisation goes first: R', the row sums of squares, the quadrature pass, Lx'
    hipLaunchKernelGGL(mt_resid_kernel, dim3((Np + 255) / 256, TS), dim3(256), 0, s, M, c, w.Rt, N, Np, T);
    hipLaunchKernelGGL(mt_rowsq_kernel, dim3((N + 3) / 4), dim3(256), 0, s, Lx, w.vx, w.logd, N);
    if (abc) {
        if ((rc = launch_mt_cv_pass(M, Lt, y, w.vx, abc, Kc, gh_x, gh_w, Q, min_var, min_scale, w_ell, w.gm, w.rowred, w.colpart,
                                    w.ellpart, w.cvpart, grad_abc, N, T, s)))        // gpcv_mt_cv.hip
            return rc;
    } else {
        hipLaunchKernelGGL(mt_gh_kernel, dim3(w.ngh), dim3(256), 0, s, M, Lt, y, w.vx, gh_x, gh_w, Q, min_var, min_scale, w.gm,
                           w.rowred, w.colpart, w.ellpart, N, T);
    }
    if ((rc = launch_transpose_tri(Lx, N, 0, w.LxT, N, Np, 1, 1, s))) return rc;
    // K_x + jitter I = L L',  Y = L^-T,  logdet K, tr K^-1: the exact-GP step at B = 1, ONCE for all T series
    // (its own right-hand side is row 0 of R'; the T solves run on the GEMM below)
    rc = volt_mll_step_f32(K, ldk, 0, w.Rt, nullptr, jitter, w.mllout, w.beta, info, w.mll, 1, N,
                           VOLT_WANT_GRAD | (ws_flags & VOLT_WS_INITIALISED), stream);
    if (rc) return rc;
    const float* Y = volt_internal_mll_y(workspace, 1, N);
    if ((rc = launch_transpose_tri(Y, Np, mat, w.W, Np, Np, 2, 1, s))) return rc;
    // T' = Lx' L^-T (upper tiles; |T'|_F^2 = tau_x),  G = K^-1 Lx = Y T
    GemmArgs g1{w.LxT, w.W, w.Tt, Np, mat, Np, mat, Np, mat, n, n, n, 2, 1, 2, 1.f, 0.f, w.frobT};
    if ((rc = launch_gemm(g1, 1, s))) return rc;
    GemmArgs g2{Y, w.Tt, w.G, Np, mat, Np, mat, Np, mat, n, n, n, 2, 2, 0, 1.f, 0.f, w.frobG};
    if ((rc = launch_gemm(g2, 1, s))) return rc;
    // V = R' L^-T: rows of R' against rows of W = L^-1 (lower);  A' = V Y': rows of V against rows of Y (upper)
    GemmArgs g3{w.Rt, w.W, w.V, Np, 0, Np, 0, Np, 0, 1, n, n, 0, 1, 0, 1.f, 0.f, nullptr};
    if ((rc = launch_gemm(g3, 1, s))) return rc;
    GemmArgs g4{w.V, Y, w.At, Np, 0, Np, 0, Np, 0, 1, n, n, 0, 2, 0, 1.f, 0.f, nullptr};
    if ((rc = launch_gemm(g4, 1, s))) return rc;
    hipLaunchKernelGGL(mt_rta_kernel, dim3(w.nch), dim3(256), 0, s, w.Rt, w.At, w.part, N, Np, T);
    MtTaskArgs ta{covar_factor, raw_var, Lt, w.part, w.colpart, w.ellpart, w.logd, w.frobT, w.frobG, w.mllout,
                  out, grad_c, grad_Lt, grad_covar_factor, grad_raw_var, w.kti, w.cinv, w.tsc,
                  info + 1, w.nch, w.ngh, n * n, N, T, jitter, w_ell, w_kl};
    hipLaunchKernelGGL(mt_task_kernel, dim3(1), dim3(T <= 16 ? 256 : TASK_NT), 0, s, ta);
    hipLaunchKernelGGL(mt_grad_kernel, dim3((N + 255) / 256, N > T ? N : T), dim3(256), 0, s, Lx, w.G, w.rowred, w.gm, w.At, w.kti,
                       w.tsc, grad_Lx, grad_M, N, Np, T, w_ell, w_kl);
    if (want_dk) {
        hipLaunchKernelGGL(mt_bmat_kernel, dim3(Np * TS / 256), dim3(256), 0, s, w.At, w.cinv, w.Bm, N, Np, T);
        GemmArgs g5{Y, Y, w.P1, Np, mat, Np, mat, Np, mat, n, n, n, 2, 2, 0, (float)T, 0.f, nullptr};        // T K^-1 = T Y Y'
        if ((rc = launch_gemm(g5, 1, s))) return rc;
        GemmArgs g6{w.Bm, w.Bm, w.P1, TS, 0, TS, 0, Np, mat, n, n, 1, 0, 0, 0, -1.f, 1.f, nullptr};        // - Bm Bm'
        if ((rc = launch_gemm(g6, 1, s))) return rc;
        GemmArgs g7{w.G, w.G, w.P2, Np, mat, Np, mat, Np, mat, n, n, n, 0, 0, 0, 1.f, 0.f, nullptr};       // G G'
        if ((rc = launch_gemm(g7, 1, s))) return rc;
        hipLaunchKernelGGL(mt_dk_kernel, dim3((N + 255) / 256, N), dim3(256), 0, s, w.P1, w.P2, w.tsc, grad_K, N, Np, w_kl);
    }
    VOLT_LAUNCH_CHECK();
    return 0;
}

}  // namespace volt

using namespace volt;

extern "C" {

size_t volt_gpcv_mt_workspace_bytes(int N, int T, int want_dk) {
    if (N <= 0 || T < 1 || T > MT_MAX) return 0;
    return carve_mt(nullptr, N, T, want_dk).bytes;
}

int volt_gpcv_mt_step_f32(const float* K, int64_t ldk, float jitter, const float* M, const float* c, const float* Lx,
                          const float* Lt, const float* covar_factor, const float* raw_var, const float* y,
                          const float* gh_x, const float* gh_w, int Q, float min_var, float min_scale, float w_ell,
                          float w_kl, float* out, float* grad_M, float* grad_c, float* grad_Lx, float* grad_Lt,
                          float* grad_covar_factor, float* grad_raw_var, float* grad_K, int* info, void* workspace, int N,
                          int T, int ws_flags, void* stream) {
    if (!K) return -1;
    if (ldk < N) return -2;
    if (!M) return -4;
    if (!c) return -5;
    if (!Lx) return -6;
    if (!Lt) return -7;
    if (!covar_factor) return -8;
    if (!raw_var) return -9;
    if (!y) return -10;
    if (!gh_x) return -11;
    if (!gh_w) return -12;
    if (Q < 1 || Q > 1024) return -13;
    if (!out) return -18;
    if (!grad_M) return -19;
    if (!grad_c) return -20;
    if (!grad_Lx) return -21;
    if (!grad_Lt) return -22;
    if (!grad_covar_factor) return -23;
    if (!grad_raw_var) return -24;
    if (!info) return -26;
    if (!workspace || ((uintptr_t)workspace & 255)) return -27;
    if (N < 1) return -28;
    if (T < 1 || T > MT_MAX) return -29;
    return mt_step_impl(K, ldk, jitter, M, c, Lx, Lt, covar_factor, raw_var, y, nullptr, 0, gh_x, gh_w, Q, min_var, min_scale,
                        w_ell, w_kl, out, grad_M, grad_c, grad_Lx, grad_Lt, grad_covar_factor, grad_raw_var, grad_K, nullptr,
                        info, workspace, N, T, ws_flags, stream);
}

size_t volt_gpcv_mt_cv_workspace_bytes(int N, int T, int want_dk, int Kc) {
    if (N <= 0 || T < 1 || T > MT_MAX || Kc < 1 || Kc > VOLT_GPCV_CV_K_MAX) return 0;
    return carve_mt(nullptr, N, T, want_dk, Kc).bytes;
}

int volt_gpcv_mt_cv_step_f32(const float* K, int64_t ldk, float jitter, const float* M, const float* c, const float* Lx,
                             const float* Lt, const float* covar_factor, const float* raw_var, const float* y,
                             const float* abc, int Kc, const float* gh_x, const float* gh_w, int Q, float min_var,
                             float min_scale, float w_ell, float w_kl, float* out, float* grad_M, float* grad_c,
                             float* grad_Lx, float* grad_Lt, float* grad_covar_factor, float* grad_raw_var, float* grad_K,
                             float* grad_abc, int* info, void* workspace, int N, int T, int ws_flags, void* stream) {
    if (!K) return -1;
    if (ldk < N) return -2;
    if (!M) return -4;
    if (!c) return -5;
    if (!Lx) return -6;
    if (!Lt) return -7;
    if (!covar_factor) return -8;
    if (!raw_var) return -9;
    if (!y) return -10;
    if (!abc) return -11;
    if (Kc < 1 || Kc > VOLT_GPCV_CV_K_MAX) return -12;
    if (!gh_x) return -13;
    if (!gh_w) return -14;
    if (Q < 1 || Q > 1024) return -15;
    if (!out) return -20;
    if (!grad_M) return -21;
    if (!grad_c) return -22;
    if (!grad_Lx) return -23;
    if (!grad_Lt) return -24;
    if (!grad_covar_factor) return -25;
    if (!grad_raw_var) return -26;
    if (!grad_abc) return -28;
    if (!info) return -29;
    if (!workspace || ((uintptr_t)workspace & 255)) return -30;
    if (N < 1) return -31;
    if (T < 1 || T > MT_MAX) return -32;
    return mt_step_impl(K, ldk, jitter, M, c, Lx, Lt, covar_factor, raw_var, y, abc, Kc, gh_x, gh_w, Q, min_var, min_scale, w_ell,
                        w_kl, out, grad_M, grad_c, grad_Lx, grad_Lt, grad_covar_factor, grad_raw_var, grad_K, grad_abc, info,
                        workspace, N, T, ws_flags, stream);
}

}  // extern "C"
