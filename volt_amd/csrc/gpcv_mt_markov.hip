// Multi-task GPCV ELBO + gradient step in O(N T (Q + T) + T^3): the Markov variational family under the Kronecker prior
// (MultitaskVariationalGP(prior_solver="markov")).  No N x N array anywhere.
//
//     p(F) = N(mu, K_M (x) K_t),  K_M = v min(x, x') + j 1 1'  (the level-jitter Brownian prior of gpcv_markov.hip: increments
//            q_0 = v x_0 + j, q_i = v (x_i - x_{i-1}), K_M^-1 exactly tridiagonal),  K_t = f f' + diag softplus(raw_var),  mu[n,t] = c_t
//     q(F) = N(M, P^-1 (x) S_t),  P = Lp Lp', Lp lower bidiagonal (diagonal e^rho_i, entry (i+1, i) gamma_i e^rho_i),  S_t = Lt Lt'
//     s_i = e^{-2 rho_i} + gamma_i^2 s_{i+1}  (diag P^-1),   e_0 = s_0,  e_i = e^{-2 rho_{i-1}} + (1 + gamma_{i-1})^2 s_i  (Var of the increment)
//     R = M - 1 c',  D_0 = R_0,  D_i = R_i - R_{i-1}  (T-vectors; c cancels for i > 0)
//     tau_x = sum e_i / q_i,  tau_t = tr(K_t^-1 S_t),  G = sum D_i D_i' / q_i,  G2 = sum Delta_i D_i D_i' / q_i^2,  quad = tr(K_t^-1 G)
//     KL = 1/2 [tau_x tau_t + quad - N T + T sum log q_i + N logdet K_t + 2 T sum rho_i - N logdet S_t]
// The x side (s, its adjoint sh) is T-independent: two affine scans over N alone, markov_scan.h's affine_scan (4 points a
// thread, 64 runs a wave, waves through LDS in order, chunks in order; s through its markov_var_scan, so it equals
// volt_markov_root_var_f32's bit for bit).  The task side is T x T: one fp64 workgroup running gpcv_task.h's task algebra, the
// one gpcv_mt.hip's mt_task_kernel runs, with G in the place of R'A.  Between them the N x T quadrature pass runs as a grid
// over row tiles, its nodes gpcv_shared.h's exp_node / cv_node.
//
// Four launches (five with the "cv" likelihood):
//   front  workgroup 0: s backward (-> workspace), tau_x, sum log q, sum rho, sum Delta/q, sum Delta e/q^2
//          workgroups 1 ..: the partial sums of G and G2 over MM_GCH rows each (they need nothing of the scan)
//   rows   the N x T Gauss-Hermite pass, MM_ROWS rows a workgroup: dE/dM, a_n = sum_t gv_nt st_t, and per workgroup the partial
//          sums of b_t = sum_n gv_nt s_n, of ell and of the 3 Kc "cv" parameter sums per task (KC = 0: "exp", a thread per
//          (n, t); KC > 0: "cv", a wave per task)          [+ cv_abc_reduce_kernel of gpcv.hip with the "cv" likelihood]
//   task   one workgroup, fp64 in LDS: K_t, its Cholesky factor and inverse, tau_t, the partial sums in fixed order, H pushed
//          through to covar_factor and raw_var, grad_Lt, grad_c, the scalars, info
//   back   workgroup 0: sh forward with grad_rho, grad_gamma;  workgroups 1 ..: grad_M = w_ell gm - w_kl A K_t^-1 over
//          MM_MROWS rows each, A_i = D_i / q_i - D_{i+1} / q_{i+1}
// No atomics, no host synchronisation; every sum has an order that depends on (N, T) alone.  Recurrences and sums fp64,
// the quadrature nodes and all I/O fp32.
#include "common.h"
#include "gpcv_task.h"
#include "markov_scan.h"
#include "../../include/volt_hip.h"
#include <math.h>

namespace volt {
namespace mtm {

constexpr int MM_T = MARKOV_VAR_T;         // threads of every workgroup but the task algebra's (8 waves)
constexpr int MM_W = MM_T / 64;
constexpr int MM_ROWS = 16;                // rows n per quadrature workgroup
constexpr int MM_GCH = 128;                // rows n per partial sum of G, G2
constexpr int MM_GST = 32;                 // ... staged in LDS per pass
constexpr int MM_PPT = MT_MAX * MT_MAX / MM_T;   // (s, t) pairs a thread of the partial sums owns
constexpr int MM_MROWS = 32;               // rows n per grad_M workgroup


// ---- front: workgroup 0 the x side's backward scan and sums (xs[0..4] = tau_x, sum log q, sum rho, sum Delta / q,
// sum Delta e / q^2; xs[5] = q_0), workgroups 1 .. the partial sums gpart[blk][2][T,T] of G and G2 over rows blk MM_GCH .. + MM_GCH
__global__ __launch_bounds__(MM_T) void front_kernel(const float* __restrict__ x, const float* __restrict__ vol, double jit,
                                                     const float* __restrict__ M, const float* __restrict__ c,
                                                     const float* __restrict__ rho, const float* __restrict__ gam,
                                                     double* __restrict__ ws_s, double* __restrict__ ws_e,
                                                     double* __restrict__ xs, double* __restrict__ gpart, int N, int T) {
    __shared__ double lds[2 * MM_W + 1];
    __shared__ double sd[MM_GST][MLD], sw1[MM_GST], sw2[MM_GST];
    const int tid = threadIdx.x;
    const int64_t n = N;
    const double v = (double)vol[0];
    if (blockIdx.x == 0) {
        double ldq = 0.0, srho = 0.0;
        for (int64_t i = tid; i < n; i += MM_T) {
            ldq += log(prior_inc(x, v, jit, i));
            srho += (double)rho[i];
        }
        markov_var_scan<MM_T, false>(rho, gam, ws_s, ws_e, n, lds);
        __syncthreads();
        double tx = 0.0, x1 = 0.0, x2 = 0.0;
        for (int64_t i = tid; i < n; i += MM_T) {
            const double q = prior_inc(x, v, jit, i), del = grid_step(x, i);
            double e = ws_s[i];
            if (i > 0) {
                const double o = 1.0 + (double)gam[i - 1];
                e = ws_e[i - 1] + o * o * e;                           // Var_q of the increment: no cancellation in this form
            }
            tx += e / q;
            x1 += del / q;
            x2 += del * e / (q * q);
        }
        tx = block_sum_d<MM_T>(tx, lds);
        ldq = block_sum_d<MM_T>(ldq, lds);
        srho = block_sum_d<MM_T>(srho, lds);
        x1 = block_sum_d<MM_T>(x1, lds);
        x2 = block_sum_d<MM_T>(x2, lds);
        if (tid == 0) {
            xs[0] = tx;
            xs[1] = ldq;
            xs[2] = srho;
            xs[3] = x1;
            xs[4] = x2;
            xs[5] = prior_inc(x, v, jit, 0);
        }
        return;
    }
    const int blk = blockIdx.x - 1, TT = T * T;
    const int64_t r0 = (int64_t)blk * MM_GCH;
    double g1[MM_PPT], g2[MM_PPT];
#pragma unroll
    for (int k = 0; k < MM_PPT; ++k) g1[k] = g2[k] = 0.0;
    for (int pass = 0; pass < MM_GCH / MM_GST; ++pass) {
        const int64_t c0 = r0 + pass * MM_GST;
        if (c0 >= n) break;
        __syncthreads();
        for (int e = tid; e < MM_GST * T; e += MM_T) {
            const int cc = e / T, t = e - cc * T;
            const int64_t i = c0 + cc;
            double d = 0.0;
            if (i < n) {
                const double mi = (double)M[i * T + t];
                d = i > 0 ? mi - (double)M[(i - 1) * T + t] : mi - (double)c[t];
            }
            sd[cc][t] = d;
        }
        if (tid < MM_GST) {
            const int64_t i = c0 + tid;
            double w1 = 0.0, w2 = 0.0;
            if (i < n) {
                const double q = prior_inc(x, v, jit, i);
                w1 = 1.0 / q;
                w2 = grid_step(x, i) / (q * q);
            }
            sw1[tid] = w1;
            sw2[tid] = w2;
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < MM_PPT; ++k) {
            const int p = tid + k * MM_T;
            if (p < TT) {
                const int s = p / T, t = p - s * T;
                double a1 = g1[k], a2 = g2[k];
#pragma unroll 4
                for (int cc = 0; cc < MM_GST; ++cc) {
                    const double pr = sd[cc][s] * sd[cc][t];
                    a1 = __builtin_fma(pr, sw1[cc], a1);
                    a2 = __builtin_fma(pr, sw2[cc], a2);
                }
                g1[k] = a1;
                g2[k] = a2;
            }
        }
    }
    double* o = gpart + (int64_t)blk * 2 * TT;
#pragma unroll
    for (int k = 0; k < MM_PPT; ++k) {
        const int p = tid + k * MM_T;
        if (p < TT) {
            o[p] = g1[k];
            o[TT + p] = g2[k];
        }
    }
}

// ---- rows: the N x T Gauss-Hermite pass over rows blockIdx.x MM_ROWS .. + MM_ROWS, variance max(s_n st_t, min_var).
//   gm [N,T] = dE/dM;  rowred[n] = a_n = sum_t gv_nt st_t;  colpart[blk, t] = sum_{n in blk} gv_nt s_n;  ellpart[blk];
//   KC > 0: cvpart[t][blk][3 KC].  gv = dE/dvar (0 where the variance is floored).
// KC = 0 ("exp"): a thread per (n, t), the node formulas of gpcv_mt.hip's mt_gh_kernel;  KC > 0 ("cv"): a wave per task
// with lane q on nodes q, q + 64, .., the 3 KC parameter sums of its task in registers across the rows (gpcv_mt_cv.hip's
// mt_gh_cv_kernel).  The per-point values are fp32; every sum over points is fp64 in a fixed order.
template <int KC>
__global__ __launch_bounds__(MM_T) void rows_kernel(const float* __restrict__ M, const float* __restrict__ Lt,
                                                    const float* __restrict__ y, const double* __restrict__ ws_s,
                                                    const float* __restrict__ abc, const float* __restrict__ ghx,
                                                    const float* __restrict__ ghw, int Q, float min_var, float min_scale,
                                                    float* __restrict__ gm, double* __restrict__ rowred,
                                                    double* __restrict__ colpart, double* __restrict__ ellpart,
                                                    float* __restrict__ cvpart, int N, int T) {
    __shared__ double svt[MT_MAX], sx[MM_ROWS], sre[MM_ROWS];
    __shared__ float sgv[MM_ROWS][MLD], sel[MM_ROWS][MLD];
    const int tid = threadIdx.x;
    const int64_t r0 = (int64_t)blockIdx.x * MM_ROWS;
    if (tid < T) {
        double s2 = 0.0;
        for (int s = 0; s <= tid; ++s) {
            const double v = (double)Lt[tid * T + s];
            s2 = __builtin_fma(v, v, s2);
        }
        svt[tid] = s2;
    }
    if (tid >= 64 && tid < 64 + MM_ROWS) sx[tid - 64] = r0 + tid - 64 < N ? ws_s[r0 + tid - 64] : 0.0;
    __syncthreads();
    if constexpr (KC == 0) {
        const float lms = logf(min_scale);
        for (int e = tid; e < MM_ROWS * T; e += MM_T) {
            const int rr = e / T, t = e - rr * T;
            const int64_t n = r0 + rr;
            float el = 0.f, g1 = 0.f, g2 = 0.f;
            if (n < N) {
                float var = (float)(sx[rr] * svt[t]);
                const bool floored = var < min_var;
                if (floored) var = min_var;
                const float mi = M[n * T + t], yi = y[n * T + t];
                const float sd2 = sqrtf(2.f * var);
                for (int k = 0; k < Q; ++k) {
                    const float xk = ghx[k], wq = ghw[k];
                    const ExpNode nd = exp_node(mi + sd2 * xk, yi, min_scale, lms);
                    el += wq * nd.logp;
                    g1 += wq * nd.g;
                    g2 += wq * nd.g * xk;
                }
                g2 = floored ? 0.f : g2 / sd2;               // df/dvar = x_k / sqrt(2 var)
                gm[n * T + t] = g1;
            }
            sgv[rr][t] = g2;
            sel[rr][t] = el;
        }
    } else {
        const int lane = tid & 63, wave = tid >> 6;
        for (int t = wave; t < T; t += MM_W) {
            float pa[KC], pb[KC], pc[KC], ga[KC], gb[KC], gc[KC];
            float bad = 0.f;                                     // 0, or NaN if a parameter of this task is NaN / inf
#pragma unroll
            for (int k = 0; k < KC; ++k) {
                pa[k] = abc[(t * 3 + 0) * KC + k];
                pb[k] = abc[(t * 3 + 1) * KC + k];
                pc[k] = abc[(t * 3 + 2) * KC + k];
                ga[k] = gb[k] = gc[k] = 0.f;
                bad += 0.f * pa[k] + 0.f * pb[k] + 0.f * pc[k];
            }
            const double vt = svt[t];
            for (int rr = 0; rr < MM_ROWS; ++rr) {
                const int64_t n = r0 + rr;
                float el = 0.f, g1 = 0.f, g2 = 0.f;
                if (n < N) {
                    float var = (float)(sx[rr] * vt);
                    const bool floored = var < min_var;
                    if (floored) var = min_var;
                    const float mi = M[n * T + t], yi = y[n * T + t];
                    const float sd2 = sqrtf(2.f * var);
                    for (int q = lane; q < Q; q += 64) {
                        const float xq = ghx[q];
                        cv_node<KC>(mi + sd2 * xq, xq, ghw[q], yi, min_scale, pa, pb, pc, ga, gb, gc, el, g1, g2);
                    }
                    el = wave_sum_f(el);
                    g1 = wave_sum_f(g1);
                    g2 = wave_sum_f(g2);
                    g2 = floored ? 0.f : g2 / sd2;               // df/dvar = x_q / sqrt(2 var)
                    if (lane == 0) gm[n * T + t] = g1;
                }
                if (lane == 0) {
                    sgv[rr][t] = g2;
                    sel[rr][t] = el + bad;                       // (the clamp would swallow a NaN scale: ell must show it)
                }
            }
            float* o = cvpart + ((int64_t)t * gridDim.x + blockIdx.x) * (3 * KC);
#pragma unroll
            for (int k = 0; k < KC; ++k) {
                const float ra = wave_sum_f(ga[k]), rb = wave_sum_f(gb[k]), rc = wave_sum_f(gc[k]);
                if (lane == 0) {
                    o[k] = ra;
                    o[KC + k] = rb;
                    o[2 * KC + k] = rc;
                }
            }
        }
    }
    __syncthreads();
    if (tid < MM_ROWS) {
        double a = 0.0, b = 0.0;
        for (int t = 0; t < T; ++t) {
            a = __builtin_fma((double)sgv[tid][t], svt[t], a);
            b += (double)sel[tid][t];
        }
        if (r0 + tid < N) rowred[r0 + tid] = a;
        sre[tid] = b;
    }
    if (tid >= 64 && tid < 64 + T) {
        const int t = tid - 64;
        double a = 0.0;
        for (int rr = 0; rr < MM_ROWS; ++rr) a = __builtin_fma((double)sgv[rr][t], sx[rr], a);
        colpart[(int64_t)blockIdx.x * T + t] = a;
    }
    __syncthreads();
    if (tid == 0) {
        double a = 0.0;
        for (int rr = 0; rr < MM_ROWS; ++rr) a += sre[rr];
        ellpart[blockIdx.x] = a;
    }
}

struct TaskArgs {
    const float *cf, *raw_var, *Lt, *M, *c;
    const double* gpart;      // [nch][2][T,T]
    const double* colpart;    // [ngh, T]
    const double* ellpart;    // [ngh]
    const double* xs;         // tau_x, sum log q, sum rho, sum Delta / q, sum Delta e / q^2, q_0
    float *out, *grad_c, *grad_Lt, *grad_cf, *grad_rv;
    double *kti, *tsc;
    int* info;
    int nch, ngh, N, T;
    float jitter;
    double we, wk;
};

// ---- task: everything T x T, one workgroup of TASK_NT threads, fp64 in LDS: the task algebra of gpcv_task.h (shared with
// gpcv_mt.hip's mt_task_kernel) with the x side's scalars read from xs, G in the place of R'A, tr(K_t^-1 G2) in the place of
// tr(K_t^-1 A'A) and colsum A = D_0 / q_0 (the rows of A = K_M^-1 R telescope).  The partial sums of G, G2 are added by
// TASK_NT / T^2 groups of threads striding over the chunks, then the groups in order.  Leaves K_t^-1 and tau_t (fp64) for
// the back kernel.
__global__ __launch_bounds__(TASK_NT) void task_kernel(TaskArgs a) {
    __shared__ double sC[MT_MAX * MLD], sI[MT_MAX * MLD], sK[MT_MAX * MLD], sA[MT_MAX * MLD];
    __shared__ double sgrp[TASK_NT], sgrp2[TASK_NT], sred[4 * (TASK_NT / 64)];
    __shared__ double sf[MT_MAX], scs[MT_MAX], scol[MT_MAX], spiv[MT_MAX];
    __shared__ int sbad;
    const int tid = threadIdx.x, nt = blockDim.x, T = a.T, TT = T * T, N = a.N;
    auto block_sum4 = [&](double (&v)[4]) { task_block_sum4(v, sred, [](double x) { return wave_sum_d(x); }); };
    if (tid < T) sf[tid] = (double)a.cf[tid];
    if (tid == 0) sbad = 0;
    double r0[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll 2
    for (int i = tid; i < a.ngh; i += nt) r0[0] += a.ellpart[i];
    block_sum4(r0);                                       // (its barriers publish sf and sbad)
    const double ell = r0[0], tau_x = a.xs[0], ld_k = a.xs[1], ld_sx = -2.0 * a.xs[2];
    task_build_kt(sC, sf, a.raw_var, T);
    task_colsum<4>(a.colpart, a.ngh, T, sgrp, scol);
    task_chol_inverse(sC, sI, spiv, &sbad, T);
    double r1[4] = {0.0, 0.0, 0.0, 0.0};
    task_inverse_and_u(sC, sI, sK, sA, spiv, a.Lt, T, r1, [&](int e, int, int, double v) { a.kti[e] = v; });
    block_sum4(r1);
    const double tau_t = r1[0], ld_kt = r1[1], ld_st = r1[2];
    task_grad_lt(sC, sA, scol, tau_x, N, a.we, a.wk, a.grad_Lt, T);
    // sC <- G (chunks by groups, groups in order);  tr(K_t^-1 G2);  quad = tr(K_t^-1 G);  colsum A = D_0 / q_0
    const int Gn = TT >= nt ? 1 : nt / TT;
    if (Gn > 1 && tid < Gn * TT) {
        const int g = tid / TT, e = tid - g * TT;
        double ra = 0.0, aa = 0.0;
#pragma unroll 2
        for (int cc = g; cc < a.nch; cc += Gn) {
            ra += a.gpart[(int64_t)cc * 2 * TT + e];
            aa += a.gpart[(int64_t)cc * 2 * TT + TT + e];
        }
        sgrp[tid] = ra;
        sgrp2[tid] = aa;
    }
    __syncthreads();                                      // (also: grad_Lt is done with sC)
    double r2[4] = {0.0, 0.0, 0.0, 0.0};
    for (int e = tid; e < TT; e += nt) {
        const int s = e / T, t = e - s * T;
        double ra = 0.0, aa = 0.0;
        if (Gn > 1) {
#pragma unroll 1
            for (int g = 0; g < Gn; ++g) {
                ra += sgrp[g * TT + e];
                aa += sgrp2[g * TT + e];
            }
        } else {
#pragma unroll 2
            for (int cc = 0; cc < a.nch; ++cc) {
                ra += a.gpart[(int64_t)cc * 2 * TT + e];
                aa += a.gpart[(int64_t)cc * 2 * TT + TT + e];
            }
        }
        sC[s * MLD + t] = ra;
        r2[0] += aa * sK[t * MLD + s];
        r2[1] += ra * sK[t * MLD + s];
    }
    if (tid < T) {
        scs[tid] = ((double)a.M[tid] - (double)a.c[tid]) / a.xs[5];
    }
    block_sum4(r2);                                       // (its barriers publish sC and scs)
    const double tr_g2 = r2[0], q = r2[1];
    task_push_through(sC, sI, sK, sA, sf, scs, tau_x, N, a.wk, a.raw_var, a.grad_cf, a.grad_rv, a.grad_c, T);
    if (tid == 0) {
        const double kl = 0.5 * (tau_x * tau_t + q - (double)N * T + T * ld_k + N * ld_kt - T * ld_sx - N * ld_st);
        const double F = a.we * ell - a.wk * kl;
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
        o[9] = (float)(-0.5 * a.wk * ((double)T * a.xs[3] - tau_t * a.xs[4] - tr_g2));
        o[10] = (float)F;
        o[11] = a.jitter;
        a.tsc[0] = tau_t;
        a.info[0] = (F - F == 0.0) ? 0 : 1;               // 1: F is NaN or infinite
        a.info[1] = sbad;
    }
}

// ---- back: workgroup 0 the adjoint sh of s (forward scan) with grad_rho, grad_gamma as each sh arrives; workgroups 1 ..
// grad_M over rows blk MM_MROWS .. + MM_MROWS
__global__ __launch_bounds__(MM_T) void back_kernel(const float* __restrict__ x, const float* __restrict__ vol, double jit,
                                                    const float* __restrict__ M, const float* __restrict__ c,
                                                    const float* __restrict__ gam, const double* __restrict__ ws_s,
                                                    const double* __restrict__ ws_e, const double* __restrict__ rowred,
                                                    const float* __restrict__ gm, const double* __restrict__ kti,
                                                    const double* __restrict__ tsc, double we, double wk,
                                                    float* __restrict__ grad_M, float* __restrict__ grad_rho,
                                                    float* __restrict__ grad_gam, int N, int T) {
    __shared__ double lds[2 * MM_W + 1];
    __shared__ double sk[MT_MAX * MLD], sa[MM_MROWS][MLD], sq[MM_MROWS + 1];
    const int tid = threadIdx.x;
    const int64_t n = N;
    const double v = (double)vol[0];
    if (blockIdx.x == 0) {
        const double wt = wk * tsc[0];                                 // w_kl tau_t
        affine_scan<MM_T>(
            n, lds,
            [&](int64_t i, double& a, double& b) {
                const double gp = i > 0 ? (double)gam[i - 1] : 0.0, o = 1.0 + gp;
                a = we * rowred[i] - wt * (i > 0 ? o * o : 1.0) / (2.0 * prior_inc(x, v, jit, i));
                b = gp * gp;
            },
            [&](int64_t i, double sh) {
                double t = sh;
                float gg = 0.f;
                if (i < n - 1) {
                    const double qn = prior_inc(x, v, jit, i + 1), sn = ws_s[i + 1], g = (double)gam[i];
                    gg = (float)(2.0 * g * sn * sh - wt * (1.0 + g) * sn / qn);
                    t -= wt / (2.0 * qn);
                }
                grad_gam[i] = gg;                                      // (the unused last entry: 0)
                grad_rho[i] = (float)(-2.0 * ws_e[i] * t - wk * (double)T);
            });
        return;
    }
    const int64_t r0 = (int64_t)(blockIdx.x - 1) * MM_MROWS;
    for (int e = tid; e < T * T; e += MM_T) sk[(e / T) * MLD + e % T] = kti[e];
    if (tid <= MM_MROWS) sq[tid] = r0 + tid < n ? prior_inc(x, v, jit, r0 + tid) : 1.0;
    __syncthreads();
    for (int e = tid; e < MM_MROWS * T; e += MM_T) {
        const int rr = e / T, t = e - rr * T;
        const int64_t i = r0 + rr;
        double av = 0.0;
        if (i < n) {
            const double mi = (double)M[i * T + t];
            av = (i > 0 ? mi - (double)M[(i - 1) * T + t] : mi - (double)c[t]) / sq[rr];
            if (i < n - 1) av -= ((double)M[(i + 1) * T + t] - mi) / sq[rr + 1];
        }
        sa[rr][t] = av;
    }
    __syncthreads();
    for (int e = tid; e < MM_MROWS * T; e += MM_T) {
        const int rr = e / T, t = e - rr * T;
        const int64_t i = r0 + rr;
        if (i >= n) continue;
        double acc = 0.0;
        for (int s = 0; s < T; ++s) acc = __builtin_fma(sa[rr][s], sk[s * MLD + t], acc);
        grad_M[i * T + t] = (float)(we * (double)gm[i * T + t] - wk * acc);
    }
}

struct Ws {
    double *s, *e, *xs, *rowred, *colpart, *ellpart, *gpart, *kti, *tsc;
    float *gm, *cvpart;
    int ngh, nch, ngm;
    size_t bytes;
};

static Ws carve(void* base, int N, int T, int Kc) {
    Carver c{base};
    Ws w;
    w.ngh = (N + MM_ROWS - 1) / MM_ROWS;
    w.nch = (N + MM_GCH - 1) / MM_GCH;
    w.ngm = (N + MM_MROWS - 1) / MM_MROWS;
    w.s = c.take<double>(N);                               // first: the caller reads diag P^-1 from here
    w.e = c.take<double>(N);
    w.xs = c.take<double>(8);
    w.rowred = c.take<double>(N);
    w.colpart = c.take<double>((size_t)w.ngh * T);
    w.ellpart = c.take<double>(w.ngh);
    w.gpart = c.take<double>((size_t)w.nch * 2 * T * T);
    w.kti = c.take<double>((size_t)T * T);
    w.tsc = c.take<double>(8);
    w.gm = c.take<float>((size_t)N * T);
    w.cvpart = c.take<float>(Kc > 0 ? (size_t)T * w.ngh * 3 * Kc : 0);
    w.bytes = c.off;
    return w;
}

}  // namespace mtm
}  // namespace volt

using namespace volt;

extern "C" {

size_t volt_gpcv_mt_markov_workspace_bytes(int N, int T, int Kc) {
    if (N < 1 || T < 1 || T > MT_MAX || Kc < 0 || Kc > VOLT_GPCV_CV_K_MAX) return 0;
    return mtm::carve(nullptr, N, T, Kc).bytes;
}

int volt_gpcv_mt_markov_step_f32(const float* x, const float* vol, float jitter, const float* M, const float* c, const float* rho,
                                 const float* gamma, const float* Lt, const float* covar_factor, const float* raw_var,
                                 const float* y, const float* abc, int Kc, const float* gh_x, const float* gh_w, int Q,
                                 float min_var, float min_scale, float w_ell, float w_kl, float* out, float* grad_M,
                                 float* grad_c, float* grad_rho, float* grad_gamma, float* grad_Lt, float* grad_covar_factor,
                                 float* grad_raw_var, float* grad_abc, int* info, void* workspace, int N, int T, void* stream) {
    if (!x) return -1;
    if (!vol) return -2;
    if (!M) return -4;
    if (!c) return -5;
    if (!rho) return -6;
    if (!gamma) return -7;
    if (!Lt) return -8;
    if (!covar_factor) return -9;
    if (!raw_var) return -10;
    if (!y) return -11;
    if (abc ? (Kc < 1 || Kc > VOLT_GPCV_CV_K_MAX) : Kc != 0) return -13;
    if (!gh_x) return -14;
    if (!gh_w) return -15;
    if (Q < 1 || Q > 1024) return -16;
    if (!out) return -21;
    if (!grad_M) return -22;
    if (!grad_c) return -23;
    if (!grad_rho) return -24;
    if (!grad_gamma) return -25;
    if (!grad_Lt) return -26;
    if (!grad_covar_factor) return -27;
    if (!grad_raw_var) return -28;
    if (abc && !grad_abc) return -29;
    if (!info) return -30;
    if (!workspace || ((uintptr_t)workspace & 255)) return -31;
    if (N < 1) return -32;
    if (T < 1 || T > MT_MAX) return -33;
    hipStream_t s = (hipStream_t)stream;
    const mtm::Ws w = mtm::carve(workspace, N, T, Kc);
    const double jit = (double)jitter, we = (double)w_ell, wk = (double)w_kl;
    hipLaunchKernelGGL(mtm::front_kernel, dim3(1 + w.nch), dim3(mtm::MM_T), 0, s, x, vol, jit, M, c, rho, gamma, w.s, w.e, w.xs,
                       w.gpart, N, T);
#define VOLT_MTM_ROWS(KC)                                                                                                     \
    case KC:                                                                                                                  \
        hipLaunchKernelGGL(mtm::rows_kernel<KC>, dim3(w.ngh), dim3(mtm::MM_T), 0, s, M, Lt, y, w.s, abc, gh_x, gh_w, Q, min_var, \
                           min_scale, w.gm, w.rowred, w.colpart, w.ellpart, w.cvpart, N, T);                                  \
        break;
    switch (Kc) {
        VOLT_MTM_ROWS(0)
        VOLT_MTM_ROWS(1)
        VOLT_MTM_ROWS(2)
        VOLT_MTM_ROWS(3)
        VOLT_MTM_ROWS(4)
        VOLT_MTM_ROWS(5)
        VOLT_MTM_ROWS(6)
        VOLT_MTM_ROWS(7)
        VOLT_MTM_ROWS(8)
    }
#undef VOLT_MTM_ROWS
    VOLT_LAUNCH_CHECK();
    if (abc) {
        const int rc = launch_cv_abc_reduce(w.cvpart, w.ngh, 3 * Kc, w_ell, grad_abc, T, s);
        if (rc) return rc;
    }
    mtm::TaskArgs ta{covar_factor, raw_var, Lt, M, c, w.gpart, w.colpart, w.ellpart, w.xs, out, grad_c, grad_Lt,
                     grad_covar_factor, grad_raw_var, w.kti, w.tsc, info, w.nch, w.ngh, N, T, jitter, we, wk};
    hipLaunchKernelGGL(mtm::task_kernel, dim3(1), dim3(TASK_NT), 0, s, ta);
    hipLaunchKernelGGL(mtm::back_kernel, dim3(1 + w.ngm), dim3(mtm::MM_T), 0, s, x, vol, jit, M, c, gamma, w.s, w.e, w.rowred, w.gm,
                       w.kti, w.tsc, we, wk, grad_M, grad_rho, grad_gamma, N, T);
    VOLT_LAUNCH_CHECK();
    return 0;
}

}  // extern "C"
