// GPCV ELBO + gradient step in O(N) for the Brownian-motion prior with a Markov variational family
// (SingleTaskVariationalGP(prior_solver="markov")).
//
// Prior: f - mu is Brownian motion started from an N(0, j) level, K_M = v min(x, x') + j 1 1' -- independent increments of
// variance q_0 = v x_0 + j, q_i = v (x_i - x_{i-1}), so K_M^-1 is exactly tridiagonal (this is NOT the dense steps' K + j I).
// Family: q = N(m, P^-1), P = Lp Lp', Lp lower bidiagonal with diagonal exp(rho_i) and (i+1, i) entry gamma_i exp(rho_i).
// Everything the step needs is an AFFINE recurrence t_p = a_p + b_p t_{p-1} -- there is no pivot chain:
//     s_i   = e^{-2 rho_i} + gamma_i^2 s_{i+1}              diag P^-1, backward, positive terms only
//     sh_i  = h_i + gamma_{i-1}^2 sh_{i-1}                  its adjoint, forward
//     u_i   = eps_i e^{-rho_i} - gamma_i u_{i+1}            a draw m + Lp^-T eps, backward
// so all three run through ONE device primitive, affine_scan (markov_scan.h, shared with gpcv_mt_markov.hip and
// markov_predict.hip): the maps (a, b): t -> a + b t compose associatively; a thread composes a contiguous run of 4 of them, a
// wave combines its 64 runs with cross-lane shuffles (six steps), the workgroup combines its waves through LDS in wave order,
// and chunks of MK_T * 4 points carry into each other in order.  The order of every operation depends on N alone: no atomics,
// bitwise repeatable.  fp64 throughout, I/O fp32.
// No rescaling of the coefficient products is needed: every term is positive in the s recurrence, so a product of the
// b = gamma^2 can only overflow where s_i >= prod b * s_N, the true variance, overflows too (info then reports F not finite).
//
// gpcv_markov_step_kernel<KC>: ONE launch per step, one workgroup per series:
//     scan back (s -> workspace)  ->  rows (a wave per point, lanes over the quadrature nodes: the node formulas of gpcv.hip's
//     gh_ell_kernel / gh_cv_ell_kernel with the variance read from s instead of summed from a row of Lq)  ->  scan forward
//     (sh), with the gradients and the scalars' partial sums formed at each point as its sh arrives  ->  fixed-order sums.
// The "cv" node is gpcv_shared.h's cv_node, the one the multi-task steps call.  The "exp" node loop is written out here: through
// gpcv_shared.h's exp_node the compiler fuses the three accumulations of this kernel differently (other bits).
#include "common.h"
#include "host.h"
#include "gpcv_shared.h"
#include "markov_scan.h"
#include "../../include/volt_hip.h"

namespace volt {

constexpr int MK_T = MARKOV_VAR_T;         // threads of the step's workgroup (8 waves)
constexpr int MK_W = MK_T / 64;
constexpr int MK_DT = 256;                 // threads of the draw's workgroup

template <int KC>
__global__ __launch_bounds__(MK_T) void gpcv_markov_step_kernel(
    const float* __restrict__ x, const float* __restrict__ vol, double jit, const float* __restrict__ resid,
    const float* __restrict__ m, const float* __restrict__ rho, const float* __restrict__ gam, const float* __restrict__ y,
    const float* __restrict__ abc, const float* __restrict__ ghx, const float* __restrict__ ghw, int Q, float min_var,
    float min_scale, double we, double wk, float* __restrict__ out, float* __restrict__ grad_m, float* __restrict__ grad_mu,
    float* __restrict__ grad_rho, float* __restrict__ grad_gam, float* __restrict__ grad_abc, int* __restrict__ info,
    double* __restrict__ ws_s, double* __restrict__ ws_e, float* __restrict__ ws_g, int N) {
    constexpr int KA = KC > 0 ? KC : 1;
    __shared__ double lds[2 * MK_W + 1];
    __shared__ double cvred[MK_W][3 * KA];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);   // (scalar: the loops over waves are scalar loops)
    const int64_t n = N, b = blockIdx.x;
    const float *rb = rho + b * n, *gb = gam + b * n, *mb = m + b * n, *yb = y + b * n, *db = resid + b * n;
    double *sb = ws_s + b * n, *eb = ws_e + b * n;                   // diag P^-1, e^{-2 rho}
    float* gvb = ws_g + b * 2 * n;                                     // dE/dvar_i
    float* gmb = gvb + n;                                              // dE/dm_i
    park_in_vgpr(grad_m), park_in_vgpr(grad_mu), park_in_vgpr(grad_rho), park_in_vgpr(grad_gam), park_in_vgpr(grad_abc);
    park_in_vgpr(out), park_in_vgpr(info), park_in_vgpr(gmb), park_in_vgpr(eb), park_in_vgpr(db), park_in_vgpr(x);
    const double v = (double)vol[b];

    // ---- 1. s = diag P^-1; the two log-determinants
    double ldk = 0.0, srho = 0.0;
    for (int64_t i = tid; i < n; i += MK_T) {
        ldk += log(prior_inc(x, v, jit, i));
        srho += (double)rb[i];
    }
    markov_var_scan<MK_T, true>(rb, gb, sb, eb, n, lds);
    __syncthreads();

    // ---- 2. the likelihood rows: wave w takes points w, w + MK_W, ..
    float pa[KA], pb[KA], pc[KA];
    double GA[KA], GB[KA], GC[KA];
#pragma unroll
    for (int k = 0; k < KA; ++k) {
        pa[k] = pb[k] = pc[k] = 0.f;
        if (KC > 0) {
            pa[k] = abc[(b * 3 + 0) * KC + k];
            pb[k] = abc[(b * 3 + 1) * KC + k];
            pc[k] = abc[(b * 3 + 2) * KC + k];
        }
        GA[k] = GB[k] = GC[k] = 0.0;
    }
    double ell = 0.0;
    for (int64_t i = wave; i < n; i += MK_W) {
        float var = (float)sb[i];
        const bool floored = var < min_var;
        if (floored) var = min_var;
        const float mi = mb[i], yi = yb[i];
        const float sd2 = sqrtf(2.f * var);
        float e = 0.f, gm = 0.f, gv = 0.f;
        if (KC == 0) {
            for (int k = lane; k < Q; k += 64) {
                const float xk = ghx[k], wq = ghw[k];
                const float f = mi + sd2 * xk;
                const float ef = expf(f);
                const bool live = ef > min_scale;
                const float sc = live ? ef : min_scale;
                const float r = yi / sc;
                const float logp = -0.5f * r * r - (live ? f : logf(min_scale)) - 0.91893853320467274f;
                const float g = live ? (r * r - 1.f) : 0.f;
                e += wq * logp;
                gm += wq * g;
                gv += wq * g * xk;
            }
        } else {
            float ga[KA], gbb[KA], gc[KA];
#pragma unroll
            for (int k = 0; k < KA; ++k) ga[k] = gbb[k] = gc[k] = 0.f;
            for (int q = lane; q < Q; q += 64) {
                const float xq = ghx[q];
                cv_node<KA>(mi + sd2 * xq, xq, ghw[q], yi, min_scale, pa, pb, pc, ga, gbb, gc, e, gm, gv);
            }
#pragma unroll
            for (int k = 0; k < KA; ++k) {                             // per lane, point after point, in fp64
                GA[k] += (double)ga[k];
                GB[k] += (double)gbb[k];
                GC[k] += (double)gc[k];
            }
        }
        e = wave_sum_f(e);
        gm = wave_sum_f(gm);
        gv = wave_sum_f(gv);
        ell += (double)e;
        if (lane == 0) {
            gmb[i] = gm;
            gvb[i] = floored ? 0.f : gv / sd2;                         // df/dvar = x_k / sqrt(2 var);  floored: dE/dvar = 0
        }
    }
    if (KC > 0) {
#pragma unroll
        for (int k = 0; k < KA; ++k) {
            const double ra = wave_sum_d(GA[k]), rbb = wave_sum_d(GB[k]), rc = wave_sum_d(GC[k]);
            if (lane == 0) {
                cvred[wave][k] = ra;
                cvred[wave][KA + k] = rbb;
                cvred[wave][2 * KA + k] = rc;
            }
        }
    }
    if (lane == 0) lds[wave] = ell;
    __syncthreads();                                                   // (also: the rows' gm, gv are visible to the workgroup)
    ell = 0.0;
    for (int w = 0; w < MK_W; ++w) ell += lds[w];
    if (KC > 0 && tid < 3 * KC) {
        double r = 0.0;
        for (int w = 0; w < MK_W; ++w) r += cvred[w][tid];
        grad_abc[b * 3 * KC + tid] = (float)(we * r);
    }
    __syncthreads();

    // ---- 3. the adjoint sh (forward), the gradients and the scalars' partial sums at each point
    double tr = 0.0, quad = 0.0, dv = 0.0;
    affine_scan<MK_T>(
        n, lds,
        [&](int64_t i, double& a, double& bb) {
            const double gp = i > 0 ? (double)gb[i - 1] : 0.0, o = 1.0 + gp;
            a = we * (double)gvb[i] - wk * (i > 0 ? o * o : 1.0) / (2.0 * prior_inc(x, v, jit, i));
            bb = gp * gp;
        },
        [&](int64_t i, double sh) {
            const bool last = i == n - 1;
            const double q = prior_inc(x, v, jit, i), si = sb[i];
            const double d = (double)db[i], dp = i > 0 ? (double)db[i - 1] : 0.0, dd = d - dp;
            double e = si, kd = dd / q, t = sh;
            if (i > 0) {
                const double o = 1.0 + (double)gb[i - 1];
                e = eb[i - 1] + o * o * si;                            // Var_q(f_i - f_{i-1}): no cancellation in this form
            }
            float gg = 0.f;
            if (!last) {
                const double qn = prior_inc(x, v, jit, i + 1), sn = sb[i + 1], g = (double)gb[i];
                gg = (float)(2.0 * g * sn * sh - wk * (1.0 + g) * sn / qn);
                t -= wk / (2.0 * qn);
                kd -= ((double)db[i + 1] - d) / qn;
            }
            grad_gam[b * n + i] = gg;                                  // (the unused last entry: 0)
            grad_rho[b * n + i] = (float)(-2.0 * eb[i] * t - wk);
            grad_m[b * n + i] = (float)(we * (double)gmb[i] - wk * kd);
            grad_mu[b * n + i] = (float)(wk * kd);
            const double del = grid_step(x, i);
            tr += e / q;
            quad += dd * dd / q;
            dv += del * (1.0 / q - (e + dd * dd) / (q * q));
        });

    // ---- 4. the scalars
    tr = block_sum_d<MK_T>(tr, lds);
    quad = block_sum_d<MK_T>(quad, lds);
    ldk = block_sum_d<MK_T>(ldk, lds);
    srho = block_sum_d<MK_T>(srho, lds);
    dv = block_sum_d<MK_T>(dv, lds);
    if (tid == 0) {
        const double lds_ = -2.0 * srho;
        const double kl = 0.5 * (tr + quad - (double)n + ldk - lds_);
        const double F = we * ell - wk * kl;
        float* o = out + b * 12;
        o[0] = (float)ell;
        o[1] = (float)kl;
        o[2] = (float)quad;
        o[3] = (float)ldk;
        o[4] = (float)lds_;
        o[5] = (float)tr;
        o[6] = (float)(-0.5 * wk * dv);
        o[7] = 0.f;
        o[8] = 0.f;
        o[9] = (float)F;
        o[10] = (float)jit;
        o[11] = 0.f;
        info[b] = (F - F == 0.0) ? 0 : 1;                              // 1: F is NaN or infinite
    }
}

// out[b, r, :] = m[b] + Lp[b]^-T eps[b, r, :]: one workgroup per draw
__global__ __launch_bounds__(MK_DT) void markov_root_draw_kernel(const float* __restrict__ m, const float* __restrict__ rho,
                                                                 const float* __restrict__ gam, const float* __restrict__ eps,
                                                                 float* __restrict__ out, int reps, int N) {
    __shared__ double lds[2 * (MK_DT / 64) + 1];
    const int64_t n = N, g = blockIdx.x, b = g / reps;
    const float *rb = rho + b * n, *gb = gam + b * n, *mb = m + b * n, *eb = eps + g * n;
    float* ob = out + g * n;
    affine_scan<MK_DT>(
        n, lds,
        [&](int64_t p, double& a, double& bb) {
            const int64_t i = n - 1 - p;
            a = (double)eb[i] * exp(-(double)rb[i]);
            bb = p > 0 ? -(double)gb[i] : 0.0;
        },
        [&](int64_t p, double u) {
            const int64_t i = n - 1 - p;
            ob[i] = (float)((double)mb[i] + u);
        });
}

// (the step's workgroup size: the same scan in the same order, so var equals the step's s bit for bit)
__global__ __launch_bounds__(MK_T) void markov_root_var_kernel(const float* __restrict__ rho, const float* __restrict__ gam,
                                                               double* __restrict__ var, int N) {
    __shared__ double lds[2 * MK_W + 1];
    const int64_t n = N, b = blockIdx.x;
    markov_var_scan<MK_T, true>(rho + b * n, gam + b * n, var + b * n, nullptr, n, lds);
}

struct GpcvMarkovWs {
    double *s, *e;                         // [B,N] diag P^-1;  [B,N] e^{-2 rho}
    float* g;                              // [B,2,N] the rows' dE/dvar, dE/dm
    size_t bytes;
};

static GpcvMarkovWs carve_gpcv_markov(void* base, int B, int N) {
    Carver c{base};
    GpcvMarkovWs w;
    w.s = c.take<double>((size_t)B * N);
    w.e = c.take<double>((size_t)B * N);
    w.g = c.take<float>((size_t)B * N * 2);
    w.bytes = c.off;
    return w;
}

}  // namespace volt

using namespace volt;

extern "C" {

size_t volt_gpcv_markov_workspace_bytes(int B, int N, int Kc) {
    if (B < 1 || N < 1 || Kc < 0 || Kc > VOLT_GPCV_CV_K_MAX) return 0;
    return carve_gpcv_markov(nullptr, B, N).bytes;
}

int volt_gpcv_markov_step_f32(const float* x, const float* vol, float jitter, const float* resid, const float* m, const float* rho,
                              const float* gamma, const float* y, const float* abc, int Kc, const float* gh_x, const float* gh_w,
                              int Q, float min_var, float min_scale, float w_ell, float w_kl, float* out, float* grad_m,
                              float* grad_mu, float* grad_rho, float* grad_gamma, float* grad_abc, int* info, void* workspace,
                              int B, int N, void* stream) {
    if (!x) return -1;
    if (!vol) return -2;
    if (!resid) return -4;
    if (!m) return -5;
    if (!rho) return -6;
    if (!gamma) return -7;
    if (!y) return -8;
    if (abc ? (Kc < 1 || Kc > VOLT_GPCV_CV_K_MAX) : Kc != 0) return -10;
    if (!gh_x) return -11;
    if (!gh_w) return -12;
    if (Q < 1 || Q > 1024) return -13;
    if (!out) return -18;
    if (!grad_m) return -19;
    if (!grad_mu) return -20;
    if (!grad_rho) return -21;
    if (!grad_gamma) return -22;
    if (abc && !grad_abc) return -23;
    if (!info) return -24;
    if (!workspace || ((uintptr_t)workspace & 255)) return -25;
    if (B < 1 || B > 65535) return -26;
    if (N < 1) return -27;
    hipStream_t s = (hipStream_t)stream;
    const GpcvMarkovWs w = carve_gpcv_markov(workspace, B, N);
#define VOLT_MARKOV_STEP(KC)                                                                                                  \
    case KC:                                                                                                                  \
        hipLaunchKernelGGL(gpcv_markov_step_kernel<KC>, dim3(B), dim3(MK_T), 0, s, x, vol, (double)jitter, resid, m, rho,     \
                           gamma, y, abc, gh_x, gh_w, Q, min_var, min_scale, (double)w_ell, (double)w_kl, out, grad_m,        \
                           grad_mu, grad_rho, grad_gamma, grad_abc, info, w.s, w.e, w.g, N);                                    \
        break;
    switch (Kc) {
        VOLT_MARKOV_STEP(0)
        VOLT_MARKOV_STEP(1)
        VOLT_MARKOV_STEP(2)
        VOLT_MARKOV_STEP(3)
        VOLT_MARKOV_STEP(4)
        VOLT_MARKOV_STEP(5)
        VOLT_MARKOV_STEP(6)
        VOLT_MARKOV_STEP(7)
        VOLT_MARKOV_STEP(8)
    }
#undef VOLT_MARKOV_STEP
    VOLT_LAUNCH_CHECK();
    return 0;
}

int volt_markov_root_draw_f32(const float* m, const float* rho, const float* gamma, const float* eps, float* out, int B, int reps,
                              int N, void* stream) {
    if (!m) return -1;
    if (!rho) return -2;
    if (!gamma) return -3;
    if (!eps) return -4;
    if (!out) return -5;
    if (B < 1) return -6;
    if (reps < 1 || (int64_t)B * reps >= (1LL << 24)) return -7;     // (a launch holds fewer than 2^32 threads)
    if (N < 1) return -8;
    hipLaunchKernelGGL(markov_root_draw_kernel, dim3((unsigned)((int64_t)B * reps)), dim3(MK_DT), 0, (hipStream_t)stream, m, rho,
                       gamma, eps, out, reps, N);
    VOLT_LAUNCH_CHECK();
    return 0;
}

int volt_markov_root_var_f32(const float* rho, const float* gamma, double* var, int B, int N, void* stream) {
    if (!rho) return -1;
    if (!gamma) return -2;
    if (!var) return -3;
    if (B < 1) return -4;
    if (N < 1) return -5;
    hipLaunchKernelGGL(markov_root_var_kernel, dim3(B), dim3(MK_T), 0, (hipStream_t)stream, rho, gamma, var, N);
    VOLT_LAUNCH_CHECK();
    return 0;
}

}  // extern "C"
