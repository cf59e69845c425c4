// Natural-gradient (conjugate-computation VI) update of the Markov variational family: the fit of
// SingleTaskVariationalGP(prior_solver="markov") as a fixed-point iteration on N pairs of site numbers instead of a first-order
// descent on (m, rho, gamma).
//
// Under the level-jitter Brownian prior K_M (gpcv_markov.hip's header) and a likelihood that factorises over points, the
// optimal Gaussian has precision K_M^-1 + diag(lambda_2) and mean mu + P^-1 lambda_1.  With r = w_ell / w_kl, d = m - mu,
// gm_i = dE_i/dm_i, gv_i = dE_i/ds_i at the current q:
//     t2_i = max(-2 r gv_i, 0)          t1_i = r gm_i + t2_i d_i              the sites the current q asks for
//     lam <- (1 - beta) lam + beta t                                          damped
//     P = K_M^-1 + diag(lam2):  A_i = 1/q_i + 1/q_{i+1} + lam2_i,  o_i = -1/q_{i+1}
//     d_0 = A_0,  gamma_i = o_i / d_i,  d_{i+1} = A_{i+1} - o_i gamma_i,  rho_i = log(d_i) / 2        P = Lp Lp'
//     t_0 = lam1_0,  t_i = lam1_i - gamma_{i-1} t_{i-1};   delta_{N-1} = t_{N-1} / d_{N-1},
//     delta_i = t_i / d_i - gamma_i delta_{i+1};   m = mu + delta                                     P delta = lam1
// Every pivot is positive (K_M^-1 is positive definite, lam2 >= 0): only a non-finite input fails.
//
// gpcv_markov_ng_kernel<KC>: ONE launch per update, one workgroup of MARKOV_VAR_T threads per series, five phases with
// barriers between them:
//     1. s = diag P^-1 by markov_var_scan at the step's workgroup size: the step's s bit for bit
//     2. rows (a wave per point, lanes over the nodes: the node formulas of gpcv_markov_step_kernel), then lane 0 forms the
//        targets, blends the sites in place and leaves A_i, o_i, lam1_i in the workspace
//     3. the pivot chain, the one serial part: chunks of NG_CH points are staged in LDS by the workgroup, ONE lane walks
//        them (d_{i+1} = A_{i+1} - o_i^2 / d_i: one FMA and one reciprocal per point on the chain, the forward sweep t beside
//        it) and leaves 1/d_i, gamma_i, t_i in place, the workgroup stores them
//     4. the backward sweep through affine_scan (a = t_i / d_i, b = -gamma_i); each point's new m, rho, gamma are written as
//        its delta arrives, by the thread that has just read the old ones: outputs may alias inputs
//     5. fixed-order block reductions: clamped sites, max |change| of m, rho, gamma, failures
// fp64 for every recurrence; fp32 for the quadrature and the parameter I/O; sites fp64.  No atomics, bitwise repeatable,
// no LDS sized by N.
#include "common.h"
#include "host.h"
#include "chain.h"
#include "gpcv_shared.h"
#include "markov_scan.h"
#include "../../include/volt_hip.h"

namespace volt {

constexpr int NG_T = MARKOV_VAR_T;         // the step's workgroup size (the scan's order and so s depend on it)
constexpr int NG_W = NG_T / 64;
constexpr int NG_CH = 1024;                // points per staged chunk of the pivot chain (3 x 8 KB of LDS)
constexpr int NG_U = 4;                    // points the chain's lane loads ahead of its arithmetic

__device__ __forceinline__ bool finite_d(double v) { return v - v == 0.0; }

template <int KC>
__global__ __launch_bounds__(NG_T) void gpcv_markov_ng_kernel(
    const float* __restrict__ x, const float* __restrict__ vol, double jit, const float* __restrict__ mu, const float* m,
    const float* rho, const float* gam, const float* __restrict__ y, const float* __restrict__ abc,
    const float* __restrict__ ghx, const float* __restrict__ ghw, int Q, float min_var, float min_scale, double r, double beta,
    double* __restrict__ lam1, double* __restrict__ lam2, float* m_out, float* rho_out, float* gam_out,
    double* __restrict__ out, int* __restrict__ info, double* __restrict__ ws_s, double* __restrict__ ws_a,
    double* __restrict__ ws_o, double* __restrict__ ws_l, int N) {
    constexpr int KA = KC > 0 ? KC : 1;
    __shared__ double lds[2 * NG_W + 1];
    __shared__ double sA[NG_CH], sO[NG_CH], sL[NG_CH];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int64_t n = N, b = blockIdx.x;
    const float *rb = rho + b * n, *gb = gam + b * n, *mb = m + b * n, *yb = y + b * n, *ub = mu + b * n;
    float *mo = m_out + b * n, *ro = rho_out + b * n, *go = gam_out + b * n;
    double *sb = ws_s + b * n, *ab = ws_a + b * n, *ob = ws_o + b * n, *lb = ws_l + b * n;
    double *l1 = lam1 + b * n, *l2 = lam2 + b * n;
    // (the "cv" parameters are 3 KC scalars: what the quadrature loop does not read waits in vector registers)
    park_in_vgpr(mo), park_in_vgpr(ro), park_in_vgpr(go), park_in_vgpr(out), park_in_vgpr(info), park_in_vgpr(ab), park_in_vgpr(ob);
    park_in_vgpr(lb), park_in_vgpr(l1), park_in_vgpr(l2), park_in_vgpr(ub), park_in_vgpr(x);
    const double v = (double)vol[b];

    // ---- 1. s = diag P^-1 of the current q
    markov_var_scan<NG_T, true>(rb, gb, sb, nullptr, n, lds);
    __syncthreads();

    // ---- 2. rows, targets, blended sites; A, o, lam1 into the workspace.  Wave w takes points w, w + NG_W, ..
    float pa[KA], pb[KA], pc[KA];
#pragma unroll
    for (int k = 0; k < KA; ++k) {
        pa[k] = pb[k] = pc[k] = 0.f;
        if (KC > 0) {
            pa[k] = abc[(b * 3 + 0) * KC + k];
            pb[k] = abc[(b * 3 + 1) * KC + k];
            pc[k] = abc[(b * 3 + 2) * KC + k];
        }
    }
    const double omb = 1.0 - beta;
    double nclamp = 0.0, bad = 0.0;                                     // (lane 0's; counts as doubles: one kind of reduction)
    for (int64_t i = wave; i < n; i += NG_W) {
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
                const float rr = yi / sc;
                const float g = live ? (rr * rr - 1.f) : 0.f;
                gm += wq * g;
                gv += wq * g * xk;
            }
        } else {
            float ga[KA], gbb[KA], gc[KA];                              // (the parameter sums are not needed here: dead code)
#pragma unroll
            for (int k = 0; k < KA; ++k) ga[k] = gbb[k] = gc[k] = 0.f;
            for (int q = lane; q < Q; q += 64) {
                const float xq = ghx[q];
                cv_node<KA>(mi + sd2 * xq, xq, ghw[q], yi, min_scale, pa, pb, pc, ga, gbb, gc, e, gm, gv);
            }
        }
        gm = wave_sum_f(gm);
        gv = wave_sum_f(gv);
        if (lane == 0) {
            const double gvd = floored ? 0.0 : (double)(gv / sd2);     // df/dvar = x_k / sqrt(2 var);  floored: dE/dvar = 0
            const double dm = (double)mi - (double)ub[i];
            const bool clamp = gvd > 0.0;
            const double t2 = clamp ? 0.0 : -2.0 * r * gvd;
            const double t1 = __builtin_fma(t2, dm, r * (double)gm);
            const double n2 = omb * l2[i] + beta * t2;
            const double n1 = omb * l1[i] + beta * t1;
            l2[i] = n2;
            l1[i] = n1;
            const double iq = 1.0 / prior_inc(x, v, jit, i);
            const double iqn = i + 1 < n ? 1.0 / prior_inc(x, v, jit, i + 1) : 0.0;
            ab[i] = iq + iqn + n2;
            ob[i] = -iqn;
            lb[i] = n1;
            nclamp += clamp ? 1.0 : 0.0;
            bad += finite_d(n1) && finite_d(n2) ? 0.0 : 1.0;
        }
    }
    __syncthreads();                                                   // A, o, lam1 are visible to the workgroup

    // ---- 3. the pivot chain with the forward sweep folded in: 1/d -> ws_a, gamma -> ws_o, t -> ws_l
    double inv_p = 0.0, oo_p = 0.0, g_p = 0.0, t_p = 0.0;              // thread 0's carry: 1/d_{i-1}, o_{i-1}^2, gamma_{i-1}, t_{i-1}
    for (int64_t c0 = 0; c0 < n; c0 += NG_CH) {
        for (int j = tid; j < NG_CH; j += NG_T) {
            const bool in = c0 + j < n;                                 // (past the end: A = 1, o = 0, lam1 = 0 -- a pivot of 1)
            sA[j] = in ? ab[c0 + j] : 1.0;
            sO[j] = in ? ob[c0 + j] : 0.0;
            sL[j] = in ? lb[c0 + j] : 0.0;
        }
        __syncthreads();
        if (tid == 0) {
            const int cnt = (int)(n - c0 < NG_CH ? n - c0 : NG_CH);
            double a[NG_U], o[NG_U], l[NG_U];
#pragma unroll
            for (int u = 0; u < NG_U; ++u) a[u] = sA[u], o[u] = sO[u], l[u] = sL[u];
            for (int j0 = 0; j0 < cnt; j0 += NG_U) {
                double an[NG_U], on[NG_U], ln[NG_U];
                const int jn = j0 + NG_U < NG_CH ? j0 + NG_U : j0;      // the next group's loads are under way during this one's chain
#pragma unroll
                for (int u = 0; u < NG_U; ++u) an[u] = sA[jn + u], on[u] = sO[jn + u], ln[u] = sL[jn + u];
#pragma unroll
                for (int u = 0; u < NG_U; ++u) {
                    const double d = __builtin_fma(-oo_p, inv_p, a[u]);
                    const double inv = chain_rcp(d);
                    const double t = __builtin_fma(-g_p, t_p, l[u]);
                    const double g = o[u] * inv;
                    bad += chain_pivot_ok(d) ? 0.0 : 1.0;
                    sA[j0 + u] = inv;
                    sO[j0 + u] = g;
                    sL[j0 + u] = t;
                    inv_p = inv, oo_p = o[u] * o[u], g_p = g, t_p = t;
                }
#pragma unroll
                for (int u = 0; u < NG_U; ++u) a[u] = an[u], o[u] = on[u], l[u] = ln[u];
            }
        }
        __syncthreads();
        for (int j = tid; j < NG_CH; j += NG_T) {
            if (c0 + j < n) {
                ab[c0 + j] = sA[j];
                ob[c0 + j] = sO[j];
                lb[c0 + j] = sL[j];
            }
        }
        __syncthreads();
    }

    // ---- 4. the backward sweep; the new parameters and their distance from the old ones, point by point
    double dm_max = 0.0, dr_max = 0.0, dg_max = 0.0;
    affine_scan<NG_T>(
        n, lds,
        [&](int64_t p, double& a, double& bb) {
            const int64_t i = n - 1 - p;
            a = lb[i] * ab[i];
            bb = p > 0 ? -ob[i] : 0.0;
        },
        [&](int64_t p, double delta) {
            const int64_t i = n - 1 - p;
            const bool last = p == 0;
            const float mold = mb[i], rold = rb[i], gold = last ? 0.f : gb[i];      // (gamma_{N-1} is never read)
            const float mnew = (float)((double)ub[i] + delta);
            const float rnew = (float)(-0.5 * log(ab[i]));
            const float gnew = last ? 0.f : (float)ob[i];
            mo[i] = mnew;
            ro[i] = rnew;
            go[i] = gnew;
            dm_max = fmax(dm_max, fabs((double)mnew - (double)mold));
            dr_max = fmax(dr_max, fabs((double)rnew - (double)rold));
            dg_max = fmax(dg_max, fabs((double)gnew - (double)gold));
            bad += finite_d((double)mnew) && finite_d((double)rnew) && finite_d((double)gnew) ? 0.0 : 1.0;
        });

    // ---- 5. the diagnostics
    nclamp = block_sum_d<NG_T>(nclamp, lds);
    bad = block_sum_d<NG_T>(bad, lds);
    double mx[3] = {dm_max, dr_max, dg_max};
#pragma unroll
    for (int k = 0; k < 3; ++k) {
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) mx[k] = fmax(mx[k], __shfl_xor(mx[k], d, 64));
        if (lane == 0) lds[wave] = mx[k];
        __syncthreads();
        double t = 0.0;
        for (int w = 0; w < NG_W; ++w) t = fmax(t, lds[w]);
        mx[k] = t;
        __syncthreads();
    }
    const bool failed = bad != 0.0;
    if (failed) {                                                      // (workgroup-uniform) nothing of this series survives
        const double qn = __builtin_nan("");
        const float fn = __builtin_nanf("");
        for (int64_t i = tid; i < n; i += NG_T) {
            mo[i] = fn, ro[i] = fn, go[i] = fn;
            l1[i] = qn, l2[i] = qn;
        }
    }
    if (tid == 0) {
        const double qn = __builtin_nan("");
        double* o = out + b * 4;
        o[0] = failed ? qn : nclamp;
        o[1] = failed ? qn : mx[0];
        o[2] = failed ? qn : mx[1];
        o[3] = failed ? qn : mx[2];
        info[b] = failed ? 1 : 0;
    }
}

struct GpcvMarkovNgWs {
    double *s, *a, *o, *l;                 // [B,N] each: diag P^-1;  A -> 1/d;  o -> gamma;  lam1 -> t
    size_t bytes;
};

static GpcvMarkovNgWs carve_gpcv_markov_ng(void* base, int B, int N) {
    Carver c{base};
    GpcvMarkovNgWs w;
    w.s = c.take<double>((size_t)B * N);
    w.a = c.take<double>((size_t)B * N);
    w.o = c.take<double>((size_t)B * N);
    w.l = c.take<double>((size_t)B * N);
    w.bytes = c.off;
    return w;
}

}  // namespace volt

using namespace volt;

extern "C" {

size_t volt_gpcv_markov_ng_workspace_bytes(int B, int N, int Kc) {
    if (B < 1 || B > 65535 || N < 1 || Kc < 0 || Kc > VOLT_GPCV_CV_K_MAX) return 0;
    return carve_gpcv_markov_ng(nullptr, B, N).bytes;
}

int volt_gpcv_markov_ng_f32(const float* x, const float* vol, float jitter, const float* mu, const float* m, const float* rho,
                            const float* gamma, const float* y, const float* abc, int Kc, const float* gh_x, const float* gh_w,
                            int Q, float min_var, float min_scale, float w_ell, float w_kl, double step, double* lam1,
                            double* lam2, float* m_out, float* rho_out, float* gamma_out, double* out, int* info,
                            void* workspace, int B, int N, void* stream) {
    if (!x) return -1;
    if (!vol) return -2;
    if (!mu) return -4;
    if (!m) return -5;
    if (!rho) return -6;
    if (!gamma) return -7;
    if (!y) return -8;
    if (abc ? (Kc < 1 || Kc > VOLT_GPCV_CV_K_MAX) : Kc != 0) return -10;
    if (!gh_x) return -11;
    if (!gh_w) return -12;
    if (Q < 1 || Q > 1024) return -13;
    if (!(w_kl > 0.f)) return -17;
    if (!(step > 0.0 && step <= 1.0)) return -18;
    if (!lam1) return -19;
    if (!lam2) return -20;
    if (!m_out) return -21;
    if (!rho_out) return -22;
    if (!gamma_out) return -23;
    if (!out) return -24;
    if (!info) return -25;
    if (!workspace || ((uintptr_t)workspace & 255)) return -26;
    if (B < 1 || B > 65535) return -27;
    if (N < 1) return -28;
    hipStream_t s = (hipStream_t)stream;
    const GpcvMarkovNgWs w = carve_gpcv_markov_ng(workspace, B, N);
    const double r = (double)w_ell / (double)w_kl;
#define VOLT_MARKOV_NG(KC)                                                                                                    \
    case KC:                                                                                                                  \
        hipLaunchKernelGGL(gpcv_markov_ng_kernel<KC>, dim3(B), dim3(NG_T), 0, s, x, vol, (double)jitter, mu, m, rho, gamma, y, \
                           abc, gh_x, gh_w, Q, min_var, min_scale, r, step, lam1, lam2, m_out, rho_out, gamma_out, out, info,  \
                           w.s, w.a, w.o, w.l, N);                                                                              \
        break;
    switch (Kc) {
        VOLT_MARKOV_NG(0)
        VOLT_MARKOV_NG(1)
        VOLT_MARKOV_NG(2)
        VOLT_MARKOV_NG(3)
        VOLT_MARKOV_NG(4)
        VOLT_MARKOV_NG(5)
        VOLT_MARKOV_NG(6)
        VOLT_MARKOV_NG(7)
        VOLT_MARKOV_NG(8)
    }
#undef VOLT_MARKOV_NG
    VOLT_LAUNCH_CHECK();
    return 0;
}

}  // extern "C"
