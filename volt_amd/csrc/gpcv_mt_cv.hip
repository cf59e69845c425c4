// Multi-task GPCV, the copula-process ("cv") likelihood with one warp per task: the N x T Gauss-Hermite pass of
// volt_gpcv_mt_cv_step_f32 (gpcv_mt.hip holds the step; everything after this pass is the "exp" step's launches).
//   reference: voltron/models/multi_task_variational_gp.py:58-69, voltron/likelihoods/volatility_likelihood.py:19-22,45-47
//     scale_t(f) = sum_k a_tk softplus(b_tk f + c_tk),  y_nt | f ~ N(0, max(scale_t(f), min_scale)),  f ~ N(M_nt, var_nt)
#include "common.h"
#include "gpcv_shared.h"
#include "../../include/volt_hip.h"
#include <math.h>

namespace volt {

// mt_gh_kernel's pass (gpcv_mt.hip) for the copula-process ("cv") warp of task t, scale(f) = sum_k a_tk softplus(b_tk f +
// c_tk) (cv_node; abc [T,3,KC]).  It writes what mt_gh_kernel writes, with the same meaning, and the parameter sums besides.
// Here a WAVE owns a task: wave w of the workgroup's CV_WAVES takes t = w, w + CV_WAVES, ..., walks the workgroup's GH_ROWS
// rows with lane q on nodes q, q + 64, .. and keeps the 3 KC parameter sums of its task in registers across the rows (KC is
// a template argument so that they stay there), so they need no LDS stage: one butterfly per sum and task, then
// cvpart[t][blockIdx.x][3 KC], which cv_abc_reduce_kernel adds up over the workgroups in a fixed order with b = t.  Rows past
// N add nothing.
// A wave's tasks and rows are a serial chain (16 rows x ceil(T / CV_WAVES) tasks x 2 trips over the nodes at Q = 75), and
// GH_ROWS is fixed by the layout of colpart / ellpart: with 4 waves the pass took 0.85 ms at T = 64 whatever N was (one
// workgroup per CU at N = 4096), so the workgroup has 8 -- 1024 threads would cap the kernel at 128 VGPRs, and KC >= 7
// needs 130 .. 148.
constexpr int CV_WAVES = 8;

template <int KC>
__global__ __launch_bounds__(CV_WAVES * 64) void mt_gh_cv_kernel(const float* __restrict__ M, const float* __restrict__ Lt,
                                                       const float* __restrict__ y, const float* __restrict__ vx,
                                                       const float* __restrict__ abc, const float* __restrict__ ghx,
                                                       const float* __restrict__ ghw, int Q, float min_var, float min_scale,
                                                       float* __restrict__ gm, float* __restrict__ rowred,
                                                       float* __restrict__ colpart, float* __restrict__ ellpart,
                                                       float* __restrict__ cvpart, int N, int T) {
    __shared__ float svt[MT_MAX], sx[GH_ROWS], sre[GH_ROWS];
    __shared__ float sgv[GH_ROWS][MLD], sel[GH_ROWS][MLD];
    const int tid = threadIdx.x, r0 = blockIdx.x * GH_ROWS;
    const int lane = tid & 63, wave = tid >> 6;
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
    for (int t = wave; t < T; t += CV_WAVES) {
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
        const float vt = svt[t];
        for (int rr = 0; rr < GH_ROWS; ++rr) {
            const int n = r0 + rr;
            float el = 0.f, g1 = 0.f, g2 = 0.f;
            if (n < N) {
                float var = sx[rr] * vt;
                const bool floored = var < min_var;
                if (floored) var = min_var;
                const float mi = M[(int64_t)n * T + t], yi = y[(int64_t)n * T + t];
                const float sd2 = sqrtf(2.f * var);
                for (int q = lane; q < Q; q += 64) {
                    const float xq = ghx[q];
                    cv_node<KC>(mi + sd2 * xq, xq, ghw[q], yi, min_scale, pa, pb, pc, ga, gb, gc, el, g1, g2);
                }
                el = wave_sum_f(el);
                g1 = wave_sum_f(g1);
                g2 = wave_sum_f(g2);
                g2 = floored ? 0.f : g2 / sd2;               // df/dvar = x_q / sqrt(2 var)
                if (lane == 0) gm[(int64_t)n * T + t] = g1;
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

// The "cv" quadrature pass for Kc warp terms + the fixed-order reduction of its parameter partials into grad_abc [T,3,Kc].
int launch_mt_cv_pass(const float* M, const float* Lt, const float* y, const float* vx, const float* abc, int Kc,
                      const float* gh_x, const float* gh_w, int Q, float min_var, float min_scale, float w_ell, float* gm,
                      float* rowred, float* colpart, float* ellpart, float* cvpart, float* grad_abc, int N, int T,
                      hipStream_t s) {
    const int ngh = (N + GH_ROWS - 1) / GH_ROWS;
#define VOLT_MT_CV(KC)                                                                                                 \
    case KC:                                                                                                           \
        hipLaunchKernelGGL(mt_gh_cv_kernel<KC>, dim3(ngh), dim3(CV_WAVES * 64), 0, s, M, Lt, y, vx, abc, gh_x, gh_w, Q,    \
                           min_var, min_scale, gm, rowred, colpart, ellpart, cvpart, N, T);                            \
        break;
    switch (Kc) {
        VOLT_MT_CV(1) VOLT_MT_CV(2) VOLT_MT_CV(3) VOLT_MT_CV(4) VOLT_MT_CV(5) VOLT_MT_CV(6) VOLT_MT_CV(7) VOLT_MT_CV(8)
    }
#undef VOLT_MT_CV
    VOLT_LAUNCH_CHECK();
    return launch_cv_abc_reduce(cvpart, ngh, 3 * Kc, w_ell, grad_abc, T, s);
}

}  // namespace volt
