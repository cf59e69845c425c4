// What the two variational steps (gpcv.hip: one series per batch entry; gpcv_mt.hip + gpcv_mt_cv.hip: T series behind ONE
// prior) share:
// the structured NT GEMM on the 128x128 MFMA core, the triangle-keeping transpose and the fixed-order reduction of the
// "cv" likelihood's parameter sums.  The kernels live in gpcv.hip; these are their host-side launchers.
#pragma once
#include "common.h"
#include "host.h"

namespace volt {

// C[b] tile (tm, tn) = alpha * A[b][tm, :] B[b][tn, :]^T + beta * C, K restricted by the operands' triangles:
// s = 0 dense, 1 lower (k-block <= row-block), 2 upper (k-block >= row-block).  sc: 0 every tile, 1 only
// tn <= tm, 2 only tn >= tm (other tiles are not touched).  frob (nullable) [B, mt*nt] receives each
// tile's sum of squares (0 for skipped tiles).  All dimensions are multiples of 128.
struct GemmArgs {
    const float *A, *B;
    float* C;
    int64_t lda, bsa, ldb, bsb, ldc, bsc;
    int mt, nt, kt, sa, sb, sc;
    float alpha, beta;
    float* frob;
};

int launch_gemm(const GemmArgs& g, int B, hipStream_t s);
// dst (Np x Np, zero padded) = transpose of the kept triangle of src (N x N, leading dim lds):
// keep = 1: src lower (col <= row), keep = 2: src upper (col >= row), 0: everything.
int launch_transpose_tri(const float* src, int64_t lds, int64_t bss, float* dst, int N, int Np, int keep, int B,
                         hipStream_t s);
// grad_abc[b][j] = we * sum_k part[b][k][j], k < nblk, j < n3 = 3 Kc (cv_abc_reduce_kernel of gpcv.hip: fp64, fixed order).
int launch_cv_abc_reduce(const float* part, int nblk, int n3, float we, float* grad_abc, int B, hipStream_t s);

// ---- the multi-task step's N x T quadrature pass: mt_gh_kernel (gpcv_mt.hip, "exp") and mt_gh_cv_kernel (gpcv_mt_cv.hip)
constexpr int MT_MAX = 64;            // largest T: the task algebra is LDS resident, the T rows fit half a 128-row tile
constexpr int MLD = MT_MAX + 1;       // LDS row stride in doubles (odd: column walks spread over the banks)
constexpr int GH_ROWS = 16;           // rows n per quadrature workgroup
// The "cv" pass for Kc warp terms per task (abc [T,3,Kc]) on the multi-task workspace's buffers -- what mt_gh_kernel writes
// (gm, rowred, colpart, ellpart) plus the parameter partials cvpart [T, ceil(N / GH_ROWS), 3 Kc] -- and their fixed-order
// reduction into grad_abc [T,3,Kc] = w_ell d ell / d(a,b,c).
int launch_mt_cv_pass(const float* M, const float* Lt, const float* y, const float* vx, const float* abc, int Kc,
                      const float* gh_x, const float* gh_w, int Q, float min_var, float min_scale, float w_ell, float* gm,
                      float* rowred, float* colpart, float* ellpart, float* cvpart, float* grad_abc, int N, int T,
                      hipStream_t s);

// ---- the Gauss-Hermite node bodies of the multi-task and the Markov steps.  (gpcv.hip's gh_ell_kernel / gh_cv_ell_kernel keep
// the same statements written out: calling these from there changed that file's gfx950 ISA)
// One node of the "exp" likelihood:  sc = max(exp f, min_scale),  logp = -y^2 / (2 sc^2) - log sc - log sqrt(2 pi),
//   g = dlogp/df = (y^2/sc^2 - 1) [exp f > min_scale];  lms = log min_scale.  The caller weighs and adds them up.
struct ExpNode {
    float logp, g;
};
__device__ __forceinline__ ExpNode exp_node(float f, float yi, float min_scale, float lms) {
    const float ef = expf(f);
    const bool live = ef > min_scale;
    const float sc = live ? ef : min_scale;
    const float r = yi / sc;
    return ExpNode{-0.5f * r * r - (live ? f : lms) - 0.91893853320467274f, live ? (r * r - 1.f) : 0.f};
}

// One node of the copula-process ("cv") likelihood:  s(f) = sum_k a_k softplus(b_k f + c_k),
//   sc = max(s, min_scale),  logp = -y^2 / (2 sc^2) - log sc - log sqrt(2 pi),  wg = w_q dlogp/ds = w_q (y^2/sc^2 - 1)/sc
//   [s > min_scale].  Adds w_q logp to e, wg ds/df to gm, wg ds/df x_q to gv, and wg (softplus(u_k), a_k sigmoid(u_k) f,
//   a_k sigmoid(u_k)) to the parameter sums ga, gb, gc.
template <int KC>
__device__ __forceinline__ void cv_node(float f, float xq, float wq, float yi, float min_scale, const float (&pa)[KC],
                                        const float (&pb)[KC], const float (&pc)[KC], float (&ga)[KC], float (&gb)[KC],
                                        float (&gc)[KC], float& e, float& gm, float& gv) {
    float sp[KC], sg[KC];
    float s = 0.f;
#pragma unroll
    for (int k = 0; k < KC; ++k) {
        const float u = pb[k] * f + pc[k];
        const float t = expf(-fabsf(u));
        const float inv = 1.f / (1.f + t);
        sp[k] = fmaxf(u, 0.f) + log1pf(t);
        sg[k] = u >= 0.f ? inv : t * inv;
        s += pa[k] * sp[k];
    }
    const bool live = s > min_scale;
    const float sc = live ? s : min_scale;
    const float r = yi / sc;
    const float logp = -0.5f * r * r - logf(sc) - 0.91893853320467274f;
    const float wg = live ? wq * (r * r - 1.f) / sc : 0.f;      // w_q g_s
    float dsdf = 0.f;
#pragma unroll
    for (int k = 0; k < KC; ++k) {
        const float as = pa[k] * sg[k];
        dsdf += as * pb[k];
        ga[k] += wg * sp[k];
        gb[k] += wg * as * f;
        gc[k] += wg * as;
    }
    e += wq * logp;
    gm += wg * dsdf;
    gv += wg * dsdf * xq;
}

}  // namespace volt
