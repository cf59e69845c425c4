// GPCV ELBO + gradient step for the Brownian-motion prior in O(N^2) (SingleTaskVariationalGP(prior_solver="linear")).
//
// The dense step (gpcv.hip) factors K + j I and forms G = K^-1 Lq with two structured GEMMs: 5 N^3 / 3 flop per series.  For
// K = v min(x, x') none of it is needed: A = v M + j I = D^-1 T D^-T with T tridiagonal, T = L diag(d) L' (bm.hip has the
// algebra, chain.h the recurrences: d_i, c_i = j / d_{i-1}, rho_i = j / d_i), so every column of G is one chain solve:
//     forward   z_i = (Lq_ij - Lq_{i-1,j}) + c_i z_{i-1}    from i = j (column j of Lq is zero above row j)
//               tr(A^-1 S) = sum_j sum_{i>=j} z_ij^2 / d_i
//     backward  w_i = z_i / d_i + rho_i w_{i+1},  G_ij = w_i - w_{i+1}    from N-1 down to j: only tril(G) enters dKL/dLq
//     above the diagonal z = 0 and G is a geometric tail:  sum_{i<j} G_ij^2 = w_jj^2 Q_j,
//               Q_0 = 0,  Q_{j+1} = rho_j^2 Q_j + (rho_j - 1)^2          (|G|_F^2 is needed for d/d vol only)
// r'A^-1 r, logdet A, tr A^-1, beta = A^-1 (m - mu) and |beta|^2 are volt_bm_step_f32's for the right-hand side m - mu, and
// 1/d_i is what that step leaves in its workspace (volt_internal_bm_inv).  The likelihood rows and the scalars are gpcv.hip's kernels.
//
//   gpcv_bm_cols_kernel    the hot path.  One wave per 64 adjacent columns of one series, lane = column, so every step of
//                          the chains reads (and writes) one whole 256-byte piece of a row of the row-major Lq / grad_Lq.
//                          Rows go by in blocks of GB_PF: the NEXT block's loads are requested into registers before the
//                          current block's chain runs (their addresses do not depend on the chain); the per-series vectors
//                          c_i, 1/d_i and the row kernel's dE/dvar_i are staged through LDS once per block and read as
//                          broadcasts.  z goes to the workspace as a row-packed fp64 lower triangle (a wave's piece of a row
//                          is contiguous there too).  The backward sweep fuses gpcv_grad_kernel:
//                              dF/dLq[i,j] = w_ell 2 gv_i Lq_ij - w_kl (G_ij - [i == j] / Lq_ii)   (j <= i), zero above,
//                          and leaves per column sum z^2/d, sum_{i>=j} G^2 and w_jj.  Elements of Lq above the diagonal are
//                          never read.  Chain arithmetic fp64, I/O fp32.
//   gpcv_bm_finish_kernel  one workgroup per series: the Q recurrence (256 chunks composed as affine maps, then one serial pass
//                          over the chunks), the three column sums in a fixed order, dF/dm and dF/dmu.
// No atomics; every reduction has a fixed order: the step is bitwise repeatable.
#include "common.h"
#include "chain.h"
#include "host.h"
#include "../../include/volt_hip.h"

namespace volt {

constexpr int GB_W = 64;                   // columns per workgroup (one wave)
constexpr int GB_PF = 32;                  // rows per register-prefetched block of the sweeps

__global__ __launch_bounds__(256) void gpcv_bm_sigma_kernel(float* __restrict__ sig, float jitter, int B) {
    const int b = blockIdx.x * 256 + threadIdx.x;
    if (b < B) sig[b] = jitter;
}

__global__ __launch_bounds__(GB_W) void gpcv_bm_cols_kernel(const float* __restrict__ Lq, const float* __restrict__ rowstat,
                                                            const double* __restrict__ inv, double* __restrict__ zt,
                                                            double* __restrict__ colv, float* __restrict__ gLq, double jit,
                                                            double we, double wk, int B, int N) {
    __shared__ double s_c[GB_PF], s_iv[GB_PF];
    __shared__ float s_gv[GB_PF];
    const int lane = threadIdx.x;
    const int64_t n = N, nb = B, b = blockIdx.y;
    const int64_t j0 = (int64_t)blockIdx.x * GB_W, j = j0 + lane;
    const bool col = j < n;
    const float* Lb = Lq + b * n * n;
    float* gb = gLq + b * n * n;
    double* zb = zt + b * (n * (n + 1) / 2);
    const int64_t nblk = (n - j0 + GB_PF - 1) / GB_PF;                 // blocks of rows j0 .. N-1

    // ---- forward sweep
    float nl[GB_PF];
    double piv = 0.0, paux = 0.0;
    auto request_f = [&](int64_t q) {
        const int64_t i0 = j0 + q * GB_PF;
#pragma unroll
        for (int u = 0; u < GB_PF; ++u) {
            const int64_t i = i0 + u;
            float v = 0.f;
            if (col && i < n && i >= j) v = Lb[i * n + j];
            nl[u] = v;
        }
        const int64_t i = i0 + lane;
        piv = 0.0;
        paux = 0.0;
        if (lane < GB_PF && i < n) {
            piv = inv[i * nb + b];
            if (i > 0) paux = inv[(i - 1) * nb + b];
        }
    };
    double zprev = 0.0, lprev = 0.0, tr = 0.0;
    request_f(0);
    for (int64_t q = 0; q < nblk; ++q) {
        float cl[GB_PF];
#pragma unroll
        for (int u = 0; u < GB_PF; ++u) cl[u] = nl[u];
        if (lane < GB_PF) {
            s_iv[lane] = piv;
            s_c[lane] = jit * paux;
        }
        __syncthreads();
        if (q + 1 < nblk) request_f(q + 1);                            // in flight while this block's chain runs
        const int64_t i0 = j0 + q * GB_PF;
        double zz[GB_PF];
#pragma unroll
        for (int u = 0; u < GB_PF; ++u) {
            const int64_t i = i0 + u;
            const bool on = col && i >= j && i < n;
            const double l = (double)cl[u];
            double z = chain_z_fwd(s_c[u], zprev, l - lprev);
            z = on ? z : 0.0;
            tr = on ? __builtin_fma(z * z, s_iv[u], tr) : tr;
            zprev = on ? z : zprev;
            lprev = on ? l : lprev;
            zz[u] = z;
        }
#pragma unroll
        for (int u = 0; u < GB_PF; ++u) {
            const int64_t i = i0 + u;
            if (col && i >= j && i < n) zb[i * (i + 1) / 2 + j] = zz[u];
        }
        __syncthreads();
    }

    // ---- backward sweep, fused with the gradient
    double nz[GB_PF];
    float pgv = 0.f;
    auto request_b = [&](int64_t q) {
        const int64_t i0 = j0 + q * GB_PF;
#pragma unroll
        for (int u = 0; u < GB_PF; ++u) {
            const int64_t i = i0 + u;
            float v = 0.f;
            double z = 0.0;
            if (col && i < n && i >= j) {
                v = Lb[i * n + j];
                z = zb[i * (i + 1) / 2 + j];
            }
            nl[u] = v;
            nz[u] = z;
        }
        const int64_t i = i0 + lane;
        piv = 0.0;
        pgv = 0.f;
        if (lane < GB_PF && i < n) {
            piv = inv[i * nb + b];
            pgv = rowstat[(b * n + i) * 4 + 2];
        }
    };
    const double rdiag = col ? 1.0 / (double)Lb[j * n + j] : 0.0;
    double wn = 0.0, gg = 0.0, wd = 0.0;
    request_b(nblk - 1);
    for (int64_t q = nblk - 1; q >= 0; --q) {
        float cl[GB_PF];
        double cz[GB_PF];
#pragma unroll
        for (int u = 0; u < GB_PF; ++u) cl[u] = nl[u], cz[u] = nz[u];
        if (lane < GB_PF) {
            s_iv[lane] = piv;
            s_gv[lane] = pgv;
        }
        __syncthreads();
        if (q > 0) request_b(q - 1);
        const int64_t i0 = j0 + q * GB_PF;
        float go[GB_PF];
#pragma unroll
        for (int u = GB_PF - 1; u >= 0; --u) {
            // a row past the end (last block only, where wn = 0) was staged as 1/d = z = 0 and gives w = 0
            const int64_t i = i0 + u;
            const bool on = col && i >= j && i < n;
            const double iv = s_iv[u];
            const double w = chain_z_back(jit * iv, wn, cz[u], iv);
            const double g = w - wn;
            const double kl = g - (i == j ? rdiag : 0.0);
            const double f = we * 2.0 * (double)s_gv[u] * (double)cl[u] - wk * kl;
            go[u] = on ? (float)f : 0.f;
            gg = on ? __builtin_fma(g, g, gg) : gg;
            wd = (on && i == j) ? w : wd;
            wn = on ? w : wn;
        }
#pragma unroll
        for (int u = 0; u < GB_PF; ++u) {
            const int64_t i = i0 + u;
            if (col && i < n) gb[i * n + j] = go[u];                   // (zeros above the diagonal inside the diagonal block)
        }
        __syncthreads();
    }
    if (col) {
#pragma unroll 8
        for (int64_t i = 0; i < j0; ++i) gb[i * n + j] = 0.f;          // the rows above this wave's diagonal block
        colv[(0 * nb + b) * n + j] = tr;
        colv[(1 * nb + b) * n + j] = gg;
        colv[(2 * nb + b) * n + j] = wd;
    }
}

// frob[b] = tr(A^-1 S), frob[B + b] = |G|_F^2 (one fp32 value each: gpcv_scalars_kernel's "tile" sums with one tile);
// dF/dm = we gm - wk beta, dF/dmu = wk beta as gpcv_grad_kernel forms them.
__global__ __launch_bounds__(256) void gpcv_bm_finish_kernel(const double* __restrict__ inv, const double* __restrict__ colv,
                                                             const float* __restrict__ rowstat, const float* __restrict__ beta,
                                                             double jit, float* __restrict__ frob, float* __restrict__ gm,
                                                             float* __restrict__ gmu, int B, int N, float we, float wk) {
    __shared__ double red[256], ra[256], rb[256];
    const int tid = threadIdx.x;
    const int64_t n = N, nb = B, b = blockIdx.x;
    for (int64_t i = tid; i < n; i += 256) {
        const float be = beta[b * n + i];
        gm[b * n + i] = we * rowstat[(b * n + i) * 4 + 1] - wk * be;
        gmu[b * n + i] = wk * be;
    }
    auto block_sum = [&](double v) -> double {
        red[tid] = v;
        __syncthreads();
        for (int s = 128; s > 0; s >>= 1) {
            if (tid < s) red[tid] += red[tid + s];
            __syncthreads();
        }
        const double r = red[0];
        __syncthreads();
        return r;
    };
    const double* ctr = colv + (0 * nb + b) * n;
    const double* cgg = colv + (1 * nb + b) * n;
    const double* cwd = colv + (2 * nb + b) * n;
    // thread t owns columns [lo, hi): its chunk of the recurrence as the affine map Q_hi = a Q_lo + c
    const int64_t chunk = (n + 255) / 256;
    const int64_t lo = tid * chunk < n ? tid * chunk : n, hi = lo + chunk < n ? lo + chunk : n;
    double a = 1.0, c = 0.0, str = 0.0, sgg = 0.0;
    for (int64_t i = lo; i < hi; ++i) {
        const double r = jit * inv[i * nb + b], r2 = r * r, e = r - 1.0;
        a *= r2;
        c = __builtin_fma(r2, c, e * e);
        str += ctr[i];
        sgg += cgg[i];
    }
    ra[tid] = a;
    rb[tid] = c;
    __syncthreads();
    if (tid == 0) {
        double q = 0.0;
        for (int t = 0; t < 256; ++t) {
            const double ta = ra[t], tc = rb[t];
            ra[t] = q;                                                 // Q at the chunk's first column
            q = __builtin_fma(ta, q, tc);
        }
    }
    __syncthreads();
    double q = ra[tid], tail = 0.0;
    for (int64_t i = lo; i < hi; ++i) {
        const double r = jit * inv[i * nb + b], e = r - 1.0, w = cwd[i];
        tail = __builtin_fma(w * w, q, tail);
        q = __builtin_fma(r * r, q, e * e);
    }
    str = block_sum(str);
    sgg = block_sum(sgg);
    tail = block_sum(tail);
    if (tid == 0) {
        frob[b] = (float)str;
        frob[nb + b] = (float)(sgg + tail);
    }
}

struct GpcvBmWs {
    void* bm;                              // volt_bm_step_f32's workspace (1/d_i out of it: volt_internal_bm_inv)
    double *z, *colv;                      // z: [B] row-packed lower triangles;  colv: [3][B][N]
    float *sig, *mllout, *beta, *rowstat, *frob, *cvpart;
    size_t bytes;
};

static GpcvBmWs carve_gpcv_bm(void* base, int B, int N, int Kc) {
    Carver c{base};
    const size_t b = (size_t)B, n = (size_t)N;
    GpcvBmWs w;
    w.bm = c.region(volt_bm_workspace_bytes(B, N, 1)).p;
    w.z = c.take<double>(b * (n * (n + 1) / 2));
    w.colv = c.take<double>(3 * b * n);
    w.sig = c.take<float>(b);
    w.mllout = c.take<float>(b * 8);
    w.beta = c.take<float>(b * n);
    w.rowstat = c.take<float>(b * n * 4);
    w.frob = c.take<float>(2 * b);
    w.cvpart = c.take<float>(Kc > 0 ? b * ((n + 3) / 4) * 3 * (size_t)Kc : 0);
    w.bytes = c.off;
    return w;
}

}  // namespace volt

using namespace volt;

extern "C" {

size_t volt_gpcv_bm_workspace_bytes(int B, int N, int Kc) {
    if (B < 1 || N < 1 || Kc < 0 || Kc > VOLT_GPCV_CV_K_MAX) return 0;
    return carve_gpcv_bm(nullptr, B, N, Kc).bytes;
}

int volt_gpcv_bm_step_f32(const float* x, const float* vol, float jitter, const float* resid, const float* m, const float* Lq,
                          const float* y, const float* abc, int Kc, const float* gh_x, const float* gh_w, int Q, float min_var,
                          float min_scale, float w_ell, float w_kl, float* out, float* grad_m, float* grad_mu, float* grad_Lq,
                          float* grad_abc, int* info, void* workspace, int B, int N, void* stream) {
    if (!x) return -1;
    if (!vol) return -2;
    if (!resid) return -4;
    if (!m) return -5;
    if (!Lq) return -6;
    if (!y) return -7;
    if (abc ? (Kc < 1 || Kc > VOLT_GPCV_CV_K_MAX) : Kc != 0) return -9;
    if (!gh_x) return -10;
    if (!gh_w) return -11;
    if (Q < 1 || Q > 1024) return -12;
    if (!out) return -17;
    if (!grad_m) return -18;
    if (!grad_mu) return -19;
    if (!grad_Lq) return -20;
    if (abc && !grad_abc) return -21;
    if (!info) return -22;
    if (!workspace || ((uintptr_t)workspace & 255)) return -23;
    if (B < 1 || B > 65535) return -24;
    if (N < 1) return -25;
    hipStream_t s = (hipStream_t)stream;
    const GpcvBmWs w = carve_gpcv_bm(workspace, B, N, abc ? Kc : 0);
    // the likelihood rows do not depend on the factor: enqueue them first
    int rc = volt_internal_gpcv_rows(m, Lq, y, abc, Kc, gh_x, gh_w, Q, min_var, min_scale, w_ell, w.rowstat, w.cvpart, grad_abc,
                                     B, N, s);
    if (rc) return rc;
    hipLaunchKernelGGL(gpcv_bm_sigma_kernel, dim3((B + 255) / 256), dim3(256), 0, s, w.sig, jitter, B);
    VOLT_LAUNCH_CHECK();
    // d_i, beta = A^-1 resid, r'A^-1 r, logdet A, tr A^-1, |beta|^2, info: the vol forecaster's step with sigma2 = jitter
    rc = volt_bm_step_f32(x, vol, w.sig, resid, w.mllout, w.beta, info, w.bm, B, N, VOLT_WANT_GRAD, stream);
    if (rc) return rc;
    const double* inv = volt_internal_bm_inv(w.bm);
    hipLaunchKernelGGL(gpcv_bm_cols_kernel, dim3((N + GB_W - 1) / GB_W, B), dim3(GB_W), 0, s, Lq, w.rowstat, inv, w.z, w.colv,
                       grad_Lq, (double)jitter, (double)w_ell, (double)w_kl, B, N);
    VOLT_LAUNCH_CHECK();
    hipLaunchKernelGGL(gpcv_bm_finish_kernel, dim3(B), dim3(256), 0, s, inv, w.colv, w.rowstat, w.beta, (double)jitter, w.frob,
                       grad_m, grad_mu, B, N, w_ell, w_kl);
    VOLT_LAUNCH_CHECK();
    return volt_internal_gpcv_scalars(w.rowstat, w.mllout, w.frob, w.frob + B, jitter, out, B, N, 1, w_ell, w_kl, s);
}

}  // extern "C"
