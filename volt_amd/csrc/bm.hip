// Linear-time solver for the Brownian-motion prior of the vol forecaster (models/BMGP.py, solver="linear").
//
// K = v M, M = min(x_i, x_k) over a grid 0 <= x_0 < x_1 < ...  With D the first-difference operator (unit lower bidiagonal)
// D M D' = diag(delta), delta_0 = x_0, delta_i = x_i - x_{i-1}, so A = v M + s I = D^-1 T D^-T with the SPD tridiagonal
// T = v diag(delta) + s D D' (D D': diagonal 1, 2, 2, .., off-diagonals -1).  T = L diag(d) L' with L unit lower bidiagonal,
// L_{i,i-1} = -c_i:
//     d_0 = v delta_0 + s,   c_i = s / d_{i-1},   d_i = v delta_i + 2 s - s c_i
//     forward   u = D r,  z_i = u_i + c_i z_{i-1}                     logdet = sum log d_i,  r'A^-1 r = sum z_i^2 / d_i
//     backward  w_i = z_i / d_i + (s / d_i) w_{i+1},  alpha = D'w     (alpha_i = w_i - w_{i+1})
//     trace     G = T^-1:  G_ii = 1/d_i + (s/d_i)^2 G_{i+1,i+1},  G_{i,i+1} = (s/d_i) G_{i+1,i+1},
//               tr A^-1 = tr(D'G D) = sum_i (1 + [i>0]) G_ii - 2 sum_i G_{i,i+1}
// All arithmetic is fp64 whatever the I/O type; nothing is O(N^2); no atomics, every sum has a fixed order.
//
//   bm_step_kernel    one lane per series, ONE wave per workgroup (B > 64 spreads over CUs).  resid [B,N] is staged through
//                     LDS in transposed tiles of 64 series x 64 steps (whole 256 / 512-byte rows from global memory, a
//                     conflict-free column per lane out of LDS); the next tile's rows are requested into registers before the
//                     current tile's chain runs.  1/d_i and z_i go to the workspace series-fastest for the backward sweep,
//                     which reads them sixteen steps ahead and sends alpha back through the same LDS tile.
//                     The chain is one FMA and one reciprocal per step (chain.h); the log, the z chain and the sums hang off it.
//                     VK = true (volt_vk_step_*, the volatility-kernel data model: K_b = V_b[min(i,k)], v = 1): every series
//                     has its OWN grid V_b, staged like resid through a second transposed LDS tile; the lane carries
//                     V_{b,i-1} and forms delta in fp64.  Both arrays then travel in tiles of BM_VT = 32 steps (two rows per
//                     load: the half-waves take neighbouring series), so that the two register prefetches together are as
//                     deep as the one of the shared-grid kernel.  Chain, sums and the backward sweep are the same code.
//   bm_forms_kernel   (volt_vk_forms_*, the forecast's conditioning: DESIGN 4.15) the VK forward sweep with a second z chain over D V
//                     next to the one over D r: V'A^-1 V, V'A^-1 r, r'A^-1 r, logdet A in doubles.  No workspace; jitter 0 allowed.
//   bm_post_kernel    (volt_bm_post_*, the vol forecaster's posterior: DESIGN 4.16) one wave per (series, 64 sorted test points):
//                     the pivot chain and z^r wave-uniform off broadcast LDS reads, per lane the z chains of its test point and
//                     of the next one over clipped grid increments, and the sums m, p, q.  Forward sweep only, no workspace.
//   bm_factor_kernel  the d chain alone, 1/d_i -> workspace (the solve's factorisation, once per series).
//   bm_solve_kernel   one lane per (series, right-hand side): R [B,N,H] with H contiguous, so the lanes of a series load and
//                     store whole rows.  Forward z -> workspace, backward X = D'w.  Its chains are one FMA per step.
#include "common.h"
#include "chain.h"
#include "host.h"
#include "../../include/volt_hip.h"

namespace volt {

constexpr int BM_T = 64;                   // tile edge: series per workgroup, steps per staged tile
constexpr int BM_VT = 32;                  // steps per staged tile of the per-series-grid step (VK): resid and V, half as deep each
constexpr int BM_VLD = BM_VT + 1;          // LDS row stride of its V tile
constexpr int BM_LD = BM_T + 1;            // LDS row stride (doubles): a column read by 64 lanes touches every bank pair once
constexpr int BM_PF = 16;                  // steps per register-prefetched block of the workspace sweeps
constexpr int BM_FB = 8;                   // steps per block of the step kernel's forward chain (divides BM_T)
constexpr double BM_LOG_2PI = 1.837877066409345483560659472811;

template <typename T>
struct BmStepParams {
    const T *x, *vol, *sigma2, *resid;     // x: the shared grid [N], or (VK) the per-series grids [B,N] with batch stride bsx; vol NULL: 1
    T *out, *alpha;
    int* info;
    double *inv, *zs;                      // [N][B], series-fastest (inv: volt_internal_bm_inv hands it to gpcv_bm.hip)
    int64_t B, N, bsx;
};

// A staged tile of TS steps x BM_T series of src [B,N] (batch stride bs) that starts at step i0: BM_T / TS rows per load, the
// lanes of a row on consecutive steps, TS registers per lane.  Rows r >= nb and steps >= N come as 0.
template <typename T, int TS>
__device__ __forceinline__ void bm_fetch_rows(const T* src, int64_t bs, int64_t b0, int nb, int64_t i0, int64_t N, T (&pre)[TS]) {
    constexpr int RP = BM_T / TS;
    const int sub = RP == 1 ? 0 : threadIdx.x / TS;                    // (RP == 1: r < nb stays wave-uniform)
    const int64_t i = i0 + (RP == 1 ? threadIdx.x : threadIdx.x % TS);
    const bool in = i < N;
#pragma unroll
    for (int k = 0; k < TS; ++k) {
        const int r = k * RP + sub;
        const int64_t row = (b0 + k * RP) * bs;                          // (wave-uniform; the half-wave picks its row)
        T val = (T)0;
        if (r < nb && in) val = src[(sub ? row + bs : row) + i];
        pre[k] = val;
    }
}
template <typename T, int TS>
__device__ __forceinline__ void bm_commit_rows(double* tile, int ld, int nb, const T (&pre)[TS]) {
    constexpr int RP = BM_T / TS;
    const int sub = RP == 1 ? 0 : threadIdx.x / TS, st = RP == 1 ? threadIdx.x : threadIdx.x % TS;
#pragma unroll
    for (int k = 0; k < TS; ++k) {
        const int r = k * RP + sub;
        if (r < nb) tile[r * ld + st] = (double)pre[k];
    }
}
// the shared grid's points x_i, x_{i-1} of the tile that starts at step i0 (lane = step)
template <typename T>
__device__ __forceinline__ void bm_fetch_grid(const BmStepParams<T>& p, int64_t i0, T& px, T& pxm) {
    const int64_t i = i0 + threadIdx.x;
    const bool in = i < p.N;
    px = pxm = (T)0;
    if (in) px = p.x[i];
    if (in && i > 0) pxm = p.x[i - 1];
}

template <typename T, bool GRAD, bool VK>
__global__ __launch_bounds__(BM_T) void bm_step_kernel(BmStepParams<T> p) {
    constexpr int TS = VK ? BM_VT : BM_T;                               // steps per staged tile of the forward sweep
    __shared__ double tile[BM_T * BM_LD];
    __shared__ double gl[VK ? BM_T * BM_VLD : BM_T];                    // VK: the V tile [series][step]; else delta of the tile's steps
    const int lane = threadIdx.x;
    const int64_t N = p.N, B = p.B;
    const int64_t b0 = (int64_t)blockIdx.x * BM_T;
    const int nb = (int)(B - b0 < BM_T ? B - b0 : BM_T);              // series of this workgroup (wave-uniform)
    const bool act = lane < nb;
    const int64_t b = b0 + lane;
    const double v = act && !VK ? (double)p.vol[b] : 1.0, s = act ? (double)p.sigma2[b] : 1.0;
    const ChainBm ch(s);

    // ---- forward sweep
    T pre[TS], pg[VK ? TS : 2];                                        // pg: (VK) the V tile's rows; else x_i, x_{i-1} of this lane's step
    auto fetch = [&](int64_t i0) {
        bm_fetch_rows<T, TS>(p.resid, N, b0, nb, i0, N, pre);
        if constexpr (VK) bm_fetch_rows<T, TS>(p.x, p.bsx, b0, nb, i0, N, pg);
        else bm_fetch_grid(p, i0, pg[0], pg[1]);
    };
    fetch(0);
    double inv_prev = 0.0, zprev = 0.0, rprev = 0.0, gprev = 0.0, quad = 0.0, P = 1.0;
    int64_t E = 0;
    int info = 0;
    for (int64_t i0 = 0; i0 < N; i0 += TS) {
        bm_commit_rows<T, TS>(tile, BM_LD, nb, pre);
        if constexpr (VK) bm_commit_rows<T, TS>(gl, BM_VLD, nb, pg);
        else gl[lane] = (double)pg[0] - (double)pg[1];
        __syncthreads();
        if (i0 + TS < N) fetch(i0 + TS);                                       // in flight while this tile's chain runs
        const int cnt = (int)(N - i0 < TS ? N - i0 : TS);
        int e = 0;
        // blocks of BM_FB steps: their LDS reads first (one wait), the chain in one basic block (a step past the tile's end --
        // last tile only -- reads stale LDS and is discarded by selects, not branches), then the block's stores
        for (int j0 = 0; j0 < cnt; j0 += BM_FB) {
            double rr[BM_FB], dd[BM_FB], iv[BM_FB], zz[BM_FB];
#pragma unroll
            for (int u = 0; u < BM_FB; ++u) {
                rr[u] = tile[lane * BM_LD + j0 + u];
                dd[u] = VK ? gl[lane * BM_VLD + j0 + u] : gl[j0 + u];
            }
            if constexpr (VK) {                                                // delta_i = V_i - V_{i-1} (V_{-1} = 0), exact in fp64
#pragma unroll
                for (int u = 0; u < BM_FB; ++u) {
                    const double g = dd[u];
                    dd[u] = g - gprev;
                    gprev = j0 + u < cnt ? g : gprev;
                }
            }
#pragma unroll
            for (int u = 0; u < BM_FB; ++u) {
                const int64_t i = i0 + j0 + u;
                const bool on = j0 + u < cnt;
                const ChainPivot pv = ch.pivot(inv_prev, ch.base(v, dd[u], i));   // the chain: one FMA and the reciprocal
                const double d = pv.d, inv = pv.inv, z = chain_z_fwd(pv.c, zprev, rr[u] - rprev);
                quad = on ? __builtin_fma(z * z, inv, quad) : quad;
                P = ChainLogDet::mul(P, d, on);
                e += ChainLogDet::exp(d, on);
                if (on && !chain_pivot_ok(d) && info == 0) info = chain_fail_code(i);
                iv[u] = inv;
                zz[u] = z;
                inv_prev = on ? inv : inv_prev;
                zprev = on ? z : zprev;
                rprev = on ? rr[u] : rprev;
            }
            if (GRAD && act) {
#pragma unroll
                for (int u = 0; u < BM_FB; ++u)
                    if (j0 + u < cnt) {
                        const int64_t i = i0 + j0 + u;
                        p.inv[i * B + b] = iv[u];
                        p.zs[i * B + b] = zz[u];
                    }
            }
        }
        e += ChainLogDet::exp(P);                                              // (at most BM_T mantissas in [1/2, 1) since the last time)
        P = ChainLogDet::mant(P);
        E += e;
        __syncthreads();
    }
    const double logdet = info ? __builtin_nan("") : ChainLogDet::value(P, E);
    const double nd = (double)N;
    if (act) {
        T* o = p.out + b * 8;
        o[0] = (T)(-0.5 * (quad + logdet + nd * BM_LOG_2PI) / nd);
        o[2] = (T)quad;
        o[3] = (T)logdet;
        o[6] = (T)s;
        o[7] = (T)v;
        p.info[b] = info;
    }
    if constexpr (!GRAD) return;

    // ---- backward sweep: blocks of BM_PF steps from the end, the block below already requested
    double ci[BM_PF], cz[BM_PF], ni[BM_PF], nz[BM_PF];
    auto request = [&](int64_t q) {
#pragma unroll
        for (int j = 0; j < BM_PF; ++j) {
            const int64_t i = q * BM_PF + j;
            double a = 0.0, c = 0.0;
            if (act && i < N) {
                a = p.inv[i * B + b];
                c = p.zs[i * B + b];
            }
            ni[j] = a;
            nz[j] = c;
        }
    };
    double wn = 0.0, gn = 0.0, aa = 0.0, tr = 0.0;
    const int64_t qlast = (N - 1) / BM_PF;
    request(qlast);
    for (int64_t q = qlast; q >= 0; --q) {
#pragma unroll
        for (int j = 0; j < BM_PF; ++j) ci[j] = ni[j], cz[j] = nz[j];
        if (q > 0) request(q - 1);
#pragma unroll
        for (int j = BM_PF - 1; j >= 0; --j) {
            // no guard: a step past the end (first block only, where wn = gn = 0) was requested as 1/d = z = 0 and so gives
            // w = g = alpha = 0, adds nothing to the sums, and lands in a tile column that is never sent out
            const int64_t i = q * BM_PF + j;
            const double inv = ci[j], e = s * inv;
            const double w = chain_z_back(e, wn, cz[j], inv);
            const double a = w - wn;
            aa = __builtin_fma(a, a, aa);
            const double g = __builtin_fma(e * e, gn, inv);
            tr += __builtin_fma(-2.0 * e, gn, (i > 0 ? 2.0 : 1.0) * g);
            tile[lane * BM_LD + (int)(i & (BM_T - 1))] = a;
            wn = w;
            gn = g;
        }
        if ((q & (BM_T / BM_PF - 1)) == 0) {                                   // a tile of alpha is complete: rows go out whole
            __syncthreads();
            const int64_t i = q * BM_PF + lane;
            if (i < N) {
#pragma unroll 8
                for (int r = 0; r < nb; ++r) p.alpha[(b0 + r) * N + i] = (T)tile[r * BM_LD + lane];
            }
            __syncthreads();
        }
    }
    if (act) {
        T* o = p.out + b * 8;
        o[1] = (T)(0.5 * (aa - tr) / nd);
        o[4] = (T)tr;
        o[5] = (T)aa;
    }
}

template <typename T>
struct BmFormsParams {
    const T *V, *resid;                    // V: the per-series grids [B,N] with batch stride bsv (0: one grid for all)
    const double* jitter;                  // [B], >= 0
    double* out;                           // [B,4]
    int* info;
    int64_t B, N, bsv;
};

// The conditioning scalars of a forecast from the volatility-kernel data model (volt_vk_forms_*): per series, with
// A = V[min(i,k)] + j I, the forms V'A^-1 V, V'A^-1 r, r'A^-1 r and logdet A.  The forward sweep of the VK step with TWO z
// chains on the one pivot chain -- z^V over D V = delta, z^r over D r -- and nothing else: no workspace, no backward sweep.
// (Written out next to bm_step_kernel's, not shared with it: either way of sharing the sweep cost these chains ~1 %)
// j = 0 is legal (c_i = 0, d_i = delta_i: the forms are then V_{N-1}, r_{N-1}, sum (D r)_i^2 / delta_i, sum log delta_i).
template <typename T>
__global__ __launch_bounds__(BM_T) void bm_forms_kernel(BmFormsParams<T> p) {
    constexpr int TS = BM_VT;
    __shared__ double tile[BM_T * BM_LD];                               // resid [series][step]
    __shared__ double gl[BM_T * BM_VLD];                                // V [series][step]
    const int lane = threadIdx.x;
    const int64_t N = p.N, B = p.B;
    const int64_t b0 = (int64_t)blockIdx.x * BM_T;
    const int nb = (int)(B - b0 < BM_T ? B - b0 : BM_T);
    const bool act = lane < nb;
    const int64_t b = b0 + lane;
    const ChainBm ch(act ? p.jitter[b] : 1.0);

    T pre[TS], pg[TS];
    auto fetch = [&](int64_t i0) {
        bm_fetch_rows<T, TS>(p.resid, N, b0, nb, i0, N, pre);
        bm_fetch_rows<T, TS>(p.V, p.bsv, b0, nb, i0, N, pg);
    };
    fetch(0);
    double inv_prev = 0.0, zr = 0.0, zv = 0.0, rprev = 0.0, gprev = 0.0, rho = 0.0, tau = 0.0, quad = 0.0, P = 1.0;
    int64_t E = 0;
    int info = 0;
    for (int64_t i0 = 0; i0 < N; i0 += TS) {
        bm_commit_rows<T, TS>(tile, BM_LD, nb, pre);
        bm_commit_rows<T, TS>(gl, BM_VLD, nb, pg);
        __syncthreads();
        if (i0 + TS < N) fetch(i0 + TS);                                       // in flight while this tile's chains run
        const int cnt = (int)(N - i0 < TS ? N - i0 : TS);
        int e = 0;
        for (int j0 = 0; j0 < cnt; j0 += BM_FB) {                              // (as bm_step_kernel: stale steps are discarded by selects)
            double rr[BM_FB], dd[BM_FB];
#pragma unroll
            for (int u = 0; u < BM_FB; ++u) {
                rr[u] = tile[lane * BM_LD + j0 + u];
                dd[u] = gl[lane * BM_VLD + j0 + u];
            }
#pragma unroll
            for (int u = 0; u < BM_FB; ++u) {                                  // delta_i = V_i - V_{i-1} (V_{-1} = 0), exact in fp64
                const double g = dd[u];
                dd[u] = g - gprev;
                gprev = j0 + u < cnt ? g : gprev;
            }
#pragma unroll
            for (int u = 0; u < BM_FB; ++u) {
                const int64_t i = i0 + j0 + u;
                const bool on = j0 + u < cnt;
                const ChainPivot pv = ch.pivot(inv_prev, ch.base(1.0, dd[u], i)); // (v = 1: fma(1.0, delta, s) is folded to delta + s)
                const double d = pv.d, inv = pv.inv, a = chain_z_fwd(pv.c, zv, dd[u]);   // z^V_i = delta_i + c_i z^V_{i-1}
                const double z = chain_z_fwd(pv.c, zr, rr[u] - rprev);         // z^r_i = (r_i - r_{i-1}) + c_i z^r_{i-1}
                rho = on ? __builtin_fma(a * a, inv, rho) : rho;
                tau = on ? __builtin_fma(a * z, inv, tau) : tau;
                quad = on ? __builtin_fma(z * z, inv, quad) : quad;
                P = ChainLogDet::mul(P, d, on);
                e += ChainLogDet::exp(d, on);
                if (on && !chain_pivot_ok(d) && info == 0) info = chain_fail_code(i);
                inv_prev = on ? inv : inv_prev;
                zv = on ? a : zv;
                zr = on ? z : zr;
                rprev = on ? rr[u] : rprev;
            }
        }
        e += ChainLogDet::exp(P);
        P = ChainLogDet::mant(P);
        E += e;
        __syncthreads();
    }
    if (act) {
        const double nan = __builtin_nan("");
        double* o = p.out + b * 4;
        o[0] = info ? nan : rho;
        o[1] = info ? nan : tau;
        o[2] = info ? nan : quad;
        o[3] = info ? nan : ChainLogDet::value(P, E);
        p.info[b] = info;
    }
}

template <typename T>
struct BmPostParams {
    const T *x, *xs, *vol, *sigma2, *resid; // x: the grid [N] (bsx = 0) or per-series grids [B,N] with batch stride bsx; xs [H] ascending
    double* out;                           // [B,3,H]: rows m, p, q
    int* info;
    int64_t B, N, H, bsx;
};

// The posterior of the Brownian-motion vol forecaster at H sorted test points xi_0 <= .. <= xi_{H-1} (volt_bm_post_*; DESIGN
// 4.16): per series the forms m_h = k_h'A^-1 r, p_h = k_h'A^-1 k_h, q_h = k_h'A^-1 k_{h+1} (q_{H-1} = p_{H-1}) of the columns
// k_h = v min(x, xi_h), from the forward sweep alone.  (D k_h)_i = v clamp(xi_h - x_{i-1}, 0, delta_i) is formed on the fly, so
// nothing is N x H.  One wave per (series, block of 64 test points): the pivot chain, z^r and the staged tile (delta_i, x_{i-1},
// (D r)_i, one step per lane into LDS, read back as broadcasts) are the same in every lane; a lane carries the z chain of its
// own point and of its right neighbour (the last point's neighbour is the point itself) and the three running sums.  No
// workspace, no atomics, no traffic between lanes or waves: every sum has a fixed order.
template <typename T>
__global__ __launch_bounds__(BM_T) void bm_post_kernel(BmPostParams<T> p) {
    __shared__ double sd[BM_T], sx[BM_T], sr[BM_T];
    const int lane = threadIdx.x;
    const int64_t N = p.N, H = p.H;
    const int64_t b = blockIdx.x, h = (int64_t)blockIdx.y * BM_T + lane;
    const bool act = h < H;
    const double nan = __builtin_nan("");
    double* o = p.out + b * 3 * H + h;

    // the test points, checked by every wave (H / 64 loads): the first that is NaN / inf, negative or below its predecessor
    for (int64_t h0 = 0; h0 < H; h0 += BM_T) {
        const int64_t k = h0 + lane;
        double a = 0.0, pr = 0.0;
        if (k < H) a = (double)p.xs[k];
        if (k < H && k > 0) pr = (double)p.xs[k - 1];
        const unsigned long long bad = __ballot(!(a >= pr && a < __builtin_inf()));     // (a lane past H holds 0 >= 0)
        if (bad) {
            if (act) o[0] = nan, o[H] = nan, o[2 * H] = nan;
            if (blockIdx.y == 0 && lane == 0) p.info[b] = -(int)(h0 + __builtin_ctzll(bad) + 1);
            return;
        }
    }

    const double xa = act ? (double)p.xs[h] : 0.0, xb = act ? (double)p.xs[h + 1 < H ? h + 1 : h] : 0.0;
    const double v = (double)p.vol[b];
    const ChainBm ch((double)p.sigma2[b]);
    const T* xg = p.x + b * p.bsx;
    const T* rg = p.resid + b * N;

    T px, pxm, pr, prm;                                                // x_i, x_{i-1}, r_i, r_{i-1} of this lane's step of the next tile
    auto fetch = [&](int64_t i0) {
        const int64_t i = i0 + lane;
        px = pxm = pr = prm = (T)0;
        if (i < N) px = xg[i], pr = rg[i];
        if (i < N && i > 0) pxm = xg[i - 1], prm = rg[i - 1];
    };
    fetch(0);
    double inv_prev = 0.0, zr = 0.0, za = 0.0, zb = 0.0, m = 0.0, pp = 0.0, q = 0.0;
    int info = 0;
    auto step = [&](int64_t i, double dl, double xp, double dr) {
        const ChainPivot pv = ch.pivot(inv_prev, ch.base(v, dl, i));
        const double c = pv.c;
        zr = chain_z_fwd(c, zr, dr);
        // (D k)_i by selects: v delta_i up to the bracket, the partial increment at it, 0 after; xi >= x_i gives delta_i exactly
        za = chain_z_fwd(c, za, v * __builtin_fmin(__builtin_fmax(xa - xp, 0.0), dl));
        zb = chain_z_fwd(c, zb, v * __builtin_fmin(__builtin_fmax(xb - xp, 0.0), dl));
        const double w = za * pv.inv;
        m = __builtin_fma(w, zr, m);
        pp = __builtin_fma(w, za, pp);
        q = __builtin_fma(w, zb, q);
        if (!chain_pivot_ok(pv.d) && info == 0) info = chain_fail_code(i);
        inv_prev = pv.inv;
    };
    for (int64_t i0 = 0; i0 < N; i0 += BM_T) {
        sd[lane] = (double)px - (double)pxm;
        sx[lane] = (double)pxm;
        sr[lane] = (double)pr - (double)prm;
        __syncthreads();
        if (i0 + BM_T < N) fetch(i0 + BM_T);                                   // in flight while this tile's chains run
        const int cnt = (int)(N - i0 < BM_T ? N - i0 : BM_T);                  // (wave-uniform: the loops below do not diverge)
        int j0 = 0;
        for (; j0 + BM_FB <= cnt; j0 += BM_FB) {
            double dd[BM_FB], xp[BM_FB], rr[BM_FB];
#pragma unroll
            for (int u = 0; u < BM_FB; ++u) dd[u] = sd[j0 + u], xp[u] = sx[j0 + u], rr[u] = sr[j0 + u];
#pragma unroll
            for (int u = 0; u < BM_FB; ++u) step(i0 + j0 + u, dd[u], xp[u], rr[u]);
        }
        for (; j0 < cnt; ++j0) step(i0 + j0, sd[j0], sx[j0], sr[j0]);          // the last tile's remainder
        __syncthreads();
    }
    if (act) o[0] = info ? nan : m, o[H] = info ? nan : pp, o[2 * H] = info ? nan : q;
    if (blockIdx.y == 0 && lane == 0) p.info[b] = info;
}

template <typename T>
struct BmSolveParams {
    const T *x, *vol, *sigma2, *R;
    T* X;
    int* info;
    double *inv, *zs;                      // [N][B] and [N][B H]
    int64_t B, N, H;
};

// the d chain alone: one lane per series
template <typename T>
__global__ __launch_bounds__(BM_T) void bm_factor_kernel(BmSolveParams<T> p) {
    const int64_t b = (int64_t)blockIdx.x * BM_T + threadIdx.x;
    const int64_t N = p.N, B = p.B;
    const bool act = b < B;
    const double v = act ? (double)p.vol[b] : 1.0;
    const ChainBm ch(act ? (double)p.sigma2[b] : 1.0);
    double inv_prev = 0.0, xprev = 0.0;
    int info = 0;
    for (int64_t i0 = 0; i0 < N; i0 += BM_PF) {
        double xs[BM_PF];
#pragma unroll
        for (int j = 0; j < BM_PF; ++j) xs[j] = i0 + j < N ? (double)p.x[i0 + j] : 0.0;     // (uniform: scalar loads)
#pragma unroll
        for (int j = 0; j < BM_PF; ++j) {
            const int64_t i = i0 + j;
            if (i < N) {
                const ChainPivot pv = ch.pivot(inv_prev, ch.base(v, xs[j] - xprev, i));
                if (!chain_pivot_ok(pv.d) && info == 0) info = chain_fail_code(i);
                if (act) p.inv[i * B + b] = pv.inv;
                inv_prev = pv.inv;
                xprev = xs[j];
            }
        }
    }
    if (act) p.info[b] = info;
}

template <typename T>
__global__ __launch_bounds__(BM_T) void bm_solve_kernel(BmSolveParams<T> p) {
    const int64_t g = (int64_t)blockIdx.x * BM_T + threadIdx.x;
    const int64_t N = p.N, B = p.B, H = p.H, BH = B * H;
    const bool act = g < BH;
    const int64_t b = act ? g / H : 0, h = act ? g % H : 0;
    const double s = act ? (double)p.sigma2[b] : 1.0;
    const T* R = p.R + b * N * H + h;
    T* X = p.X + b * N * H + h;
    const int64_t nq = (N + BM_PF - 1) / BM_PF;

    // ---- forward: z_i = (r_i - r_{i-1}) + s / d_{i-1} z_{i-1}
    double cr[BM_PF], ci[BM_PF], nr[BM_PF], ni[BM_PF];
    auto request_f = [&](int64_t q) {
#pragma unroll
        for (int j = 0; j < BM_PF; ++j) {
            const int64_t i = q * BM_PF + j;
            double r = 0.0, a = 0.0;
            if (act && i < N) {
                r = (double)R[i * H];
                if (i > 0) a = p.inv[(i - 1) * B + b];
            }
            nr[j] = r;
            ni[j] = a;
        }
    };
    double zprev = 0.0, rprev = 0.0;
    request_f(0);
    for (int64_t q = 0; q < nq; ++q) {
#pragma unroll
        for (int j = 0; j < BM_PF; ++j) cr[j] = nr[j], ci[j] = ni[j];
        if (q + 1 < nq) request_f(q + 1);
#pragma unroll
        for (int j = 0; j < BM_PF; ++j) {
            const int64_t i = q * BM_PF + j;
            if (i < N) {
                const double z = chain_z_fwd(s * ci[j], zprev, cr[j] - rprev);
                if (act) p.zs[i * BH + g] = z;
                zprev = z;
                rprev = cr[j];
            }
        }
    }

    // ---- backward: w_i = z_i / d_i + s / d_i w_{i+1},  X_i = w_i - w_{i+1}   (this lane reads back its own z)
    auto request_b = [&](int64_t q) {
#pragma unroll
        for (int j = 0; j < BM_PF; ++j) {
            const int64_t i = q * BM_PF + j;
            double z = 0.0, a = 0.0;
            if (act && i < N) {
                z = p.zs[i * BH + g];
                a = p.inv[i * B + b];
            }
            nr[j] = z;
            ni[j] = a;
        }
    };
    double wn = 0.0;
    request_b(nq - 1);
    for (int64_t q = nq - 1; q >= 0; --q) {
#pragma unroll
        for (int j = 0; j < BM_PF; ++j) cr[j] = nr[j], ci[j] = ni[j];
        if (q > 0) request_b(q - 1);
#pragma unroll
        for (int j = BM_PF - 1; j >= 0; --j) {
            const int64_t i = q * BM_PF + j;
            if (i < N) {
                const double w = chain_z_back(s * ci[j], wn, cr[j], ci[j]);
                if (act) X[i * H] = (T)(w - wn);
                wn = w;
            }
        }
    }
}

inline size_t bm_inv_bytes(int64_t B, int64_t N) { return al256((size_t)B * (size_t)N * sizeof(double)); }

// the checked launch of both steps; VK (volt_vk_step_*): x the per-series grids V [B,N] with batch stride bsx (0: one grid), no vol
template <typename T, bool VK>
int bm_step(const T* x, int64_t bsx, const T* vol, const T* sigma2, const T* resid, T* out, T* alpha, int* info, void* workspace,
            int B, int N, int flags, void* stream) {
    if (!x) return -1;
    if (VK ? (bsx < 0 || (bsx > 0 && bsx < N)) : !vol) return -2;
    if (!sigma2) return -3;
    if (!resid) return -4;
    if (!out) return -5;
    const bool grad = (flags & VOLT_WANT_GRAD) != 0;
    if (grad && !alpha) return -6;
    if (!info) return -7;
    if (grad && (!workspace || ((uintptr_t)workspace & 255))) return -8;
    if (B < 1) return -9;
    if (N < 1) return -10;
    if (flags & ~VOLT_WANT_GRAD) return -11;
    BmStepParams<T> p{x, vol, sigma2, resid, out, alpha, info, (double*)workspace,
                      (double*)((char*)workspace + (grad ? bm_inv_bytes(B, N) : 0)), B, N, bsx};
    const dim3 grid((unsigned)((B + BM_T - 1) / BM_T));
    if (grad) hipLaunchKernelGGL((bm_step_kernel<T, true, VK>), grid, dim3(BM_T), 0, (hipStream_t)stream, p);
    else hipLaunchKernelGGL((bm_step_kernel<T, false, VK>), grid, dim3(BM_T), 0, (hipStream_t)stream, p);
    VOLT_LAUNCH_CHECK();
    return 0;
}

// V'A^-1 V, V'A^-1 r, r'A^-1 r and logdet A for A_b = V_b[min(i,k)] + jitter_b I: the forward sweep alone, doubles out
template <typename T>
int vk_forms(const T* V, int64_t bsv, const double* jitter, const T* resid, double* out, int* info, int B, int N, void* stream) {
    if (!V) return -1;
    if (bsv < 0 || (bsv > 0 && bsv < N)) return -2;
    if (!jitter) return -3;
    if (!resid) return -4;
    if (!out) return -5;
    if (!info) return -6;
    if (B < 1) return -7;
    if (N < 1) return -8;
    BmFormsParams<T> p{V, resid, jitter, out, info, B, N, bsv};
    hipLaunchKernelGGL((bm_forms_kernel<T>), dim3((unsigned)((B + BM_T - 1) / BM_T)), dim3(BM_T), 0, (hipStream_t)stream, p);
    VOLT_LAUNCH_CHECK();
    return 0;
}

// m_h, p_h, q_h of the Brownian-motion posterior at H sorted test points: the forward sweep alone, doubles out
template <typename T>
int bm_post(const T* x, int64_t bsx, const T* xs, const T* vol, const T* sigma2, const T* resid, double* out, int* info, int B,
            int N, int H, void* stream) {
    if (!x) return -1;
    if (bsx < 0 || (bsx > 0 && bsx < N)) return -2;
    if (!xs) return -3;
    if (!vol) return -4;
    if (!sigma2) return -5;
    if (!resid) return -6;
    if (!out) return -7;
    if (!info) return -8;
    if (B < 1) return -9;
    if (N < 1) return -10;
    const int64_t blocks = ((int64_t)H + BM_T - 1) / BM_T;
    if (H < 1 || blocks > 65535) return -11;
    BmPostParams<T> p{x, xs, vol, sigma2, resid, out, info, B, N, H, bsx};
    hipLaunchKernelGGL((bm_post_kernel<T>), dim3((unsigned)B, (unsigned)blocks), dim3(BM_T), 0, (hipStream_t)stream, p);
    VOLT_LAUNCH_CHECK();
    return 0;
}

template <typename T>
int bm_solve(const T* x, const T* vol, const T* sigma2, const T* R, T* X, int* info, void* workspace, int B, int N, int H,
             void* stream) {
    if (!x) return -1;
    if (!vol) return -2;
    if (!sigma2) return -3;
    if (!R) return -4;
    if (!X) return -5;
    if (!info) return -6;
    if (!workspace || ((uintptr_t)workspace & 255)) return -7;
    if (B < 1) return -8;
    if (N < 1) return -9;
    if (H < 1) return -10;
    const int64_t waves = ((int64_t)B * H + BM_T - 1) / BM_T;
    if (waves > 0x7fffffff) return -10;
    BmSolveParams<T> p{x, vol, sigma2, R, X, info, (double*)workspace, (double*)((char*)workspace + bm_inv_bytes(B, N)), B, N, H};
    hipLaunchKernelGGL((bm_factor_kernel<T>), dim3((unsigned)((B + BM_T - 1) / BM_T)), dim3(BM_T), 0, (hipStream_t)stream, p);
    VOLT_LAUNCH_CHECK();
    hipLaunchKernelGGL((bm_solve_kernel<T>), dim3((unsigned)waves), dim3(BM_T), 0, (hipStream_t)stream, p);
    VOLT_LAUNCH_CHECK();
    return 0;
}

}  // namespace volt

// 1/d_i of the last volt_bm_step_* (VOLT_WANT_GRAD) on this workspace: fp64, [N][B] series-fastest (host.h; gpcv_bm.hip reads it)
const double* volt_internal_bm_inv(const void* workspace) { return static_cast<const double*>(workspace); }

extern "C" {

size_t volt_bm_workspace_bytes(int B, int N, int H) {
    if (B < 1 || N < 1 || H < 1) return 0;
    return volt::bm_inv_bytes(B, N) + volt::al256((size_t)B * (size_t)N * (size_t)H * sizeof(double));
}

int volt_bm_step_f32(const float* x, const float* vol, const float* sigma2, const float* resid, float* out, float* alpha,
                     int* info, void* workspace, int B, int N, int flags, void* stream) {
    return volt::bm_step<float, false>(x, 0, vol, sigma2, resid, out, alpha, info, workspace, B, N, flags, stream);
}
int volt_bm_step_f64(const double* x, const double* vol, const double* sigma2, const double* resid, double* out, double* alpha,
                     int* info, void* workspace, int B, int N, int flags, void* stream) {
    return volt::bm_step<double, false>(x, 0, vol, sigma2, resid, out, alpha, info, workspace, B, N, flags, stream);
}
int volt_vk_step_f32(const float* V, int64_t bsv, const float* sigma2, const float* resid, float* out, float* alpha, int* info,
                     void* workspace, int B, int N, int flags, void* stream) {
    return volt::bm_step<float, true>(V, bsv, nullptr, sigma2, resid, out, alpha, info, workspace, B, N, flags, stream);
}
int volt_vk_step_f64(const double* V, int64_t bsv, const double* sigma2, const double* resid, double* out, double* alpha,
                     int* info, void* workspace, int B, int N, int flags, void* stream) {
    return volt::bm_step<double, true>(V, bsv, nullptr, sigma2, resid, out, alpha, info, workspace, B, N, flags, stream);
}
int volt_vk_forms_f32(const float* V, int64_t bsv, const double* jitter, const float* resid, double* out, int* info, int B,
                      int N, void* stream) {
    return volt::vk_forms<float>(V, bsv, jitter, resid, out, info, B, N, stream);
}
int volt_vk_forms_f64(const double* V, int64_t bsv, const double* jitter, const double* resid, double* out, int* info, int B,
                      int N, void* stream) {
    return volt::vk_forms<double>(V, bsv, jitter, resid, out, info, B, N, stream);
}
int volt_bm_post_f32(const float* x, int64_t bsx, const float* xs, const float* vol, const float* sigma2, const float* resid,
                     double* out, int* info, int B, int N, int H, void* stream) {
    return volt::bm_post<float>(x, bsx, xs, vol, sigma2, resid, out, info, B, N, H, stream);
}
int volt_bm_post_f64(const double* x, int64_t bsx, const double* xs, const double* vol, const double* sigma2, const double* resid,
                     double* out, int* info, int B, int N, int H, void* stream) {
    return volt::bm_post<double>(x, bsx, xs, vol, sigma2, resid, out, info, B, N, H, stream);
}
int volt_bm_solve_f32(const float* x, const float* vol, const float* sigma2, const float* R, float* X, int* info,
                      void* workspace, int B, int N, int H, void* stream) {
    return volt::bm_solve<float>(x, vol, sigma2, R, X, info, workspace, B, N, H, stream);
}
int volt_bm_solve_f64(const double* x, const double* vol, const double* sigma2, const double* R, double* X, int* info,
                      void* workspace, int B, int N, int H, void* stream) {
    return volt::bm_solve<double>(x, vol, sigma2, R, X, info, workspace, B, N, H, stream);
}

}  // extern "C"
