// Joint draws from the two semiseparable-plus-diagonal covariances of the forecast in O(S H), without the H x H matrix
// (DESIGN 4.17): volt_markov_draw_* (the Markov posterior of the vol forecaster, posterior="chain") and volt_vk_draw_* (the
// predictive block W[min(s, t)] of the volatility-kernel data model, draw="chain"); and volt_markov_mix_f32, which carries the
// multitask model's T drawn eigen-directions to its tasks (at the end of the file).
//
// For a lower-triangular covariance with cov(i, i) = c_i and cov(i + 1, j) = g_i cov(i, j) for j <= i, plus a jitter j on the
// diagonal, row i of the Cholesky factor is (u_i l_0, .., u_i l_{i-1}, d_i) with a generator pair (u, l): L z is a running sum.
// With m_0 = s_0 = 0 (m_i = sum_{k<i} L_ik^2, s_i = sum_{k<i} L_ik z_k):
//     e_i = c_i - m_i,   d_i = sqrt(e_i + j)        (e_i + j not a positive finite number: info = i + 1)
//     y_i = mean_i + s_i + d_i z_i
//     m_{i+1} = g_i^2 (m_i + (e_i / d_i)^2),   s_{i+1} = g_i (s_i + (e_i / d_i) z_i)
// (L_{i+1,i} = g_i e_i / d_i: the jitter sits on the diagonal only, so the column below d_i carries e_i, not d_i^2.)  The
// factor is unique, so y = mean + chol(C + j I) z of the dense routes for the same z.  `chain_step` below is that recursion,
// in two halves: `chain_coef` (d_i, e_i / d_i and the next m: no z in it) and `chain_emit` (y_i and the next s).  The vk kernel
// runs both per lane (every path has its own c); the Markov kernel runs chain_coef ONCE per series and chain_emit per lane.
// All arithmetic fp64; z and the output carry the entry's type.
//
// Data movement (both kernels): the 64 paths of a wave own one contiguous 64 * H block of z / out.  It passes through LDS in
// chunks of CD_CH steps, one padded row (CD_CH + 1 elements: the per-step column read of 64 lanes is conflict-free) per path:
// the global side moves 16-byte groups along the rows (8 rows x 128 contiguous bytes per wave-instruction in fp32) whenever
// H is a multiple of the group and the pointers are 16-byte aligned, single elements along the rows (2 rows x 128 contiguous
// bytes) otherwise -- never a load per lane per step at stride H.  The draw overwrites its z in the tile and the tile goes
// back the same way.  No workspace, no atomics, one launch, fixed order of every sum: bitwise repeatable.
#include "common.h"
#include "chain.h"
#include "../../include/volt_hip.h"

namespace volt {

constexpr int CD_CH = 32;                 // steps per staged chunk
constexpr int CD_LD = CD_CH + 1;          // the padded row
constexpr int MD_WAVES = 8;               // Markov kernel: waves per workgroup ...
constexpr int MD_ROUNDS = 2;              // ... and tiles of 64 paths per wave: MD_PATHS paths of one series per workgroup
constexpr int MD_PATHS = MD_WAVES * MD_ROUNDS * 64;
constexpr int MD_FB = 8;                  // ... steps per group of the serial coefficient chain (divides CD_CH)

struct ChainCoef {
    double d, r;                          // d_i and e_i / d_i
};

// (c_i, m_i, jitter) -> (d_i, e_i / d_i); false where e_i + j is not a positive finite number (chain_rsqrt: chain.h; on the serial chain)
__device__ __forceinline__ bool chain_coef(double c, double m, double jit, ChainCoef& k) {
    const double e = c - m, t = e + jit;
    const double rs = chain_rsqrt(t);
    k.d = t * rs;
    k.r = e * rs;
    return t > 0.0 && t < __builtin_inf();
}
__device__ __forceinline__ double chain_next_m(double g, double m, const ChainCoef& k) { return g * g * (m + k.r * k.r); }
// y_i, and s_i -> s_{i+1}
__device__ __forceinline__ double chain_emit(double mean, double g, const ChainCoef& k, double z, double& s) {
    const double y = mean + s + k.d * z;
    s = g * (s + k.r * z);
    return y;
}
// the whole step for a path that owns its coefficients
__device__ __forceinline__ bool chain_step(double c, double g, double jit, double mean, double z, double& m, double& s, double& y) {
    ChainCoef k;
    const bool ok = chain_coef(c, m, jit, k);
    y = chain_emit(mean, g, k, z, s);
    m = chain_next_m(g, m, k);
    return ok;
}

// ------------------------------------------------------------------------------------------------ Markov posterior
template <typename T>
struct MarkovDrawParams {
    const double *mean, *diag, *off;      // [G,H]
    const T* z;                           // [G,S,H]
    const double* jitter;                 // [G]
    T* out;                               // [G,S,H]
    int* info;                            // [G]
    int64_t G, S, H;
    int flags;
};

// One workgroup per (series, MD_PATHS paths).  The coefficients (d_i, e_i / d_i, g_i) do not depend on z: per chunk of CD_CH
// steps the lanes form c_i, g_i and stage the mean, THREAD 0 runs chain_coef / chain_next_m down the chunk (the only serial
// part: one square root and one division per step and SERIES, m carried in its register from chunk to chunk), and every
// lane then reads them from LDS as broadcasts -- once per series whenever S <= MD_PATHS; a series with more paths is split
// over ceil(S / MD_PATHS) workgroups, each of which repeats the O(H) chain (same arithmetic, same result).  A lane keeps the
// running sum s of each of its MD_ROUNDS paths in LDS between chunks.  A failed pivot is the same in every workgroup of the
// series: each fills its own paths with NaN, the first one writes info.
template <typename T, int V>
__global__ __launch_bounds__(MD_WAVES * 64) void markov_draw_kernel(MarkovDrawParams<T> p) {
    extern __shared__ __attribute__((aligned(16))) char cd_smem[];
    double* __restrict__ cc = reinterpret_cast<double*>(cd_smem);   // [CD_CH] c_i      (in: written by the lanes)
    double* __restrict__ cg = cc + CD_CH;                   // [CD_CH] g_i
    double* __restrict__ cm = cg + CD_CH;                   // [CD_CH] mean_i
    double* __restrict__ cd = cm + CD_CH;                   // [CD_CH] d_i      (out: written by thread 0)
    double* __restrict__ cr = cd + CD_CH;                   // [CD_CH] e_i / d_i
    double* st = cr + CD_CH;                                // [MD_ROUNDS][MD_WAVES * 64] s of every path
    int* fail = reinterpret_cast<int*>(st + MD_ROUNDS * MD_WAVES * 64);
    T* tiles = reinterpret_cast<T*>(fail + 4);              // [MD_WAVES][64][CD_LD]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t g = blockIdx.x, H = p.H, S = p.S;
    const int64_t s0 = (int64_t)blockIdx.y * MD_PATHS;
    const double* mean = p.mean + g * H;
    const double* diag = p.diag + g * H;
    const double* off = p.off + g * H;
    const T* zg = p.z + g * S * H;
    T* og = p.out + g * S * H;
    const double jit = p.jitter[g];
    const bool want_exp = (p.flags & VOLT_DRAW_EXP) != 0;
    T* tile = tiles + wave * 64 * CD_LD;
    for (int rd = 0; rd < MD_ROUNDS; ++rd) st[rd * MD_WAVES * 64 + tid] = 0.0;
    if (tid == 0) *fail = 0;
    double m = 0.0;                                         // (thread 0's is the chain's)
    int failed = 0;
    for (int64_t c0 = 0; c0 < H; c0 += CD_CH) {
        const int cnt = (int)(H - c0 < CD_CH ? H - c0 : CD_CH);
        if (tid < cnt) {
            const int64_t i = c0 + tid;
            const double dg = diag[i];
            double gi = 0.0;
            if (i + 1 < H && dg > 0.0) {                    // g_i = off_i / diag_i, 0 where diag_i <= 0 (gp._markov_cov); the last off is not read
                gi = off[i] / dg;
                gi = gi < 0.0 ? 0.0 : gi;                   // (a NaN stays a NaN)
            }
            cc[tid] = dg < 0.0 ? 0.0 : dg;
            cg[tid] = gi;
            cm[tid] = mean[i];
        }
        __syncthreads();
        if (tid == 0) {
            // groups of MD_FB steps: their inputs are read first (the arrays thread 0 writes are not the ones it reads), so
            // the LDS round trips overlap and only the arithmetic is serial.  A failed pivot is recorded once; the steps
            // behind it run on NaNs that nobody reads.
            int bad = 0;
            for (int i0 = 0; i0 < cnt; i0 += MD_FB) {
                double ci[MD_FB], gi[MD_FB];
                ChainCoef k[MD_FB];
#pragma unroll
                for (int u = 0; u < MD_FB; ++u) ci[u] = cc[i0 + u], gi[u] = cg[i0 + u];
#pragma unroll
                for (int u = 0; u < MD_FB; ++u) {
                    const bool ok = chain_coef(ci[u], m, jit, k[u]);
                    if (!ok && bad == 0 && i0 + u < cnt) bad = chain_fail_code(c0 + i0 + u);
                    m = chain_next_m(gi[u], m, k[u]);
                }
#pragma unroll
                for (int u = 0; u < MD_FB; ++u) cd[i0 + u] = k[u].d, cr[i0 + u] = k[u].r;
            }
            if (bad) *fail = bad;
        }
        __syncthreads();
        failed = *fail;
        if (failed) break;                                  // (uniform)
        for (int rd = 0; rd < MD_ROUNDS; ++rd) {
            const int64_t pb = s0 + (int64_t)(rd * MD_WAVES + wave) * 64;
            const int rows = (int)(S - pb < 64 ? (S - pb < 0 ? 0 : S - pb) : 64);
            tile_load<T, V, CD_CH>(tile, [&](int r) { return zg + (pb + r) * H + c0; }, rows, cnt, lane);
            __syncthreads();
            if (lane < rows) {
                double s = st[rd * MD_WAVES * 64 + tid];
                for (int i = 0; i < cnt; ++i) {
                    const ChainCoef k = {cd[i], cr[i]};
                    double y = chain_emit(cm[i], cg[i], k, (double)tile[lane * CD_LD + i], s);
                    if (want_exp) y = exp(y);
                    tile[lane * CD_LD + i] = (T)y;
                }
                st[rd * MD_WAVES * 64 + tid] = s;
            }
            __syncthreads();
            tile_store<T, V, CD_CH>(tile, [&](int r) { return og + (pb + r) * H + c0; }, rows, cnt, lane);
            __syncthreads();
        }
    }
    if (failed) {
        // the chunks before the failed pivot are out already: every store of this workgroup has to land before the NaNs
        __threadfence();
        __syncthreads();
        const int64_t nrows = S - s0 < MD_PATHS ? S - s0 : MD_PATHS;
        T* o = og + s0 * H;
        const T nan = (T)__builtin_nan("");
        for (int64_t i = tid; i < nrows * H; i += MD_WAVES * 64) o[i] = nan;
    }
    if (blockIdx.y == 0 && tid == 0) p.info[g] = failed;
}

// ------------------------------------------------------------------------------------------------ volatility-kernel block
template <typename T>
struct VkDrawParams {
    const T* pred_vol;                    // [G,S,H]
    const double *vol_last, *vlr, *dx;    // [G]: the last train vol, V_last - rho, the grid step
    const double* mean;                   // [G,H]
    const T* z;                           // [G,S*reps,H]
    const double* jitter;                 // [G]
    T* out;                               // [G,S*reps,H]
    int* info;                            // [G,S]
    int64_t G, S, H, reps;
};

// One wave per 64 consecutive paths of the flattened [G, S * reps] batch (a wave may straddle two series: every per-series
// number is read per lane).  c_h = W_h = (V_te,h - V_last) + (V_last - rho) is formed on the fly: the stacked integrated path
// of rollout_utils.py:17-26 past the last train point is the CumTrapz of [vol_last, pred_vol] over a uniform grid -- weights
// dx / 2 on the first and the last of its H + 1 points, dx between, each product w * (y * y) rounded on its own and added to
// an fp64 running sum, as csrc/fill.hip does for ops.cumtrapz(..., square=True) -- less its first entry (forecast.
// _standard_mean_prediction_linear: tail[..., 1:] - tail[..., :1]).  g = 1.  A path whose pivot fails writes NaN from that
// step on and rewrites its earlier steps with NaN at the end; `reps` consecutive paths share a pred_vol row and therefore a
// pivot chain and an info word, written by the first of them.
template <typename T, int V>
__global__ __launch_bounds__(64) void vk_draw_kernel(VkDrawParams<T> p) {
#pragma clang fp contract(off)
    __shared__ __attribute__((aligned(16))) T tz[64 * CD_LD];
    __shared__ __attribute__((aligned(16))) T tv[64 * CD_LD];
    __shared__ double tm[CD_CH];                             // the chunk's mean, when the wave lies inside one series
    const int lane = threadIdx.x;
    const int64_t H = p.H, SR = p.S * p.reps, P = p.G * SR;
    const int64_t p0 = (int64_t)blockIdx.x * 64;
    const int rows = (int)(P - p0 < 64 ? P - p0 : 64);
    const bool act = lane < rows;
    const int64_t path = act ? p0 + lane : P - 1;          // (idle lanes shadow the last path: every load is valid, nothing is stored)
    const int64_t g = path / SR;
    const int64_t vrow = path / p.reps;                     // this path's row of pred_vol, in [0, G * S)
    const int64_t vrow0 = p0 / p.reps;
    const int vrel = (int)(vrow - vrow0);                   // < 64: handed to the lane that loads the row
    const double vl = p.vol_last[g], vlr = p.vlr[g], dx = p.dx[g], hdx = dx * 0.5, jit = p.jitter[g];
    const double* mean = p.mean + g * H;
    const bool one_series = p0 / SR == (p0 + rows - 1) / SR;    // (wave-uniform)
    const double run0 = hdx * (vl * vl);                    // tail[0]
    double run = run0, m = 0.0, s = 0.0;
    int bad = 0;
    const T nan = (T)__builtin_nan("");
    for (int64_t c0 = 0; c0 < H; c0 += CD_CH) {
        const int cnt = (int)(H - c0 < CD_CH ? H - c0 : CD_CH);
        tile_load<T, V, CD_CH>(tz, [&](int r) { return p.z + (p0 + r) * H + c0; }, rows, cnt, lane);
        tile_load<T, V, CD_CH>(tv, [&](int r) { return p.pred_vol + (vrow0 + __shfl(vrel, r)) * H + c0; }, 64, cnt, lane);
        if (one_series && lane < cnt) tm[lane] = mean[c0 + lane];
        double mu_next = one_series ? 0.0 : mean[c0];       // a wave across series: each lane's own mean, requested a step ahead
        __syncthreads();
        for (int i = 0; i < cnt; ++i) {
            const double mu = one_series ? tm[i] : mu_next;
            if (!one_series && i + 1 < cnt) mu_next = mean[c0 + i + 1];
            const double v = (double)tv[lane * CD_LD + i];
            const double w = (c0 + i == H - 1) ? hdx : dx;
            run += w * (v * v);
            const double W = (run - run0) + vlr;
            double y;
            const bool ok = chain_step(W, 1.0, jit, mu, (double)tz[lane * CD_LD + i], m, s, y);
            if (!ok && bad == 0) bad = chain_fail_code(c0 + i);
            tz[lane * CD_LD + i] = bad ? nan : (T)y;
        }
        __syncthreads();
        tile_store<T, V, CD_CH>(tz, [&](int r) { return p.out + (p0 + r) * H + c0; }, rows, cnt, lane);
        __syncthreads();
    }
    if (__any(act && bad > 1)) {
        __threadfence();                                    // the tiles' stores land before the NaNs that replace them
        if (act && bad > 1) {
            T* o = p.out + path * H;
            for (int64_t i = 0; i < bad - 1; ++i) o[i] = nan;
        }
    }
    if (act && path % p.reps == 0) p.info[vrow] = bad;
}

template <typename T>
static bool cd_aligned(int64_t H, const void* a, const void* b, const void* c) {
    constexpr int V = 16 / sizeof(T);
    return H % V == 0 && (uintptr_t)a % 16 == 0 && (uintptr_t)b % 16 == 0 && (c == nullptr || (uintptr_t)c % 16 == 0);
}

template <typename T>
static int launch_markov_draw(const double* mean, const double* diag, const double* off, const T* z, const double* jitter,
                              T* out, int* info, int G, int S, int H, int flags, void* stream) {
    if (!mean) return -1;
    if (!diag) return -2;
    if (!off) return -3;
    if (!z) return -4;
    if (!jitter) return -5;
    if (!out) return -6;
    if (!info) return -7;
    if (G < 1) return -8;
    if (S < 1 || ((int64_t)S + MD_PATHS - 1) / MD_PATHS > 65535) return -9;
    if (H < 1) return -10;
    if (flags & ~VOLT_DRAW_EXP) return -11;
    MarkovDrawParams<T> p = {mean, diag, off, z, jitter, out, info, G, S, H, flags};
    const size_t lds = (5 * CD_CH + MD_ROUNDS * MD_WAVES * 64) * sizeof(double) + 16 + (size_t)MD_WAVES * 64 * CD_LD * sizeof(T);
    const dim3 grid(G, (unsigned)(((int64_t)S + MD_PATHS - 1) / MD_PATHS));
    constexpr int V = 16 / sizeof(T);
#define VOLT_MD_LAUNCH(VV)                                                                                             \
    do {                                                                                                               \
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(markov_draw_kernel<T, VV>),                   \
                                           hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);                     \
        if (e != hipSuccess) return (int)e;                                                                            \
        hipLaunchKernelGGL((markov_draw_kernel<T, VV>), grid, dim3(MD_WAVES * 64), lds, (hipStream_t)stream, p);       \
    } while (0)
    if (cd_aligned<T>(H, z, out, nullptr)) VOLT_MD_LAUNCH(V);
    else VOLT_MD_LAUNCH(1);
#undef VOLT_MD_LAUNCH
    VOLT_LAUNCH_CHECK();
    return 0;
}

template <typename T>
static int launch_vk_draw(const T* pred_vol, const double* vol_last, const double* vlr, const double* dx, const double* mean,
                          const T* z, const double* jitter, T* out, int* info, int G, int S, int H, int reps, void* stream) {
    if (!pred_vol) return -1;
    if (!vol_last) return -2;
    if (!vlr) return -3;
    if (!dx) return -4;
    if (!mean) return -5;
    if (!z) return -6;
    if (!jitter) return -7;
    if (!out) return -8;
    if (!info) return -9;
    if (G < 1) return -10;
    if (S < 1) return -11;
    if (H < 1) return -12;
    if (reps < 1) return -13;
    const int64_t P = (int64_t)G * S * reps;
    if ((P + 63) / 64 > 0x7fffffff) return -13;
    VkDrawParams<T> p = {pred_vol, vol_last, vlr, dx, mean, z, jitter, out, info, G, S, H, reps};
    const dim3 grid((unsigned)((P + 63) / 64));
    constexpr int V = 16 / sizeof(T);
    if (cd_aligned<T>(H, z, out, pred_vol))
        hipLaunchKernelGGL((vk_draw_kernel<T, V>), grid, dim3(64), 0, (hipStream_t)stream, p);
    else
        hipLaunchKernelGGL((vk_draw_kernel<T, 1>), grid, dim3(64), 0, (hipStream_t)stream, p);
    VOLT_LAUNCH_CHECK();
    return 0;
}

// ------------------------------------------------------------------------------------------------ the multitask mix
// out[s,h,t] = mean[h,t] + sum_j V[t,j] lz[j,s,h]: the draws L_j z_j of the T eigen-directions (volt_markov_draw_f64, G = T) carried
// to the tasks, V = D^1/2 Q.  The sum runs in fp64 in the fixed order j = 0 .. T-1 and the result is rounded ONCE: the fp32 GEMM of
// the dense route rounds L z first and accumulates T terms of either sign in fp32, which shows where they cancel.  One
// workgroup per MX_P points (s, h): V (transposed, so that the lanes' consecutive tasks read consecutive words) and the
// points' T x MX_P block of lz are staged in LDS with coalesced loads, and a thread forms one output at a time, the task
// fastest -- the block's MX_P x T outputs are contiguous in `out`.
constexpr int MX_P = 64;                  // points per workgroup
constexpr int MX_T = 64;                  // tasks at most (the Kronecker path's own limit): T * (T + MX_P) doubles of LDS
__global__ __launch_bounds__(256) void markov_mix_kernel(const double* __restrict__ lz, const double* __restrict__ V,
                                                         const float* __restrict__ mean, float* __restrict__ out, int T,
                                                         int64_t SN, int64_t n) {
    extern __shared__ __attribute__((aligned(16))) double mx_smem[];
    double* Vt = mx_smem;                                    // [T][T]: Vt[j * T + t] = V[t, j]
    double* lzs = mx_smem + T * T;                           // [T][MX_P]
    const int tid = threadIdx.x;
    const int64_t sh0 = (int64_t)blockIdx.x * MX_P;
    const int np = (int)(SN - sh0 < MX_P ? SN - sh0 : MX_P);
    for (int k = tid; k < T * T; k += 256) {
        const int t = k / T, j = k - t * T;
        Vt[j * T + t] = V[k];
    }
    for (int k = tid; k < T * MX_P; k += 256) {
        const int j = k / MX_P, pp = k - j * MX_P;
        lzs[k] = pp < np ? lz[(int64_t)j * SN + sh0 + pp] : 0.0;
    }
    __syncthreads();
    for (int k = tid; k < np * T; k += 256) {
        const int pp = k / T, t = k - pp * T;
        double acc = 0.0;
        for (int j = 0; j < T; ++j) acc = __builtin_fma(Vt[j * T + t], lzs[j * MX_P + pp], acc);
        const int64_t h = (sh0 + pp) % n;
        out[sh0 * T + k] = (float)((double)mean[h * T + t] + acc);
    }
}

static int launch_markov_mix(const double* lz, const double* V, const float* mean, float* out, int T, int S, int n, void* stream) {
    if (!lz) return -1;
    if (!V) return -2;
    if (!mean) return -3;
    if (!out) return -4;
    if (T < 1 || T > MX_T) return -5;
    if (S < 1) return -6;
    if (n < 1) return -7;
    const int64_t SN = (int64_t)S * n;
    if ((SN + MX_P - 1) / MX_P > 0x7fffffff) return -6;
    const size_t lds = (size_t)T * (T + MX_P) * sizeof(double);
    if (lds > 48 * 1024) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(markov_mix_kernel),
                                           hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return (int)e;
    }
    hipLaunchKernelGGL(markov_mix_kernel, dim3((unsigned)((SN + MX_P - 1) / MX_P)), dim3(256), lds, (hipStream_t)stream, lz, V,
                       mean, out, T, SN, (int64_t)n);
    VOLT_LAUNCH_CHECK();
    return 0;
}

}  // namespace volt

extern "C" {

int volt_markov_mix_f32(const double* lz, const double* V, const float* mean, float* out, int T, int S, int n, void* stream) {
    return volt::launch_markov_mix(lz, V, mean, out, T, S, n, stream);
}

int volt_markov_draw_f32(const double* mean, const double* diag, const double* off, const float* z, const double* jitter,
                         float* out, int* info, int G, int S, int H, int flags, void* stream) {
    return volt::launch_markov_draw<float>(mean, diag, off, z, jitter, out, info, G, S, H, flags, stream);
}
int volt_markov_draw_f64(const double* mean, const double* diag, const double* off, const double* z, const double* jitter,
                         double* out, int* info, int G, int S, int H, int flags, void* stream) {
    return volt::launch_markov_draw<double>(mean, diag, off, z, jitter, out, info, G, S, H, flags, stream);
}
int volt_vk_draw_f32(const float* pred_vol, const double* vol_last, const double* vlr, const double* dx, const double* mean,
                     const float* z, const double* jitter, float* out, int* info, int G, int S, int H, int reps, void* stream) {
    return volt::launch_vk_draw<float>(pred_vol, vol_last, vlr, dx, mean, z, jitter, out, info, G, S, H, reps, stream);
}
int volt_vk_draw_f64(const double* pred_vol, const double* vol_last, const double* vlr, const double* dx, const double* mean,
                     const double* z, const double* jitter, double* out, int* info, int G, int S, int H, int reps, void* stream) {
    return volt::launch_vk_draw<double>(pred_vol, vol_last, vlr, dx, mean, z, jitter, out, info, G, S, H, reps, stream);
}

}  // extern "C"
