// The device primitives of the Markov variational family (gpcv_markov.hip, gpcv_mt_markov.hip, markov_predict.hip; DESIGN
// 4.19): ONE affine scan, the fixed-order workgroup sum, the backward scan for s = diag P^-1, and the Brownian prior's
// increments.  The step, volt_markov_root_var_f32 and the prediction plan promise the same s bit for bit: they get it by
// calling markov_var_scan here at the same workgroup size, not by keeping three texts equal.
#pragma once
#include "common.h"

namespace volt {

struct Aff {                               // t -> a + b t
    double a, b;
};
// g after f
__device__ __forceinline__ Aff aff_then(const Aff& f, const Aff& g) { return Aff{__builtin_fma(g.b, f.a, g.a), g.b * f.b}; }

__device__ __forceinline__ double shfl_up_d(double v, int d) { return __shfl_up(v, d, 64); }
// the ASCENDING butterfly (offsets 1 .. 32); gpcv_mt.hip's task kernel sums with the descending one, which rounds differently
__device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) v += __shfl_xor(v, d, 64);
    return v;
}

// Keeps a wave-uniform value in vector registers.  A kernel's arguments, the per-series bases made from them and the fp64
// constants of exp / log do not fit the scalar register file side by side; what only the last phase needs waits here
// (an empty statement with a register constraint: it emits no instruction).
template <class V>
__device__ __forceinline__ void park_in_vgpr(V& v) {
    asm("" : "+v"(v));
}

// value_p = a_p + b_p value_{p-1}, p = 0 .. n-1, value_{-1} = 0.  coef(p, a, b) gives the map of position p, sink(p, value_p)
// takes the result; every thread of the workgroup (T threads, T / 64 waves) calls this with the same n.  A thread composes a
// contiguous run of R maps, a wave combines its 64 runs with cross-lane shuffles, the workgroup combines its waves through
// LDS in wave order, chunks of T * R points carry into each other in order: the order of every operation depends on
// (n, T, R) alone.  lds: 2 (T / 64) + 1 doubles.  A caller that runs backward in its own index passes i = n - 1 - p to its
// lambdas.
template <int T, int R = 4, class Coef, class Sink>
__device__ __forceinline__ void affine_scan(int64_t n, double* lds, Coef coef, Sink sink) {
    constexpr int W = T / 64;
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);   // (scalar: the loops over waves are scalar loops)
    constexpr int64_t CH = (int64_t)T * R;
    double carry = 0.0;
    for (int64_t c0 = 0; c0 < n; c0 += CH) {
        const int64_t p0 = c0 + (int64_t)tid * R;
        double a[R], b[R];
        Aff run{0.0, 1.0};
#pragma unroll
        for (int r = 0; r < R; ++r) {
            a[r] = 0.0;
            b[r] = 1.0;
            if (p0 + r < n) coef(p0 + r, a[r], b[r]);
            run = aff_then(run, Aff{a[r], b[r]});
        }
        // inclusive scan of the runs inside the wave
        Aff inc = run;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const Aff o{shfl_up_d(inc.a, d), shfl_up_d(inc.b, d)};
            if (lane >= d) inc = aff_then(o, inc);
        }
        if (lane == 63) {
            lds[2 * wave] = inc.a;
            lds[2 * wave + 1] = inc.b;
        }
        Aff exc{shfl_up_d(inc.a, 1), shfl_up_d(inc.b, 1)};
        if (lane == 0) exc = Aff{0.0, 1.0};
        __syncthreads();
        double v = carry;                                              // the value entering this wave, then this thread
#pragma unroll 1
        for (int w = 0; w < wave; ++w) v = __builtin_fma(lds[2 * w + 1], v, lds[2 * w]);
        double vend = v;                                               // ... and the one leaving the chunk
#pragma unroll 1
        for (int w = wave; w < W; ++w) vend = __builtin_fma(lds[2 * w + 1], vend, lds[2 * w]);
        v = __builtin_fma(exc.b, v, exc.a);
#pragma unroll
        for (int r = 0; r < R; ++r) {
            v = __builtin_fma(b[r], v, a[r]);
            if (p0 + r < n) sink(p0 + r, v);
        }
        carry = vend;
        __syncthreads();
    }
}

// sum over the workgroup in a fixed order: lanes by butterfly, waves in order.  lds: T / 64 doubles.  All threads get the sum.
template <int T>
__device__ __forceinline__ double block_sum_d(double v, double* lds) {
    v = wave_sum_d(v);
    if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = v;
    __syncthreads();
    double r = 0.0;
    for (int w = 0; w < T / 64; ++w) r += lds[w];
    __syncthreads();
    return r;
}

// The workgroup size of every kernel that promises the step's s: the scan's order, and with it the rounding, depends on it
constexpr int MARKOV_VAR_T = 512;

// s_i = diag P^-1 for one series into sb [N] (backward scan); eb [N] keeps e^{-2 rho_i}.  NULLABLE_E: eb may be null (then
// nothing is kept).  A compile-time choice because either form for everyone changes some caller's code: a caller that always
// has eb stores unconditionally.
template <int T, bool NULLABLE_E>
__device__ __forceinline__ void markov_var_scan(const float* __restrict__ rho, const float* __restrict__ gam, double* sb, double* eb,
                                                int64_t n, double* lds) {
    affine_scan<T>(
        n, lds,
        [&](int64_t p, double& a, double& b) {
            const int64_t i = n - 1 - p;
            a = exp(-2.0 * (double)rho[i]);
            if (!NULLABLE_E || eb) eb[i] = a;
            const double g = p > 0 ? (double)gam[i] : 0.0;             // gamma_{N-1} is never read
            b = g * g;
        },
        [&](int64_t p, double v) { sb[n - 1 - p] = v; });
}

// The level-jitter Brownian prior K_M = v min(x, x') + j 1 1' on the grid x: the grid step Delta_i and the increment
// variance q_0 = v x_0 + j, q_i = v (x_i - x_{i-1})
__device__ __forceinline__ double grid_step(const float* __restrict__ x, int64_t i) {
    return i == 0 ? (double)x[0] : (double)x[i] - (double)x[i - 1];
}
__device__ __forceinline__ double prior_inc(const float* __restrict__ x, double v, double jit, int64_t i) {
    return i == 0 ? __builtin_fma(v, (double)x[0], jit) : v * ((double)x[i] - (double)x[i - 1]);
}

}  // namespace volt
