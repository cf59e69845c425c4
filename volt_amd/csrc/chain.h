// The recurrences of the linear-time chain family (bm.hip, gpcv_bm.hip, chain_draw.hip), each defined ONCE.
// Device code only, all __forceinline__, all fp64; the builtins and the FMA operands' order are compared bit for bit across versions.
#pragma once
#include <cstdint>

namespace volt {
constexpr double CHAIN_LN2 = 0.693147180559945309417232121458;
// 1 / d: v_rcp_f64 and two Newton steps (d is a positive normal number wherever info stays 0; else NaN / inf, reported there)
__device__ __forceinline__ double chain_rcp(double d) {
    double r = __builtin_amdgcn_rcp(d);
    double e = __builtin_fma(-d, r, 1.0);
    r = __builtin_fma(r, e, r);
    e = __builtin_fma(-d, r, 1.0);
    return __builtin_fma(r, e, r);
}
// 1 / sqrt(t): v_rsq_f64 and two Newton steps (the estimate's ~2^-26 becomes rounding level after the second) -- a library
// square root followed by a division is ~5 x the dependent instructions.  t <= 0, inf or NaN gives inf / NaN: a failed pivot.
__device__ __forceinline__ double chain_rsqrt(double t) {
    double y = __builtin_amdgcn_rsq(t);
    const double h = 0.5 * t;
    y = __builtin_fma(y, __builtin_fma(-h * y, y, 0.5), y);
    return __builtin_fma(y, __builtin_fma(-h * y, y, 0.5), y);
}
__device__ __forceinline__ bool chain_pivot_ok(double d) { return d > 0.0 && d < __builtin_inf(); }  // false for NaN
__device__ __forceinline__ int chain_fail_code(int64_t i) { return (int)(i + 1 < 0x7fffffff ? i + 1 : 0x7fffffff); }  // info of step i
// Everything below is a pure function of its arguments.  What a lane carries down a chain (1 / d_{i-1}, the mantissa product, the
// exponent sums) stays a plain scalar of the kernel, assigned there: a helper that updates one changes bm_step_kernel's registers.
// The pivots of T = v diag(delta) + s D D' = L diag(d) L' (bm.hip's header has the algebra): d_0 = v delta_0 + s, then
// c_i = s / d_{i-1}, d_i = v delta_i + 2 s - s c_i.  One FMA and one reciprocal on the serial chain.
struct ChainPivot { double d, c, inv; };   // d_i, c_i (0 at i = 0), 1 / d_i
struct ChainBm {
    double s, ss, s2;                      // per series: s, s^2, 2 s
    __device__ __forceinline__ explicit ChainBm(double s_) : s(s_), ss(s_ * s_), s2(2.0 * s_) {}
    __device__ __forceinline__ double base(double v, double delta, int64_t i) const { return __builtin_fma(v, delta, i == 0 ? s : s2); }
    // the pivot of the step whose base is v delta_i + (i == 0 ? s : 2 s), from the carried 1 / d_{i-1} (0 before the first)
    __device__ __forceinline__ ChainPivot pivot(double inv_prev, double base) const {
        const double d = __builtin_fma(-ss, inv_prev, base);
        return {d, s * inv_prev, chain_rcp(d)};
    }
};
// sum_i log d_i with ONE log: per step P = mul(P, d, on) (from 1), e += exp(d, on), e an int of the current tile (one that lives
// across tiles costs ~20 VGPRs); per tile -- at most 64 mantissas in [1/2, 1) later -- e += exp(P), P = mant(P), E += e (64-bit).
struct ChainLogDet {
    static __device__ __forceinline__ double mul(double P, double d, bool on) { return on ? P * __builtin_amdgcn_frexp_mant(d) : P; }
    static __device__ __forceinline__ int exp(double d, bool on = true) { return on ? __builtin_amdgcn_frexp_exp(d) : 0; }
    static __device__ __forceinline__ double mant(double P) { return __builtin_amdgcn_frexp_mant(P); }
    static __device__ __forceinline__ double value(double P, int64_t E) { return log(P) + (double)E * CHAIN_LN2; }
};

// forward   z_i = u_i + c_i z_{i-1}                    (u = D r, or any other differenced right-hand side)
__device__ __forceinline__ double chain_z_fwd(double c, double zprev, double u) { return __builtin_fma(c, zprev, u); }
// backward  w_i = z_i / d_i + rho_i w_{i+1},  rho_i = s / d_i
__device__ __forceinline__ double chain_z_back(double rho, double wnext, double z, double inv) { return __builtin_fma(rho, wnext, z * inv); }

// ---- the staged tile of the draw kernels (chain_draw.hip, markov_predict.hip): a wave moves rows [0, rows) x columns [0, cnt)
// between global memory (row r at src(r) / dst(r), unit stride) and tile[r][CH + 1] in LDS, V elements per global access
template <typename T, int V, int CH, typename RowPtr>
__device__ __forceinline__ void tile_load(T* tile, RowPtr src, int rows, int cnt, int lane) {
    typedef T vec_t __attribute__((ext_vector_type(V)));
    constexpr int NV = CH / V, LD = CH + 1;
    for (int idx = lane; idx < 64 * NV; idx += 64) {
        const int r = idx / NV, c = (idx % NV) * V;
        const T* s = src(r) + c;                     // (formed by every lane: a row pointer may come from a cross-lane read)
        if (r < rows && c < cnt) {
            if constexpr (V > 1) {
                const vec_t v = *reinterpret_cast<const vec_t*>(s);
#pragma unroll
                for (int u = 0; u < V; ++u) tile[r * LD + c + u] = v[u];
            } else {
                tile[r * LD + c] = *s;
            }
        }
    }
}
template <typename T, int V, int CH, typename RowPtr>
__device__ __forceinline__ void tile_store(const T* tile, RowPtr dst, int rows, int cnt, int lane) {
    typedef T vec_t __attribute__((ext_vector_type(V)));
    constexpr int NV = CH / V, LD = CH + 1;
    for (int idx = lane; idx < 64 * NV; idx += 64) {
        const int r = idx / NV, c = (idx % NV) * V;
        T* d = dst(r) + c;
        if (r < rows && c < cnt) {
            if constexpr (V > 1) {
                vec_t v;
#pragma unroll
                for (int u = 0; u < V; ++u) v[u] = tile[r * LD + c + u];
                *reinterpret_cast<vec_t*>(d) = v;
            } else {
                *d = tile[r * LD + c];
            }
        }
    }
}

}  // namespace volt
