// The Markov GPCV away from its grid: mean, variance and joint path draws of f at H test points in O(N + S H)
// (SingleTaskVariationalGP / MultitaskVariationalGP(prior_solver="markov")(x)).
//
// Notation of gpcv_markov.hip: grid 0 <= x_0 < .. < x_{N-1}; prior f - mu Brownian motion with K_M = v min(x, x') + j 1 1';
// family q(u) = N(m, P^-1), P = Lp Lp', Lp with diagonal e^{rho_i} and (i+1, i) entry gamma_i e^{rho_i};
// s_i = e^{-2 rho_i} + gamma_i^2 s_{i+1} = diag P^-1.  The family's backward recursion
//     u_i - m_i = -gamma_i (u_{i+1} - m_{i+1}) + e^{-rho_i} eps_i
// gives for knots a < b   cov(u_a, u_b) = Phi_{a,b} s_b,  Phi_{a,b} = prod_{l=a}^{b-1} (-gamma_l),   and the innovation
// variance of u_a given u_b   r_{a,b} = sum_{l=a}^{b-1} (prod_{t=a}^{l-1} gamma_t^2) e^{-2 rho_l}   (positive terms only: it
// is s_a - Phi^2 s_b without the cancellation).  Given u, f(xi) is a Brownian bridge between the neighbouring knots, free
// Brownian motion beyond x_{N-1}, and a bridge from the anchor (x_{-1} = -j / v, level mu, variance 0: where the prior
// variance v x + j vanishes) before x_0.  With i = #{x_k <= xi} - 1 and w = (xi - x_i) / (x_{i+1} - x_i):
//     i = N-1:  mean m_{N-1}                  var_q s_{N-1}                                  var_p v (xi - x_{N-1})
//     else:     mean (1-w) m_i + w m_{i+1}    var_q (1-w)^2 s_i + w^2 s_{i+1} - 2 w (1-w) gamma_i s_{i+1}
//                                             var_p v (xi - x_i) (x_{i+1} - xi) / (x_{i+1} - x_i)
// (i = -1: x_i, m_i, s_i := x_{-1}, mu, 0 and the cross term is absent).  var_q is the q part A P^-1 A', var_p the bridge part
// K** - A K_uu A': they are kept apart because the multi-task model scales them by different task matrices.
//
// markov_predict_plan_kernel: one workgroup per series.  It locates every xi_h by binary search (validating the list), runs
// three backward scans over N -- s (the step's own scan at the step's workgroup size: bit for bit volt_markov_root_var_f32's),
// and Phi and r SEGMENTED at the selected knots (the ends of every interval that holds a test point, and N-1): the map of a
// knot whose right neighbour is selected starts afresh, so Phi_a, r_a run from a to the next selected knot above it -- and
// writes the per-point forms and the DRAW PLAN: a list of E <= 3 H + 1 steps over four numbers of state per path,
//     R  the deviation u - m of the knot the chain has reached,    L  that of the open interval's left knot,
//     Ak, Ab  the chain part and the bridge part of the point drawn last (the open interval's right anchor),
// in ONE pass over the test points in DESCENDING xi (step e consumes base sample e):
//     KNOT   R = a R + c eps                                   (step 0: a = 0, c = sqrt(s_{N-1}); else (Phi, sqrt r) down to the
//                                                               right knot of the next interval that holds points)
//     OPEN   L = a R + c eps,  Ak = R,  Ab = 0                  ((Phi, sqrt r) of one grid step; before x_0: a = c = 0; beyond
//                                                               x_{N-1} the interval has no right knot and its left knot
//                                                               is the chain's: a = 1, c = 0)
//     POINT  Ak = a L + b Ak,  Ab = b Ab + c eps,  f_h = mean_h + Ak + Ab        (a, b = 1 - w, w of the bridge between the left
//                                                               knot and the anchor to the right, c^2 its variance; a point
//                                                               ON its anchor copies it: a, b, c = 0, 1, 0 -- duplicates, and
//                                                               a duplicate on a knot, which would be 0 / 0; the farthest
//                                                               point beyond the grid has no anchor: 1, 0, sqrt(v (xi - x_{N-1})))
//     CLOSE  a POINT, then R = L                                (the interval's last point: the chain moves to the left knot)
// Beyond the grid the points are therefore drawn from the farthest inward, each a bridge between u_{N-1} and the point drawn
// before it: the same joint law as independent increments outward, and one direction of travel for the whole list.  The
// position of a point's steps in the list is a prefix sum over the points, which runs through the same affine_scan (b = 1).
// KNOT and OPEN carry the CHAIN noise (together A P^-1 A'), POINT the BRIDGE noise (K** - A K_uu A').
//
// markov_predict_draw_kernel: one lane per path, one wave per 64 paths of one series.  The plan is wave-uniform and read as
// such; the wave's 64 x E block of eps and its 64 x H block of out pass through LDS in chunks of MP_CH columns with padded
// rows (chain_draw.hip's data movement, chain.h's tile_load / tile_store: the global side moves along the rows, never a lane
// per step at stride H or E).
//
// affine_scan and markov_var_scan are markov_scan.h's, the staged tile chain.h's.  fp64 arithmetic, fp32 I/O; no atomics, no
// scratch; the order of every operation depends on (N, H) alone: bitwise repeatable.
#include "common.h"
#include "host.h"
#include "chain.h"
#include "markov_scan.h"
#include "../../include/volt_hip.h"

namespace volt {
namespace mpr {

constexpr int MP_T = MARKOV_VAR_T;         // threads of the plan's workgroup: the step's, so that markov_var_scan gives the step's s
constexpr int MP_W = MP_T / 64;
constexpr int MP_CH = 32;                  // columns per staged chunk of the draw
constexpr int MP_LD = MP_CH + 1;           // the padded row
constexpr int MP_HMAX = 1 << 24;           // test points at most (a step's code is 8 h + op in an int)

enum { OP_NOP = 0, OP_KNOT = 1, OP_OPEN = 2, OP_POINT = 3, OP_CLOSE = 4 };

// the smallest value over the workgroup (every thread gets it).  red: MP_W ints
__device__ __forceinline__ int block_min_i(int v, int* red) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int o = __shfl_xor(v, d, 64);
        v = o < v ? o : v;
    }
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    int r = red[0];
    for (int w = 1; w < MP_W; ++w) r = red[w] < r ? red[w] : r;
    __syncthreads();
    return r;
}

struct PlanParams {
    const float *x, *xs;                   // [N], [H] ascending: shared by the series
    const float *vol, *mu;                 // [B]
    const float *m, *rho, *gam;            // [B,N]
    double jit;
    double *mean, *var_q, *var_p;          // [B,H]
    double* coef;                          // [B,3H+1,3] (a, b, c) of every step
    int* code;                             // [B,3H+1]   8 h + op
    int *steps, *info;                     // [B]
    double *ws_s, *ws_phi, *ws_r;          // [B,N]
    int* ws_idx;                           // [B,H]
    int N, H;
};

__global__ __launch_bounds__(MP_T) void markov_predict_plan_kernel(PlanParams p) {
    __shared__ double lds[2 * MP_W + 1];
    __shared__ int red[MP_W];
    const int tid = threadIdx.x;
    const int64_t n = p.N, H = p.H, b = blockIdx.x, EM = 3 * H + 1;
    const float* __restrict__ x = p.x;
    const float* __restrict__ xs = p.xs;
    const float *rb = p.rho + b * n, *gb = p.gam + b * n, *mb = p.m + b * n;
    double *sb = p.ws_s + b * n, *fb = p.ws_phi + b * n, *qb = p.ws_r + b * n;
    int* ib = p.ws_idx + b * H;
    double *mean = p.mean + b * H, *vq = p.var_q + b * H, *vp = p.var_p + b * H, *coef = p.coef + b * EM * 3;
    int* code = p.code + b * EM;
    int *steps = p.steps + b, *info = p.info + b;
    park_in_vgpr(mean), park_in_vgpr(vq), park_in_vgpr(vp), park_in_vgpr(coef), park_in_vgpr(code), park_in_vgpr(steps);
    park_in_vgpr(info), park_in_vgpr(mb), park_in_vgpr(fb);
    const double v = (double)p.vol[b], mu = (double)p.mu[b];
    const double xa = -p.jit / v;                                      // x_{-1}

    // ---- 1. locate: idx_h = #{x_k <= xi_h} - 1 in [-1, N-1]; the first test point that is NaN, infinite, negative or out of order
    int bad = 0x7fffffff;
    for (int64_t h = tid; h < H; h += MP_T) {
        const float t = xs[h];
        const bool ok = t >= 0.f && t < __builtin_inff() && (h == 0 || t >= xs[h - 1]);
        if (!ok && h < bad) bad = (int)h;
        int64_t lo = 0, hi = n;                                        // the first k with x_k > t
        while (lo < hi) {
            const int64_t mid = (lo + hi) >> 1;
            if (x[mid] <= t) lo = mid + 1;
            else hi = mid;
        }
        ib[h] = (int)lo - 1;
    }
    bad = block_min_i(bad, red);                                       // (its barrier: idx is visible to the workgroup)
    if (bad != 0x7fffffff) {                                           // (uniform)
        const double nan = __builtin_nan("");
        for (int64_t h = tid; h < H; h += MP_T) mean[h] = vq[h] = vp[h] = nan;
        for (int64_t e = tid; e < EM; e += MP_T) {
            coef[3 * e] = coef[3 * e + 1] = coef[3 * e + 2] = nan;
            code[e] = OP_NOP;
        }
        if (tid == 0) {
            *steps = 0;
            *info = -(bad + 1);
        }
        return;
    }

    // ---- 2. s, and Phi, r segmented at the selected knots.  Knot k is selected iff k = N-1 or some idx is k-1 or k
    markov_var_scan<MP_T, false>(rb, gb, sb, qb, n, lds);                     // (qb holds e^{-2 rho} until the r scan replaces it)
    auto right_selected = [&](int64_t i) -> bool {                     // is knot i + 1 selected
        if (i + 1 == n - 1) return true;
        int64_t lo = 0, hi = H;                                        // the first h with idx_h >= i
        while (lo < hi) {
            const int64_t mid = (lo + hi) >> 1;
            if (ib[mid] < i) lo = mid + 1;
            else hi = mid;
        }
        return lo < H && ib[lo] <= i + 1;
    };
    affine_scan<MP_T>(
        n, lds,
        [&](int64_t q, double& a, double& bb) {
            const int64_t i = n - 1 - q;
            const double g = q > 0 ? -(double)gb[i] : 0.0;
            const bool fresh = q == 0 || right_selected(i);
            a = fresh ? g : 0.0;
            bb = fresh ? 0.0 : g;
        },
        [&](int64_t q, double val) { fb[n - 1 - q] = val; });
    affine_scan<MP_T>(
        n, lds,
        [&](int64_t q, double& a, double& bb) {
            const int64_t i = n - 1 - q;
            const double g = q > 0 ? (double)gb[i] : 0.0;
            a = qb[i];
            bb = (q == 0 || right_selected(i)) ? 0.0 : g * g;
        },
        [&](int64_t q, double val) { qb[n - 1 - q] = val; });
    __syncthreads();

    // ---- 3. the per-point forms and the plan.  Point h (taken in descending h) owns 1 step, + 1 (OPEN) where it is the first
    // of its interval, + 1 (KNOT) where the chain has to travel to that interval's right knot first
    int notfinite = 0;
    auto shape = [&](int64_t h, bool& first, bool& knot) {
        const int i = ib[h];
        first = h == H - 1 || ib[h + 1] != i;
        const int64_t kb = h == H - 1 ? n - 1 : ib[h + 1];             // where the chain stands when the interval opens
        knot = first && i + 1 < kb;
    };
    auto put = [&](int64_t e, int op, int64_t h, double a, double bb, double c) {
        coef[3 * e] = a;
        coef[3 * e + 1] = bb;
        coef[3 * e + 2] = c;
        code[e] = (int)(h * 8 + op);
    };
    affine_scan<MP_T>(
        H, lds,
        [&](int64_t q, double& a, double& bb) {
            bool first, knot;
            shape(H - 1 - q, first, knot);
            a = 1.0 + (first ? 1.0 : 0.0) + (knot ? 1.0 : 0.0);
            bb = 1.0;
        },
        [&](int64_t q, double total) {
            const int64_t h = H - 1 - q;
            bool first, knot;
            shape(h, first, knot);
            const int64_t i = ib[h];
            const int cnt = 1 + (first ? 1 : 0) + (knot ? 1 : 0);
            int64_t e = (int64_t)total - cnt + 1;                      // (+ 1: step 0 draws u_{N-1})
            if (q == 0) put(0, OP_KNOT, 0, 0.0, 0.0, sqrt(sb[n - 1]));
            if (h == 0) *steps = (int)(total + 1.0);
            const double t = (double)xs[h];
            const double xl = i >= 0 ? (double)x[i] : xa;
            if (knot) put(e++, OP_KNOT, h, fb[i + 1], 0.0, sqrt(qb[i + 1]));
            if (first) {
                if (i == n - 1) put(e++, OP_OPEN, h, 1.0, 0.0, 0.0);
                else if (i >= 0) put(e++, OP_OPEN, h, fb[i], 0.0, sqrt(qb[i]));
                else put(e++, OP_OPEN, h, 0.0, 0.0, 0.0);
            }
            // the bridge between the left knot and the anchor to the right: the point drawn before, else the right knot
            const bool anchored = !first || i < n - 1;
            const double ax = !first ? (double)xs[h + 1] : (i < n - 1 ? (double)x[i + 1] : 0.0);
            double a = 1.0, bb = 0.0, c2 = v * (t - xl);
            if (anchored) {
                if (t >= ax) {
                    a = 0.0, bb = 1.0, c2 = 0.0;
                } else {
                    const double w = (t - xl) / (ax - xl);
                    a = 1.0 - w, bb = w, c2 = v * (t - xl) * (ax - t) / (ax - xl);
                }
            }
            const bool last = h == 0 || ib[h - 1] != i;
            put(e, last ? OP_CLOSE : OP_POINT, h, a, bb, sqrt(c2 > 0.0 ? c2 : (c2 == c2 ? 0.0 : c2)));
            // the forms
            double mh, q_, p_;
            if (i == n - 1) {
                mh = (double)mb[i], q_ = sb[i], p_ = v * (t - xl);
            } else {
                const double xr = (double)x[i + 1], w = (t - xl) / (xr - xl), u = 1.0 - w;
                const double ml = i >= 0 ? (double)mb[i] : mu, sl = i >= 0 ? sb[i] : 0.0, sr = sb[i + 1];
                const double cross = i >= 0 ? 2.0 * w * u * (double)gb[i] * sr : 0.0;
                mh = u * ml + w * (double)mb[i + 1];
                q_ = u * u * sl + w * w * sr - cross;
                p_ = v * (t - xl) * (xr - t) / (xr - xl);
            }
            mean[h] = mh, vq[h] = q_, vp[h] = p_;
            const double tot = q_ + p_;
            if (!(tot - tot == 0.0)) notfinite = 1;
        });
    if (tid == 0 && !(sb[0] - sb[0] == 0.0)) notfinite = 1;            // a NaN below every selected knot reaches no output: reported all the same
    notfinite = -block_min_i(-notfinite, red);                         // (its barrier: steps[b] is visible)
    const int64_t E = *steps;
    for (int64_t e = E + tid; e < EM; e += MP_T) put(e, OP_NOP, 0, 0.0, 0.0, 0.0);
    if (tid == 0) *info = notfinite;
}

struct DrawParams {
    const double *mean, *coef;             // [B,H], [B,3H+1,3]
    const int *code, *steps;               // [B,3H+1], [B]
    const float* eps;                      // [B,S,EC]: a path's base samples, the first steps[b] of a row are read
    float* out;                            // [B,S,H]
    int64_t S, H, EC;
    int flags;
};

// VE, VO: elements per global access of eps / out (4: 16-byte groups, where the row length and the pointer allow them)
template <int VE, int VO>
__global__ __launch_bounds__(64) void markov_predict_draw_kernel(DrawParams p) {
    __shared__ __attribute__((aligned(16))) float te[64 * MP_LD];
    __shared__ __attribute__((aligned(16))) float to[64 * MP_LD];
    const int lane = threadIdx.x;
    const int64_t b = blockIdx.y, S = p.S, H = p.H, EC = p.EC, EM = 3 * H + 1;
    const int64_t p0 = (int64_t)blockIdx.x * 64;
    const int rows = (int)(S - p0 < 64 ? S - p0 : 64);
    const double* __restrict__ mean = p.mean + b * H;
    const double* __restrict__ coef = p.coef + b * EM * 3;
    const int* __restrict__ code = p.code + b * EM;
    const float* eb = p.eps + (b * S + p0) * EC;
    float* ob = p.out + (b * S + p0) * H;
    const int64_t E = p.steps[b];
    if (E < 1 || E > EC || E > EM) {                                   // (uniform) a failed plan, or rows of eps too short for it
        const float nan = __builtin_nanf("");
        for (int64_t i = lane; i < rows * H; i += 64) ob[i] = nan;
        return;
    }
    const bool want_exp = (p.flags & VOLT_DRAW_EXP) != 0;
    const double kc = (p.flags & VOLT_PREDICT_NO_CHAIN) ? 0.0 : 1.0;   // the two parts' noise, switched off on request
    const double kb = (p.flags & VOLT_PREDICT_NO_BRIDGE) ? 0.0 : 1.0;
    double R = 0.0, L = 0.0, Ak = 0.0, Ab = 0.0;
    int64_t cur = (H - 1) / MP_CH * MP_CH;                             // first column of the chunk of out in the tile
    auto flush = [&]() {
        __syncthreads();
        const int cnt = (int)(H - cur < MP_CH ? H - cur : MP_CH);
        tile_store<float, VO, MP_CH>(to, [&](int r) { return ob + r * H + cur; }, rows, cnt, lane);
        __syncthreads();
    };
    for (int64_t e0 = 0; e0 < E; e0 += MP_CH) {
        const int cnt = (int)(E - e0 < MP_CH ? E - e0 : MP_CH);
        tile_load<float, VE, MP_CH>(te, [&](int r) { return eb + r * EC + e0; }, rows, cnt, lane);
        __syncthreads();
        for (int k = 0; k < cnt; ++k) {
            const int cd = code[e0 + k], op = cd & 7;
            const int64_t h = cd >> 3;
            const double a = coef[3 * (e0 + k)], bb = coef[3 * (e0 + k) + 1], c = coef[3 * (e0 + k) + 2];
            const double z = (double)te[lane * MP_LD + k];
            if (op == OP_KNOT) {
                R = a * R + kc * c * z;
            } else if (op == OP_OPEN) {
                L = a * R + kc * c * z;
                Ak = R;
                Ab = 0.0;
            } else if ((op == OP_POINT || op == OP_CLOSE) && h >= 0 && h < H) {
                if (h < cur) {                                         // (uniform) the chunk is complete: h only descends
                    flush();
                    cur = h / MP_CH * MP_CH;
                }
                Ak = a * L + bb * Ak;
                Ab = bb * Ab + kb * c * z;
                double y = mean[h] + (Ak + Ab);
                if (want_exp) y = exp(y);
                if (h - cur < MP_CH) to[lane * MP_LD + (int)(h - cur)] = (float)y;
                if (op == OP_CLOSE) R = L;
            }
        }
        __syncthreads();
    }
    flush();
}

struct PredictWs {
    double *s, *phi, *r;                   // [B,N]
    int* idx;                              // [B,H]
    size_t bytes;
};

static PredictWs carve_predict(void* base, int B, int N, int H) {
    Carver c{base};
    PredictWs w;
    w.s = c.take<double>((size_t)B * N);
    w.phi = c.take<double>((size_t)B * N);
    w.r = c.take<double>((size_t)B * N);
    w.idx = c.take<int>((size_t)B * H);
    w.bytes = c.off;
    return w;
}

static bool predict_shape_ok(int B, int N, int H) { return B >= 1 && B <= 65535 && N >= 1 && H >= 1 && H <= MP_HMAX; }

}  // namespace mpr
}  // namespace volt

using namespace volt;
using namespace volt::mpr;

extern "C" {

size_t volt_markov_predict_workspace_bytes(int B, int N, int H) {
    if (!predict_shape_ok(B, N, H)) return 0;
    return carve_predict(nullptr, B, N, H).bytes;
}

int volt_markov_predict_plan_f32(const float* x, const float* xs, const float* vol, float jitter, const float* mu, const float* m,
                                 const float* rho, const float* gamma, double* mean, double* var_q, double* var_p, double* coef,
                                 int* code, int* steps, int* info, void* workspace, int B, int N, int H, void* stream) {
    if (!x) return -1;
    if (!xs) return -2;
    if (!vol) return -3;
    if (!mu) return -5;
    if (!m) return -6;
    if (!rho) return -7;
    if (!gamma) return -8;
    if (!mean) return -9;
    if (!var_q) return -10;
    if (!var_p) return -11;
    if (!coef) return -12;
    if (!code) return -13;
    if (!steps) return -14;
    if (!info) return -15;
    if (!workspace || ((uintptr_t)workspace & 255)) return -16;
    if (B < 1 || B > 65535) return -17;
    if (N < 1) return -18;
    if (H < 1 || H > MP_HMAX) return -19;
    const PredictWs w = carve_predict(workspace, B, N, H);
    PlanParams p = {x, xs, vol, mu, m, rho, gamma, (double)jitter, mean, var_q, var_p, coef, code, steps, info,
                    w.s, w.phi, w.r, w.idx, N, H};
    hipLaunchKernelGGL(markov_predict_plan_kernel, dim3(B), dim3(MP_T), 0, (hipStream_t)stream, p);
    VOLT_LAUNCH_CHECK();
    return 0;
}

int volt_markov_predict_draw_f32(const double* mean, const double* coef, const int* code, const int* steps, const float* eps,
                                 float* out, int B, int S, int H, int E, int flags, void* stream) {
    if (!mean) return -1;
    if (!coef) return -2;
    if (!code) return -3;
    if (!steps) return -4;
    if (!eps) return -5;
    if (!out) return -6;
    if (B < 1 || B > 65535) return -7;
    if (S < 1) return -8;
    if (H < 1 || H > MP_HMAX) return -9;
    if (E < 1) return -10;
    if (flags & ~(VOLT_DRAW_EXP | VOLT_PREDICT_NO_CHAIN | VOLT_PREDICT_NO_BRIDGE)) return -11;
    DrawParams p = {mean, coef, code, steps, eps, out, S, H, E, flags};
    const dim3 grid((unsigned)(((int64_t)S + 63) / 64), (unsigned)B);
    const bool ve = E % 4 == 0 && (uintptr_t)eps % 16 == 0, vo = H % 4 == 0 && (uintptr_t)out % 16 == 0;
    hipStream_t s = (hipStream_t)stream;
    if (ve && vo) hipLaunchKernelGGL((markov_predict_draw_kernel<4, 4>), grid, dim3(64), 0, s, p);
    else if (ve) hipLaunchKernelGGL((markov_predict_draw_kernel<4, 1>), grid, dim3(64), 0, s, p);
    else if (vo) hipLaunchKernelGGL((markov_predict_draw_kernel<1, 4>), grid, dim3(64), 0, s, p);
    else hipLaunchKernelGGL((markov_predict_draw_kernel<1, 1>), grid, dim3(64), 0, s, p);
    VOLT_LAUNCH_CHECK();
    return 0;
}

}  // extern "C"
