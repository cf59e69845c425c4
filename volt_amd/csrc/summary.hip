// Path summaries: for every series g and horizon step h, the S sample paths samples[g, :, h] reduced to moments, quantiles,
// counts against a realised value (the reference's ECDF numerator, voltron/option_utils.py:48-52), CRPS and call / put values
// (Pricer's valuation, :36) -- what every consumer of a rollout computes on the host after samples.cpu().
//
// Two kernels, no communication between workgroups, no atomics, every reduction in a fixed order (bitwise repeatable):
//   summary_transpose_kernel   samples[g, s, h] (h contiguous, row stride ld) -> scratch[g][h][s] (s contiguous, row stride
//                              round_up(S, 64)) through a 64 x 64 LDS tile: both sides move whole 256-byte rows.  The samples
//                              stay fp32 and untransformed: exp is monotone, so the sort runs on x, and the fp64 exponential
//                              the statistics want is taken after the sort from the fp32 sample.
//   summary_column_kernel      one workgroup per column: load, count NaN, bitonic sort in LDS over the next power of two P
//                              (the padding is +inf and stays out of every statistic BY COUNT: only the first S entries of
//                              the sorted column are ever read, nothing is compared with the padding's value), then the
//                              reductions in fp64.
#include "common.h"
#include "host.h"
#include "../../include/volt_hip.h"

namespace volt {

constexpr int SUM_TILE = 64;               // transpose tile edge (256-byte rows on both sides)
constexpr int SUM_STRIKES = 8;             // strikes per pass over the column (their sums live in registers)

__host__ __device__ inline int64_t summary_col_stride(int S) { return ((int64_t)S + 63) & ~(int64_t)63; }

struct SummaryParams {
    const float* samples;
    int64_t ld, bs;
    int G, S, H, flags;
    const double* q;
    int Q;
    const float* truth;
    const float* strikes;
    int M;
    float *moments, *quant;
    int* counts;
    float *crps, *call, *put;
    float* scratch;
    int P, lgP;                            // the sort's size: next power of two >= S
};

__global__ __launch_bounds__(256) void summary_transpose_kernel(SummaryParams p) {
    __shared__ float tile[SUM_TILE][SUM_TILE + 1];
    const int th = (p.H + SUM_TILE - 1) / SUM_TILE, ts = (p.S + SUM_TILE - 1) / SUM_TILE;
    int w = blockIdx.x;
    const int bh = w % th;
    w /= th;
    const int bsi = w % ts;
    const int g = w / ts;
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    const int h0 = bh * SUM_TILE, s0 = bsi * SUM_TILE;
    const float* src = p.samples + (int64_t)g * p.bs;
#pragma unroll 4
    for (int r = ty; r < SUM_TILE; r += 4) {
        const int s = s0 + r, h = h0 + tx;
        if (s < p.S && h < p.H) tile[r][tx] = src[(int64_t)s * p.ld + h];
    }
    __syncthreads();
    const int64_t cs = summary_col_stride(p.S);
    float* dst = p.scratch + (int64_t)g * p.H * cs;
#pragma unroll 4
    for (int r = ty; r < SUM_TILE; r += 4) {
        const int h = h0 + r, s = s0 + tx;
        if (h < p.H && s < p.S) dst[(int64_t)h * cs + s] = tile[tx][r];
    }
}

// sum over the workgroup, the same value in every thread: xor butterfly inside a wave, then the waves' sums in wave order
__device__ __forceinline__ double block_sum(double v, double* red) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = (blockDim.x + 63) >> 6;
    if (lane == 0) red[wave] = v;
    __syncthreads();
    double s = 0.0;
    for (int i = 0; i < nw; ++i) s += red[i];
    __syncthreads();
    return s;
}
__device__ __forceinline__ int block_sum_i(int v, int* red) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = (blockDim.x + 63) >> 6;
    if (lane == 0) red[wave] = v;
    __syncthreads();
    int s = 0;
    for (int i = 0; i < nw; ++i) s += red[i];
    __syncthreads();
    return s;
}

__device__ __forceinline__ void cex(float& a, float& b, bool asc) {
    const bool sw = asc ? (a > b) : (a < b);
    const float t = a;
    a = sw ? b : a;
    b = sw ? t : b;
}

// R consecutive layers of the bitonic merge of size k, strides jtop, jtop / 2, .. jl = jtop >> (R - 1), in ONE pass over LDS
// and one barrier: a thread takes the 2^R entries those layers connect (i + m jl, m < 2^R; all in one block of k, so one
// direction), runs the layers in registers and puts them back.  With jl = 1 the entries are contiguous: 16-byte accesses.
template <int R>
__device__ __forceinline__ void sort_pass(float* xs, int P, int k, int jtop) {
    constexpr int E = 1 << R;
    const int jl = jtop >> (R - 1);
    for (int t = threadIdx.x; t < (P >> R); t += blockDim.x) {
        const int i = ((t & ~(jl - 1)) << R) | (t & (jl - 1));
        const bool asc = (i & k) == 0;
        float a[E];
        if (E >= 4 && jl == 1) {
#pragma unroll
            for (int m = 0; m + 3 < E; m += 4) {
                const f32x4 v = *reinterpret_cast<const f32x4*>(xs + i + m);
                a[m] = v[0], a[m + 1] = v[1], a[m + 2] = v[2], a[m + 3] = v[3];
            }
        } else {
#pragma unroll
            for (int m = 0; m < E; ++m) a[m] = xs[i + m * jl];
        }
#pragma unroll
        for (int r = R - 1; r >= 0; --r)
#pragma unroll
            for (int m = 0; m < E; ++m)
                if (!(m & (1 << r))) cex(a[m], a[m | (1 << r)], asc);
        if (E >= 4 && jl == 1) {
#pragma unroll
            for (int m = 0; m + 3 < E; m += 4) {
                f32x4 v;
                v[0] = a[m], v[1] = a[m + 1], v[2] = a[m + 2], v[3] = a[m + 3];
                *reinterpret_cast<f32x4*>(xs + i + m) = v;
            }
        } else {
#pragma unroll
            for (int m = 0; m < E; ++m) xs[i + m * jl] = a[m];
        }
    }
    __syncthreads();
}

template <bool EXP> __device__ __forceinline__ double value_of(float x) {
    if constexpr (EXP) return exp((double)x);
    else return (double)x;
}

// sums of max(v - K, 0) and max(K - v, 0) over the sorted column for the strikes m0 .. m0 + SUM_STRIKES - 1
template <bool EXP>
__device__ void strike_pass(const SummaryParams& p, const float* xs, int g, int h, int m0, double* red) {
    double kk[SUM_STRIKES], c[SUM_STRIKES], u[SUM_STRIKES];
#pragma unroll
    for (int m = 0; m < SUM_STRIKES; ++m) {
        kk[m] = (m0 + m < p.M) ? (double)p.strikes[(int64_t)g * p.M + m0 + m] : 0.0;
        c[m] = 0.0;
        u[m] = 0.0;
    }
    for (int i = threadIdx.x; i < p.S; i += blockDim.x) {
        const double v = value_of<EXP>(xs[i]);
#pragma unroll
        for (int m = 0; m < SUM_STRIKES; ++m) {
            c[m] += fmax(v - kk[m], 0.0);
            u[m] += fmax(kk[m] - v, 0.0);
        }
    }
#pragma unroll
    for (int m = 0; m < SUM_STRIKES; ++m) {
        const double cs = block_sum(c[m], red), us = block_sum(u[m], red);
        if (threadIdx.x == 0 && m0 + m < p.M) {
            const int64_t o = ((int64_t)g * p.M + m0 + m) * p.H + h;
            p.call[o] = (float)(cs / p.S);
            p.put[o] = (float)(us / p.S);
        }
    }
}

template <bool EXP>
__global__ __launch_bounds__(1024) void summary_column_kernel(SummaryParams p) {
    extern __shared__ __attribute__((aligned(16))) float xs[];          // P floats
    __shared__ double red[16];
    __shared__ int redi[16];
    const int col = blockIdx.x, g = col / p.H, h = col % p.H;
    const int tid = threadIdx.x, nt = blockDim.x;
    const int S = p.S, P = p.P;
    const float* src = p.scratch + (int64_t)col * summary_col_stride(S);
    const float inf = __builtin_inff(), nanf = __builtin_nanf("");

    int nn = 0;
    for (int i = tid; i < P; i += nt) {
        float x = inf;
        if (i < S) {
            x = src[i];
            nn += (x != x);
        }
        xs[i] = x;
    }
    const int n_nan = block_sum_i(nn, redi);       // (its barriers also publish xs)
    const float ty = p.truth ? p.truth[(int64_t)g * p.H + h] : nanf;
    const bool has_truth = ty == ty;

    if (n_nan > 0) {                               // a column with a NaN sample: NaN everywhere, the count reported
        if (tid == 0) {
            if (p.moments)
                for (int k = 0; k < 4; ++k) p.moments[((int64_t)g * 4 + k) * p.H + h] = nanf;
            if (p.counts) {
                p.counts[((int64_t)g * 3 + 0) * p.H + h] = n_nan;
                p.counts[((int64_t)g * 3 + 1) * p.H + h] = -1;
                p.counts[((int64_t)g * 3 + 2) * p.H + h] = -1;
            }
            if (p.crps) p.crps[(int64_t)g * p.H + h] = nanf;
        }
        for (int j = tid; j < p.Q; j += nt) p.quant[((int64_t)g * p.Q + j) * p.H + h] = nanf;
        for (int m = tid; m < p.M; m += nt) {
            p.call[((int64_t)g * p.M + m) * p.H + h] = nanf;
            p.put[((int64_t)g * p.M + m) * p.H + h] = nanf;
        }
        return;
    }

    // ---- bitonic sort, ascending, over P entries.  The log2(k) compare-exchange layers of a merge of size k run three at
    // a time (sort_pass<3>: one pass over LDS and one barrier per three layers); a layer count that is no multiple of three
    // starts with a pass of one or two layers, so the last pass of every merge ends at stride 1.
    for (int k = 2, lk = 1; k <= P; k <<= 1, ++lk) {
        int j = k >> 1;                            // the merge's layers: strides k/2 .. 1, lk of them
        const int first = lk % 3;
        if (first == 1) sort_pass<1>(xs, P, k, j), j >>= 1;
        else if (first == 2) sort_pass<2>(xs, P, k, j), j >>= 2;
        for (; j >= 4; j >>= 3) sort_pass<3>(xs, P, k, j);
    }

    // ---- pass 1: sum, sum |v - y|, the CRPS spread sum, the counts
    const double y = (double)ty;
    double s1 = 0.0, sa = 0.0, sw = 0.0;
    int lt = 0, le = 0;
    for (int i = tid; i < S; i += nt) {
        const double v = value_of<EXP>(xs[i]);
        s1 += v;
        sw += (double)(2 * i + 1 - S) * v;         // (2 i1 - S - 1) v, i1 = i + 1
        if (has_truth) {
            sa += fabs(v - y);
            lt += (v < y);
            le += (v <= y);
        }
    }
    const double sum = block_sum(s1, red);
    const double wsum = block_sum(sw, red);
    const double mean = sum / S;
    if (has_truth) {                               // (uniform over the workgroup)
        const double asum = block_sum(sa, red);
        lt = block_sum_i(lt, redi);
        le = block_sum_i(le, redi);
        if (tid == 0 && p.crps) p.crps[(int64_t)g * p.H + h] = (float)(asum / S - wsum / ((double)S * (double)S));
    } else if (tid == 0 && p.crps) {
        p.crps[(int64_t)g * p.H + h] = nanf;
    }
    if (tid == 0 && p.counts) {
        p.counts[((int64_t)g * 3 + 0) * p.H + h] = 0;
        p.counts[((int64_t)g * 3 + 1) * p.H + h] = has_truth ? lt : -1;
        p.counts[((int64_t)g * 3 + 2) * p.H + h] = has_truth ? le : -1;
    }

    // ---- pass 2: the deviation about the mean (the column is resident)
    if (p.moments) {
        double s2 = 0.0;
        for (int i = tid; i < S; i += nt) {
            const double d = value_of<EXP>(xs[i]) - mean;
            s2 += d * d;
        }
        const double ss = block_sum(s2, red);
        if (tid == 0) {
            p.moments[((int64_t)g * 4 + 0) * p.H + h] = (float)mean;
            p.moments[((int64_t)g * 4 + 1) * p.H + h] = (float)sqrt(ss / (double)(S - 1));     // S = 1: 0 / 0
            p.moments[((int64_t)g * 4 + 2) * p.H + h] = (float)value_of<EXP>(xs[0]);
            p.moments[((int64_t)g * 4 + 3) * p.H + h] = (float)value_of<EXP>(xs[S - 1]);
        }
    }

    // ---- quantiles: torch's "linear" rule in fp64
    for (int j = tid; j < p.Q; j += nt) {
        const double pos = p.q[j] * (double)(S - 1);
        int lo = (int)floor(pos);
        lo = lo < 0 ? 0 : (lo > S - 1 ? S - 1 : lo);           // (levels outside [0, 1] never index outside the column)
        const int hi = lo + 1 > S - 1 ? S - 1 : lo + 1;
        const double vl = value_of<EXP>(xs[lo]), vh = value_of<EXP>(xs[hi]);
        p.quant[((int64_t)g * p.Q + j) * p.H + h] = (float)(vl + (vh - vl) * (pos - (double)lo));
    }

    // ---- option values, SUM_STRIKES strikes per pass
    for (int m0 = 0; m0 < p.M; m0 += SUM_STRIKES) strike_pass<EXP>(p, xs, g, h, m0, red);
}

}  // namespace volt

extern "C" {

size_t volt_path_summary_scratch_bytes(int G, int S, int H) {
    if (G < 1 || S < 1 || S > VOLT_SUMMARY_MAX_S || H < 1) return 0;
    return (size_t)G * H * (size_t)volt::summary_col_stride(S) * sizeof(float);
}

int volt_path_summary_f32(const float* samples, int64_t ld, int64_t bs, int G, int S, int H, int flags, const double* q,
                          int Q, const float* truth, const float* strikes, int M, float* moments, float* quant, int* counts,
                          float* crps, float* call, float* put, void* scratch, size_t scratch_bytes, void* stream) {
    using namespace volt;
    if (!samples) return -1;
    if (G < 1) return -4;
    if (S < 1 || S > VOLT_SUMMARY_MAX_S) return -5;
    if (H < 1) return -6;
    if (ld < H) return -2;
    if (flags & ~VOLT_SUMMARY_EXP) return -7;
    if (Q < 0) return -9;
    if (Q > 0 && !q) return -8;
    if (Q > 0 && !quant) return -14;
    if (M < 0) return -12;
    if (M > 0 && !strikes) return -11;
    if (M > 0 && !call) return -17;
    if (M > 0 && !put) return -18;
    if (!scratch || ((uintptr_t)scratch & 255)) return -19;
    if (scratch_bytes < volt_path_summary_scratch_bytes(G, S, H)) return -20;
    const int64_t tiles = (int64_t)G * ((S + SUM_TILE - 1) / SUM_TILE) * ((H + SUM_TILE - 1) / SUM_TILE);
    if (tiles > 0x7fffffff || (int64_t)G * H > 0x7fffffff) return -4;
    int P = 1, lgP = 0;
    while (P < S) P <<= 1, ++lgP;
    SummaryParams p{samples, ld, bs, G, S, H, flags, q, Q, truth, strikes, M, moments, quant, counts, crps, call, put,
                    (float*)scratch, P, lgP};
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(summary_transpose_kernel, dim3((unsigned)tiles), dim3(256), 0, s, p);
    VOLT_LAUNCH_CHECK();
    const size_t lds = (size_t)P * sizeof(float);
    int nt = P / 8;                                // one group of eight entries per thread and pass, up to 1024 threads
    nt = nt < 64 ? 64 : (nt > 1024 ? 1024 : nt);
    hipError_t e;
#define VOLT_SUMMARY_LAUNCH(EXP)                                                                                       \
    do {                                                                                                               \
        e = hipFuncSetAttribute(reinterpret_cast<const void*>(summary_column_kernel<EXP>),                            \
                                hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);                                \
        if (e != hipSuccess) return (int)e;                                                                            \
        hipLaunchKernelGGL(summary_column_kernel<EXP>, dim3((unsigned)((int64_t)G * H)), dim3(nt), lds, s, p);        \
    } while (0)
    if (flags & VOLT_SUMMARY_EXP) VOLT_SUMMARY_LAUNCH(true);
    else VOLT_SUMMARY_LAUNCH(false);
#undef VOLT_SUMMARY_LAUNCH
    VOLT_LAUNCH_CHECK();
    return 0;
}

}  // extern "C"
