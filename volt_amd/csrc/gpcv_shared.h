// What the two variational steps (gpcv.hip: one series per batch entry; gpcv_mt.hip: T series behind ONE prior) share:
// the structured NT GEMM on the 128x128 MFMA core and the triangle-keeping transpose.  The kernels live in gpcv.hip;
// these are their host-side launchers.
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

}  // namespace volt
