// gemm_tile.hpp -- device helpers the MFMA NT-GEMM kernels share (kernels_gemm.hip, kernels_adat.hip): the LDS image of a
// k-tile, the accumulator tile and its store.
#pragma once
#include "lpipm_internal.hpp"

namespace lpipm {

typedef double d4 __attribute__((ext_vector_type(4)));
typedef double d2 __attribute__((ext_vector_type(2)));

constexpr int LDS_STRIDE = BK + 2;  // doubles per LDS row (144 B, keeps 16-B alignment)
// Bank-conflict-free fragment reads.  A ds_read_b128 of a wave is served in four groups of 16 lanes that are NOT lanes
// 16g .. 16g+15 but {0-3,12-15,20-27}, {4-11,16-19,28-31}, {32-35,44-47,52-59}, {36-43,48-51,60-63} (MI355X_MICROARCH.md, LDS
// table): with rows 36 dwords apart and lane (fr, fq) reading the 16-byte k-block fq of row fr, 28 of every 64 lane slots
// collided (PMC, round 3: SQ_LDS_BANK_CONFLICT = 37 % of SQ_LDS_IDX_ACTIVE in the A.D.A^T launch).  Rows 4..11 of every
// 16 keep their k-blocks pairwise swapped (block kb sits at kb ^ 1): every group then covers the 64 banks exactly once
// (exhaustive search over per-row XOR / rotation swizzles; none exists for a plain rotation).  The staging stores of a
// row are its 8 blocks in another order: still one contiguous 128-byte run per 8 lanes.  Which k a lane multiplies is
// unchanged, so are all results.
__device__ __forceinline__ int lds_swz(int row) { return ((row + 4) >> 3) & 1; }
__device__ __forceinline__ int lds_wcol(int row, int scol) { return scol ^ (lds_swz(row) << 1); }     // scol = 2 * k-block
__device__ __forceinline__ int lds_rq(int fr, int fq) { return (fq ^ lds_swz(fr)) << 1; }

// The panel solve's products of one k-tile for one 16x16 block, from the k-tile's LDS images (rows row0 .. row0 + 15 of either
// operand): per round one fragment of each side, then two MFMAs.  An element's sum is this sequence over the k-tiles in
// ascending order and nothing else: gemm_nt_rows32_k128_kernel and the panel workgroups of potrf_diag_kernel both run it.
__device__ __forceinline__ d2 ktile_frag(const double (*img)[LDS_STRIDE], int row0, int round, int fr, int fq) {
    return *(const d2*)&img[row0 + fr][round * 8 + lds_rq(fr, fq)];
}
__device__ __forceinline__ void ktile_mfma2(d4& acc, const d2& a, const d2& b) {
#pragma unroll
    for (int t = 0; t < 2; ++t) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a[t], b[t], acc, 0, 0, 0);
}

template <int MTM, int MTN>
__device__ __forceinline__ void acc_clear(d4 (&acc)[MTM][MTN]) {
#pragma unroll
    for (int mi = 0; mi < MTM; ++mi)
#pragma unroll
        for (int nj = 0; nj < MTN; ++nj) acc[mi][nj] = (d4){0.0, 0.0, 0.0, 0.0};
}

// C tile <- beta*C + alpha*acc.  C/D layout of v_mfma_f64_16x16x4_f64: col = lane&15,
// row = (lane>>4) + 4*reg.  Per-lane base pointer + wave-uniform row offsets keep the address math
// in SGPRs.  cb = &C[tile_row0 + wr*16*MTM + fq][tile_col0 + wc*16*MTN + fr].
template <int MTM, int MTN>
__device__ __forceinline__ void tile_store(double* cb, long long ldc, const d4 (&acc)[MTM][MTN], double alpha,
                                           double beta, bool pad_diag, int row0, int diag_pad_from, int fr, int fq,
                                           int diag_delta = 0) {   // (wave's column offset - row offset) inside the tile
    if (beta != 0.0) {   // wave-uniform.  All C values of a 16-row block are requested before any is used.
#pragma unroll
        for (int mi = 0; mi < MTM; ++mi) {
            double cv[4][MTN];
#pragma unroll
            for (int r = 0; r < 4; ++r)
#pragma unroll
                for (int nj = 0; nj < MTN; ++nj) cv[r][nj] = cb[(long long)(mi * 16 + 4 * r) * ldc + nj * 16];
#pragma unroll
            for (int r = 0; r < 4; ++r)
#pragma unroll
                for (int nj = 0; nj < MTN; ++nj)
                    cb[(long long)(mi * 16 + 4 * r) * ldc + nj * 16] = fma(alpha, acc[mi][nj][r], beta * cv[r][nj]);
        }
        return;
    }
#pragma unroll
    for (int mi = 0; mi < MTM; ++mi)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            double* rp = cb + (long long)(mi * 16 + 4 * r) * ldc;
#pragma unroll
            for (int nj = 0; nj < MTN; ++nj) {
                double v = alpha * acc[mi][nj][r];
                if (pad_diag && (mi - nj) * 16 + fq + 4 * r - fr == diag_delta && row0 + mi * 16 + 4 * r >= diag_pad_from) v = 1.0;
                rp[nj * 16] = v;
            }
        }
}

}  // namespace lpipm
