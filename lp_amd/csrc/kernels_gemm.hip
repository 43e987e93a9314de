// kernels_gemm.hip -- fp64 MFMA "NT" GEMM for gfx950 (CDNA4): the whole-tile and grouped launches of the factorisation.
//
//   C(ti,tj) = beta*C + alpha * sum_k P[ti*TM + r][k] * Q[tj*TN + c][k]
//
// Row-major operands with K contiguous, which is exactly the A/B fragment shape of v_mfma_f64_16x16x4_f64 (lane l holds
// X[l&15][k = l>>4]); K is permuted so that each lane reads two consecutive k (one ds_read_b128) per pair of MFMAs.
// k-tiles of 16 are register-staged (global_load_dwordx4: 8 lanes x 16 B = one full 128-B line per row) and written to a
// double-buffered padded LDS image (gemm_tile.hpp), one barrier per k-tile.  One output tile per 256-thread workgroup of
// 2x2 waves (512 threads for the 32-row panel solve): the Cholesky trailing update (alpha=-1, beta=1), TRSM-as-GEMM, and
// the grouped products of the super-block inverses.  A.D.A^T shares the tile helpers and lives in kernels_adat.hip.
#include "gemm_tile.hpp"

namespace lpipm {

struct GemmK {
    const double* P; long long ldp;
    const double* Q; long long ldq;
    double* C; long long ldc;
    int KT;
    double alpha, beta;
    int tiles_lower, ntj, skip_upper;
    BatchK bk;
};
// LP blockIdx.z of a lockstep batch: per-LP pointers shifted
__device__ __forceinline__ GemmK batch_shift(const GemmK& p0) {
    GemmK p = p0;
    const long long sh = batch_lp(p0.bk) * p0.bk.stride;
    p.P = (const double*)((const char*)p0.P + sh); p.Q = (const double*)((const char*)p0.Q + sh); p.C = (double*)((char*)p0.C + sh);
    return p;
}

__device__ __forceinline__ void tile_coords(const GemmK& p, int t, int& ti, int& tj) {
    if (p.tiles_lower) {
        int i = (int)((sqrt(8.0 * (double)t + 1.0) - 1.0) * 0.5);
        while ((i + 1) * (i + 2) / 2 <= t) ++i;
        while (i * (i + 1) / 2 > t) --i;
        ti = i; tj = t - i * (i + 1) / 2;
    } else {
        ti = t / p.ntj; tj = t - ti * p.ntj;
    }
}
// A tile of a rectangular band whose rows all lie above its columns: nothing reads it (GemmArgs::skip_upper).
__device__ __forceinline__ bool tile_unread(const GemmK& p, int ti, int tj, int TM, int TN) {
    return p.skip_upper && ti * TM + TM <= tj * TN;
}

// acc(128x128 tile, 64 doubles per lane) += sum over k-tiles [kb, ke) of P-panel . (s o Q-panel)^T
// Pp / Qp point at this thread's first staging element (row srow, column scol of the panels).
// MTM x MTN = 16x16 MFMA tiles per wave (2x2 waves per workgroup): workgroup tile = 32*MTM x 32*MTN.
//   4x4 -> 128x128 (throughput launches), 2x2 -> 64x64 and 1x4 -> 32x128 (latency-bound launches)
// PF register stages of global loads are in flight: k-tile k + PF is requested while k-tile k is multiplied, so a
// load has PF - 1 whole k-tile periods to arrive.  With one stage (the first version) the small-tile launches of
// the factorisation -- one round of tiles, nothing else on the CU -- ran at ~1.5 us per k-tile, the latency of an L2 /
// Infinity-Cache load, against 0.43 us of MFMA work (trace: a K = 512 trailing update of 64x64 tiles 50 us).
template <bool SCALE, int MTM, int MTN, int PF = (MTM * MTN >= 16 ? 2 : 3)>
__device__ __forceinline__ void tile_mainloop(double (*ldsA)[32 * MTM][LDS_STRIDE], double (*ldsB)[32 * MTN][LDS_STRIDE],
                                              const double* __restrict__ Pp, long long ldp,
                                              const double* __restrict__ Qp, long long ldq,
                                              const double* __restrict__ s, int kb, int ke, d4 (&acc)[MTM][MTN],
                                              int srow, int scol, int wr, int wc, int fr, int fq) {
    d2 sa[PF][MTM], sb[PF][MTN], sv[PF];
    auto gload = [&](int kt, int st) {
        const long long ko = (long long)kt * BK;
#pragma unroll
        for (int r = 0; r < MTM; ++r) sa[st][r] = *(const d2*)(Pp + (long long)(32 * r) * ldp + ko);
#pragma unroll
        for (int r = 0; r < MTN; ++r) sb[st][r] = *(const d2*)(Qp + (long long)(32 * r) * ldq + ko);
        sv[st] = SCALE ? *(const d2*)(s + ko + scol) : (d2){1.0, 1.0};
    };
    // the scale is applied here, after the MFMAs of the current k-tile: multiplying right after the
    // loads would make the wave wait for the prefetch it has just issued
    auto lstore = [&](int buf, int st) {
#pragma unroll
        for (int r = 0; r < MTM; ++r) *(d2*)&ldsA[buf][srow + 32 * r][lds_wcol(srow, scol)] = sa[st][r];
#pragma unroll
        for (int r = 0; r < MTN; ++r) *(d2*)&ldsB[buf][srow + 32 * r][lds_wcol(srow, scol)] = SCALE ? sb[st][r] * sv[st] : sb[st][r];
    };
#pragma unroll
    for (int u = 0; u < PF; ++u)
        if (kb + u < ke) gload(kb + u, u);
    lstore(0, 0);
    __syncthreads();
    int cur = 0;
    for (int kt0 = kb; kt0 < ke; kt0 += PF) {
#pragma unroll
        for (int u = 0; u < PF; ++u) {          // k-tile kt0 + u lives in stage u and is in LDS buffer `cur`
            const int kt = kt0 + u;
            if (kt < ke) {
                if (kt + PF < ke) gload(kt + PF, u);
#pragma unroll
                for (int round = 0; round < 2; ++round) {
                    d2 a[MTM], b[MTN];
#pragma unroll
                    for (int mi = 0; mi < MTM; ++mi)
                        a[mi] = *(const d2*)&ldsA[cur][wr * (16 * MTM) + mi * 16 + fr][round * 8 + lds_rq(fr, fq)];
#pragma unroll
                    for (int nj = 0; nj < MTN; ++nj)
                        b[nj] = *(const d2*)&ldsB[cur][wc * (16 * MTN) + nj * 16 + fr][round * 8 + lds_rq(fr, fq)];
#pragma unroll
                    for (int t = 0; t < 2; ++t)
#pragma unroll
                        for (int mi = 0; mi < MTM; ++mi)
#pragma unroll
                            for (int nj = 0; nj < MTN; ++nj)
                                acc[mi][nj] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[mi][t], b[nj][t], acc[mi][nj], 0, 0, 0);
                }
                if (kt + 1 < ke) lstore(cur ^ 1, (u + 1) % PF);
                __syncthreads();
                cur ^= 1;
            }
        }
    }
}

#define TILE_THREAD_IDS                                                    \
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;         \
    const int wr = wave >> 1, wc = wave & 1;                               \
    const int fr = lane & 15, fq = lane >> 4;                              \
    const int srow = tid >> 3;  /* staging: 32 rows per pass, 8 lanes per 128-B row segment */ \
    const int scol = (tid & 7) * 2;

// One full tile per workgroup (Cholesky trailing update, TRSM-as-GEMM): no k-split, no slabs.
// Tile coordinates are in units of (32*MTM rows, 32*MTN columns).
template <int MTM, int MTN>
__global__ __launch_bounds__(256, 2) void gemm_nt_tile_kernel(const GemmK p0) {
    if (batch_done(p0.bk)) return;
    const GemmK p = batch_shift(p0);
    constexpr int TM = 32 * MTM, TN = 32 * MTN;
    __shared__ __attribute__((aligned(16))) double ldsA[2][TM][LDS_STRIDE];
    __shared__ __attribute__((aligned(16))) double ldsB[2][TN][LDS_STRIDE];
    TILE_THREAD_IDS
    int ti, tj;
    tile_coords(p, blockIdx.x, ti, tj);
    if (tile_unread(p, ti, tj, TM, TN)) return;
    d4 acc[MTM][MTN];
    acc_clear(acc);
    tile_mainloop<false, MTM, MTN>(ldsA, ldsB, p.P + (long long)(ti * TM + srow) * p.ldp + scol, p.ldp,
                                   p.Q + (long long)(tj * TN + srow) * p.ldq + scol, p.ldq, nullptr, 0, p.KT, acc,
                                   srow, scol, wr, wc, fr, fq);
    double* cb = p.C + (long long)(ti * TM + wr * (16 * MTM) + fq) * p.ldc + (tj * TN + wc * (16 * MTN) + fr);
    tile_store<MTM, MTN>(cb, p.ldc, acc, p.alpha, p.beta, false, 0, -1, fr, fq);
}

// K = 128 specialisation of the whole-tile kernel for the latency-bound steps of the factorisation
// (panel solve, update inside an outer panel): with 16 MFMAs per wave and k-tile the one-ahead
// prefetch of tile_mainloop cannot hide a global-load round trip, so all 8 k-tiles are requested up
// front (they fit in registers for these small tiles) and the round trip is paid once per tile.
template <int MTM, int MTN>
__global__ __launch_bounds__(256, 2) void gemm_nt_tile_k128_kernel(const GemmK p0) {
    if (batch_done(p0.bk)) return;
    const GemmK p = batch_shift(p0);
    constexpr int TM = 32 * MTM, TN = 32 * MTN, KT8 = 8;
    __shared__ __attribute__((aligned(16))) double ldsA[2][TM][LDS_STRIDE];
    __shared__ __attribute__((aligned(16))) double ldsB[2][TN][LDS_STRIDE];
    TILE_THREAD_IDS
    int ti, tj;
    tile_coords(p, blockIdx.x, ti, tj);
    if (tile_unread(p, ti, tj, TM, TN)) return;
    const double* Pp = p.P + (long long)(ti * TM + srow) * p.ldp + scol;
    const double* Qp = p.Q + (long long)(tj * TN + srow) * p.ldq + scol;
    d2 pa[KT8][MTM], pb[KT8][MTN];
#pragma unroll
    for (int kt = 0; kt < KT8; ++kt) {
#pragma unroll
        for (int r = 0; r < MTM; ++r) pa[kt][r] = *(const d2*)(Pp + (long long)(32 * r) * p.ldp + kt * BK);
#pragma unroll
        for (int r = 0; r < MTN; ++r) pb[kt][r] = *(const d2*)(Qp + (long long)(32 * r) * p.ldq + kt * BK);
    }
    d4 acc[MTM][MTN];
    acc_clear(acc);
#pragma unroll
    for (int kt = 0; kt < KT8; ++kt) {
        const int buf = kt & 1;
#pragma unroll
        for (int r = 0; r < MTM; ++r) *(d2*)&ldsA[buf][srow + 32 * r][lds_wcol(srow, scol)] = pa[kt][r];
#pragma unroll
        for (int r = 0; r < MTN; ++r) *(d2*)&ldsB[buf][srow + 32 * r][lds_wcol(srow, scol)] = pb[kt][r];
        __syncthreads();   // buffer `buf` was last read two k-tiles ago: that read finished before the previous barrier
#pragma unroll
        for (int round = 0; round < 2; ++round) {
            d2 a[MTM], b[MTN];
#pragma unroll
            for (int mi = 0; mi < MTM; ++mi)
                a[mi] = *(const d2*)&ldsA[buf][wr * (16 * MTM) + mi * 16 + fr][round * 8 + lds_rq(fr, fq)];
#pragma unroll
            for (int nj = 0; nj < MTN; ++nj)
                b[nj] = *(const d2*)&ldsB[buf][wc * (16 * MTN) + nj * 16 + fr][round * 8 + lds_rq(fr, fq)];
#pragma unroll
            for (int t = 0; t < 2; ++t)
#pragma unroll
                for (int mi = 0; mi < MTM; ++mi)
#pragma unroll
                    for (int nj = 0; nj < MTN; ++nj)
                        acc[mi][nj] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[mi][t], b[nj][t], acc[mi][nj], 0, 0, 0);
        }
    }
    double* cb = p.C + (long long)(ti * TM + wr * (16 * MTM) + fq) * p.ldc + (tj * TN + wc * (16 * MTN) + fr);
    tile_store<MTM, MTN>(cb, p.ldc, acc, p.alpha, p.beta, false, 0, -1, fr, fq);
}

// The in-place panel solve of the factorisation (L21 = A21 . inv(L_kk)^T): a workgroup must own whole rows, so its tile is
// 32 rows x all 128 columns; on 8 waves (2 x 4 waves of 16 x 32) a wave runs 64 MFMAs instead of the 128 of the 4-wave
// <1, 4> tile -- the launch is one round of tiles on a chain, its length is the per-wave MFMA count plus one round trip
// (factorisation at m = 4096: 1909 -> 1896 us).  Q MUST be lower triangular with exact zeros above its diagonal (the
// 128-block inverse): the kernel neither loads nor multiplies what lies above it.
__global__ __launch_bounds__(512, 1) void gemm_nt_rows32_k128_kernel(const GemmK p0) {
    if (batch_done(p0.bk)) return;
    const GemmK p = batch_shift(p0);
    constexpr int TM = 32, TN = 128, KT8 = 8;
    __shared__ __attribute__((aligned(16))) double ldsA[2][TM][LDS_STRIDE];
    __shared__ __attribute__((aligned(16))) double ldsB[2][TN][LDS_STRIDE];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);   // wave-uniform: the triangle's tests below go scalar
    const int wr = wave >> 2, wc = wave & 3;
    const int fr = lane & 15, fq = lane >> 4;
    const int srow = tid >> 3, scol = (tid & 7) * 2;          // staging: 64 rows per pass, 8 lanes per 128-B row segment
    int ti, tj;
    tile_coords(p, blockIdx.x, ti, tj);
    // Q = inv(L_kk) is lower triangular: Q[c][k] = 0 for k > c, so k-tile kt meets only the rows c >= 16 kt of Q and the
    // 16-column blocks >= kt of the product.  Only those rows are requested (72 of Q's 128 KB) and only those products run
    // (36 of 64), each in the k order it always had.  Wave column wc takes the column blocks wc and 7 - wc: 9 products on
    // every wave.  (qb, the 16-row block of a staging row, is the same for the 8 rows a wave stages: the tests are scalar.)
    const bool stage_a = srow < TM;
    const int qb = wave >> 1;                                  // == srow >> 4; staging rows srow, srow + 64: blocks qb, qb + 4
    const double* Pp = p.P + (long long)(ti * TM + (stage_a ? srow : 0)) * p.ldp + scol;
    const double* Qp = p.Q + (long long)(tj * TN + srow) * p.ldq + scol;
    d2 pa[KT8], pb[KT8][2];
#pragma unroll
    for (int kt = 0; kt < KT8; ++kt) {
        pa[kt] = *(const d2*)(Pp + kt * BK);
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            pb[kt][r] = (d2){0.0, 0.0};
            if (kt <= qb + 4 * r) pb[kt][r] = *(const d2*)(Qp + (long long)(64 * r) * p.ldq + kt * BK);
        }
    }
    const int cblk[2] = {wc, 7 - wc};
    d4 acc[1][2];
    acc_clear(acc);
#pragma unroll
    for (int kt = 0; kt < KT8; ++kt) {
        const int buf = kt & 1;
        if (stage_a) *(d2*)&ldsA[buf][srow][lds_wcol(srow, scol)] = pa[kt];
#pragma unroll
        for (int r = 0; r < 2; ++r)
            if (kt <= qb + 4 * r) *(d2*)&ldsB[buf][srow + 64 * r][lds_wcol(srow, scol)] = pb[kt][r];
        __syncthreads();   // buffer `buf` was last read two k-tiles ago: that read finished before the previous barrier
        if (kt <= cblk[1]) {                                   // wave-uniform; cblk[0] <= cblk[1]
#pragma unroll
            for (int round = 0; round < 2; ++round) {
                const d2 a = ktile_frag(ldsA[buf], wr * 16, round, fr, fq);
#pragma unroll
                for (int nj = 0; nj < 2; ++nj) {
                    if (kt > cblk[nj]) continue;
                    ktile_mfma2(acc[0][nj], a, ktile_frag(ldsB[buf], cblk[nj] * 16, round, fr, fq));
                }
            }
        }
    }
#pragma unroll
    for (int nj = 0; nj < 2; ++nj) {
        const d4 one[1][1] = {{acc[0][nj]}};
        double* cb = p.C + (long long)(ti * TM + wr * 16 + fq) * p.ldc + (tj * TN + cblk[nj] * 16 + fr);
        tile_store<1, 1>(cb, p.ldc, one, p.alpha, p.beta, false, 0, -1, fr, fq);
    }
}

// Grouped GEMM: every workgroup takes its own descriptor (operands, k-range, alpha): the doubling
// levels of the super-block triangular inverse are a few such launches over many small products.
// Output tiles of 32 * MT rows and columns:
//   MT = 4 (128x128): flop-bound stages, 2 resident workgroups per CU.
//   MT = 2 (64x64, 4 resident workgroups per CU): a merge stage of one LP is a few dozen 128x128 tiles on 512 slots and
//          each tile's k-loop is pure latency, so quartering the tiles quarters the stage's duration; the triangular
//          k-ranges are also tighter at 64 granularity.
//   MT = 1 (32x32): the merge stages of one LP are one round of tiles each, so a stage lasts as long as its longest k-loop,
//          and a quarter-size tile has the shortest MFMA chain and the tightest triangular k-range.
template <int MT>
__global__ __launch_bounds__(256, MT == 4 ? 2 : 4) void gemm_nt_grouped_kernel(const GemmTileDesc* __restrict__ descs, BatchK bk) {
    if (batch_done(bk)) return;
    __shared__ __attribute__((aligned(16))) double ldsA[2][32 * MT][LDS_STRIDE];
    __shared__ __attribute__((aligned(16))) double ldsB[2][32 * MT][LDS_STRIDE];
    TILE_THREAD_IDS
    GemmTileDesc d = descs[blockIdx.x];
    d.P = batch_ptr(d.P, bk); d.Q = batch_ptr(d.Q, bk); d.C = batch_ptr(d.C, bk);
    d4 acc[MT][MT];
    acc_clear(acc);
    tile_mainloop<false, MT, MT>(ldsA, ldsB, d.P + (long long)srow * d.ldp + scol, d.ldp, d.Q + (long long)srow * d.ldq + scol,
                                 d.ldq, nullptr, d.kt_begin, d.kt_end, acc, srow, scol, wr, wc, fr, fq);
    double* cb = d.C + (long long)(wr * (16 * MT) + fq) * d.ldc + (wc * (16 * MT) + fr);
    tile_store<MT, MT>(cb, d.ldc, acc, d.alpha, 0.0, false, 0, -1, fr, fq);
}

hipError_t launch_gemm_nt(const GemmArgs& a, hipStream_t st) {
    GemmK k;
    k.P = a.P; k.ldp = a.ldp; k.Q = a.Q; k.ldq = a.ldq;
    k.C = a.C; k.ldc = a.ldc; k.KT = a.K / BK; k.alpha = a.alpha; k.beta = a.beta;
    k.tiles_lower = a.tiles_lower; k.ntj = a.ntj; k.skip_upper = a.skip_upper; k.bk = batch_k(a.batch);
    if (a.ntiles <= 0 || k.KT <= 0) return hipSuccess;
    const dim3 grid(a.ntiles, 1, a.batch.count);
    const TileShape shape = a.tile_shape;
    const bool k128 = k.KT == 8;    // the K = 128 specialisations (128x128 has none)
    if (shape == TileShape::T64x64 && k128)       hipLaunchKernelGGL((gemm_nt_tile_k128_kernel<2, 2>), grid, dim3(256), 0, st, k);
    else if (shape == TileShape::T32x128 && k128) hipLaunchKernelGGL(gemm_nt_rows32_k128_kernel, grid, dim3(512), 0, st, k);
    else if (shape == TileShape::T32x32 && k128)  hipLaunchKernelGGL((gemm_nt_tile_k128_kernel<1, 1>), grid, dim3(256), 0, st, k);
    else if (shape == TileShape::T64x64)          hipLaunchKernelGGL((gemm_nt_tile_kernel<2, 2>), grid, dim3(256), 0, st, k);
    else if (shape == TileShape::T32x32)          hipLaunchKernelGGL((gemm_nt_tile_kernel<1, 1>), grid, dim3(256), 0, st, k);
    else if (shape == TileShape::T32x128)         hipLaunchKernelGGL((gemm_nt_tile_kernel<1, 4>), grid, dim3(256), 0, st, k);
    else                                          hipLaunchKernelGGL((gemm_nt_tile_kernel<4, 4>), grid, dim3(256), 0, st, k);
    return hipGetLastError();
}

hipError_t launch_gemm_grouped(const GemmTileDesc* descs_dev, int ntiles, hipStream_t st, const Batch& bt, int edge) {
    if (ntiles <= 0) return hipSuccess;
    const dim3 grid(ntiles, 1, bt.count);
    if (edge == 32)      hipLaunchKernelGGL(gemm_nt_grouped_kernel<1>, grid, dim3(256), 0, st, descs_dev, batch_k(bt));
    else if (edge == 64) hipLaunchKernelGGL(gemm_nt_grouped_kernel<2>, grid, dim3(256), 0, st, descs_dev, batch_k(bt));
    else                 hipLaunchKernelGGL(gemm_nt_grouped_kernel<4>, grid, dim3(256), 0, st, descs_dev, batch_k(bt));
    return hipGetLastError();
}

}  // namespace lpipm
