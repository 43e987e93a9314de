// kernels_adat.hip -- M = A . diag(x/z) . A^T by fp64 MFMA for gfx950 (CDNA4), the dominant kernel of the hot path: the
// plan of a launch, its device resources, its two kernels and the launch (AdatPlan .. launch_adat, lpipm_internal.hpp).
//
//   M(ti,tj) = sum_k A[ti*128 + r][k] * s[k] * A[tj*128 + c][k]
//
// Replaces newton_equations.rs:54-57 (`A.dot(&(Dinv[:,None] * A.t()))`): the n x m scaled
// temporary is never materialised -- s = x/z is applied to the Q panel while it is staged into LDS
// -- and only the lower-triangular tiles are computed (the reference forms the full square).
// The whole-tile launches of the factorisation (kernels_gemm.hip) share the LDS image and the tile store (gemm_tile.hpp).
//
// Design (MI355X: 256 CUs, wave64, 160 KB LDS/CU, v_mfma_f64_16x16x4_f64):
//   * 128x128 output tile per 256-thread workgroup = 2x2 waves of 64x64 = 4x4 MFMA tiles each:
//     64 fp64 accumulators per lane (128 VGPRs), 2 workgroups per CU (2 waves per SIMD) so one
//     wave's LDS/barrier stalls hide under the other's MFMAs.
//   * both operands are row-major with K contiguous, which is exactly the A/B fragment shape of
//     the 16x16x4 MFMA (lane l holds X[l&15][k = l>>4]); K is permuted so that each lane reads
//     two consecutive k (one ds_read_b128) per pair of MFMAs.
//   * k-tiles of 16 are register-staged (global_load_dwordx4: 8 lanes x 16 B = one full 128-B line
//     per row), written to a double-buffered padded LDS image (row stride 18 doubles: the 16
//     rows x 2 k-groups of a 32-lane LDS phase land on distinct banks), one barrier per k-tile.
//   * data-parallel + stream-K hybrid: whole tiles while they divide over the resident workgroups,
//     the remaining tiles' k-range in CHUNKS claimed through one device word (528 lower tiles at
//     m=4096 do not divide over 512 resident workgroups); a chunk's partial tile goes to a slab and
//     a second pass adds the slabs of a tile in chunk order -- deterministic, no data atomics.
//   * CANONICAL SUMMATION ORDER (A.D.A^T): the contraction is cut into chunks of kc k-tiles (256
//     columns up to n = 4096, the KC panel depth of the reference's dgemm -- matrixmultiply, whose
//     `C += A_panel . B_panel` per packed panel is restated in oracle/oracle_linalg.c); every chunk is
//     summed from zero in k order and the chunk sums are added in chunk order.  A data-parallel tile
//     flushes its accumulators into C at every chunk boundary, a stream-K chunk goes to its slab and
//     the fix-up adds the slabs in the same order: M has the same bits whatever the decomposition
//     (single LP, lockstep batch, any workgroup count), and the rounding error of a length-n sum is
//     that of a two-level sum, like the reference's, instead of a length-n running sum (measured on
//     the 256 C4 members: without it the lockstep path ended one-sidedly further from the vertex).
//   * workgroups are renumbered so that the 64 that share an XCD (and its L2) work on one
//     8x8 super-block of tiles: 16 row panels of A feed 64 tiles.
#include "gemm_tile.hpp"

namespace lpipm {

__device__ __forceinline__ int xcd_remap(int b, int n) {
    // blocks b and b+8 share an XCD (round-robin dispatch): give each XCD a contiguous range.
    const int xcd = b & 7, q = n >> 3, r = n & 7;
    return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (b >> 3);
}

// ---------------------------------------------------------------------------------------------------------
// A.D.A^T kernel.  128x128 workgroup tile, 512 threads = 2x4 waves of 64x32 (4x2 MFMA tiles, 32 fp64
// accumulators per lane), <= 128 VGPRs, so TWO such workgroups = 4 waves per SIMD are resident per CU.
// Why 8 waves: with 2 waves per SIMD (the first version: 4 waves of 64x64 per workgroup) a wave's non-MFMA phase of a
// k-tile (issue the prefetch, ds_read the fragments, scale + ds_write the next k-tile, barrier: ~4000 cycles under
// contention, s_memtime stamps) is as long as its partner's MFMA phase (64 x 64 cycles), so the two can only just
// cover each other (measured 87 % MFMA-busy); with 4 waves per SIMD each wave issues 32 MFMAs per k-tile and has
// three partners' 6144 cycles of cover (93 %).
//
// chunk_end(q) is called when the k-tile that ends chunk q (kc k-tiles, counted from k-tile 0) has been
// accumulated and more k-tiles follow: the caller flushes and clears the accumulators there, while the software
// pipeline (next k-tile already in LDS) keeps running.
// Addressing: buffer loads.  A tile's row panel is one buffer resource (wave-uniform origin in SGPRs), the k advance
// and the +64-row step go into the scalar offset, and a lane contributes ONE 32-bit byte offset (its staging row and
// column): the five loads of a k-tile cost one VGPR of addresses instead of ten.  At 128 VGPRs per wave (4 waves per
// SIMD) every register the compiler spills inside this loop puts an `s_waitcnt vmcnt(0)` in front of the prefetch it
// has just issued.  (A panel of 128 rows must stay below 4 GiB: ld < 4M columns, checked at launch.)
typedef unsigned int u4v __attribute__((ext_vector_type(4)));
typedef unsigned int u2v __attribute__((ext_vector_type(2)));
__device__ __forceinline__ __amdgpu_buffer_rsrc_t make_rsrc(const void* base, unsigned bytes) {
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(base), 0, (int)bytes, 0x00020000);
}
__device__ __forceinline__ d2 buf_load_d2(__amdgpu_buffer_rsrc_t r, unsigned voff, unsigned soff) {
    return __builtin_bit_cast(d2, __builtin_amdgcn_raw_buffer_load_b128(r, (int)voff, (int)soff, 0));
}
__device__ __forceinline__ double buf_load_d(__amdgpu_buffer_rsrc_t r, unsigned voff, unsigned soff) {
    return __builtin_bit_cast(double, __builtin_amdgcn_raw_buffer_load_b64(r, (int)voff, (int)soff, 0));
}
__device__ __forceinline__ void buf_store_d(__amdgpu_buffer_rsrc_t r, unsigned voff, unsigned soff, double v) {
    __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(u2v, v), r, (int)voff, (int)soff, 0);
}
// the same with a cache-policy operand (16 = sc1: write-through / L1-bypassing, see the units kernel).  The value goes
// through a by-value double: a bit_cast written directly on `acc[mi][nj][r]` inside the unrolled loops stored element 0
// of the accumulator quad for every r (hipcc 7.2, seen on the GPU: rows fq + 4r, r > 0, received row fq's values).
template <int AUX>
__device__ __forceinline__ void buf_store_d_aux(__amdgpu_buffer_rsrc_t r, unsigned voff, unsigned soff, double v) {
    __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(u2v, v), r, (int)voff, (int)soff, AUX);
}
template <int AUX>
__device__ __forceinline__ void buf_store_d2_aux(__amdgpu_buffer_rsrc_t r, unsigned voff, unsigned soff, d2 v) {
    __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u4v, v), r, (int)voff, (int)soff, AUX);
}
template <int AUX>
__device__ __forceinline__ d2 buf_load_d2_aux(__amdgpu_buffer_rsrc_t r, unsigned voff, unsigned soff) {
    return __builtin_bit_cast(d2, __builtin_amdgcn_raw_buffer_load_b128(r, (int)voff, (int)soff, AUX));
}

// Diagonal tiles of a symmetric product (A.D.A^T): wave (wr, wc) of the 2 x 4 layout owns the 16x16 blocks with block row
// 4 wr + mi and block column 2 wc + nj of the tile; a block is strictly above the diagonal when its column index exceeds
// its row index, i.e. d + nj > mi with d = 2 wc - 4 wr.  Patterns: 0 nothing skipped (d <= -2), 1 (d = 0), 2 (d = 2),
// 3 everything (d >= 4).  28 of a diagonal tile's 64 blocks go: 3 % of the MFMA work at 4096x8192, 11 % at 1024x2048.
__device__ __forceinline__ int diag_pattern(int wr, int wc) {
    const int d = 2 * wc - 4 * wr;
    return d < 0 ? 0 : (d == 0 ? 1 : (d == 2 ? 2 : 3));
}
// Which 64 x 32 part of the tile wave w takes.  Waves w and w + 4 share a SIMD (a 512-thread workgroup's waves go round the
// four SIMDs), and a workgroup advances at the pace of its busiest SIMD (one barrier per k-tile), so on a diagonal tile the
// blocks left (7, 3, 0, 0 / 8, 8, 7, 3 of 8 for wc = 0..3 in rows wr = 0 / 1) are paired to 8, 8, 10, 10 per SIMD.
__device__ __forceinline__ void wave_part(int wave, int& wr, int& wc) {
    wr = (0x4B >> wave) & 1;             // w: 0 1 2 3 4 5 6 7 -> wr 1 1 0 1 0 0 1 0
    wc = (0x7E84 >> (2 * wave)) & 3;     //                       wc 0 1 0 2 2 3 3 1
}
// the first pattern that leaves block (mi, nj) out: the block is issued while the wave's pattern is below it
__device__ __forceinline__ constexpr int diag_group(int mi, int nj) {
    return nj > mi ? 1 : (2 + nj > mi ? 2 : 3);
}

// f.template operator()<PAT>() for the wave-uniform pattern `pat`
template <typename F> __device__ __forceinline__ void diag_dispatch(int pat, F&& f) {
    if (pat == 0) f.template operator()<0>();
    else if (pat == 1) f.template operator()<1>();
    else if (pat == 2) f.template operator()<2>();
    else f.template operator()<3>();
}

// One pass over the k-tiles [kb, ke) of a tile, in chunks that end at multiples of kc k-tiles (kc == 0: one chunk).
// The software pipeline (next k-tile prefetched into registers while the current one is multiplied out of LDS) runs
// across chunk boundaries; the hot inner loop is the plain k-tile loop and the chunk logic lives around it:
//   touch(first)  at the start of a chunk's last k-tile: may issue loads that pull the C tile towards L2
//   flush(first, last)  after a chunk's last k-tile: stores / adds the accumulators (the caller's business); the
//                 accumulators restart from zero if more chunks follow.
template <int PAT = 0, typename FL, typename TC>
__device__ __forceinline__ void tile_pass_w8(double (*ldsA)[TILE][LDS_STRIDE], double (*ldsB)[TILE][LDS_STRIDE],
                                             __amdgpu_buffer_rsrc_t Pr, unsigned p64, __amdgpu_buffer_rsrc_t Qr, unsigned q64,
                                             __amdgpu_buffer_rsrc_t Sr, unsigned offP, unsigned offQ, unsigned offS,
                                             int kb, int ke, d4 (&acc)[4][2],
                                             int srow, int scol, int wr, int wc, int fr, int fq, int kc, FL&& flush,
                                             TC&& touch) {
    d2 sa[2], sb[2], sv;
    auto gload = [&](int kt) {
        const unsigned ko = (unsigned)kt * (unsigned)(BK * sizeof(double));
        sv = buf_load_d2(Sr, offS, ko);
        sa[0] = buf_load_d2(Pr, offP, ko);
        sa[1] = buf_load_d2(Pr, offP, ko + p64);
        sb[0] = buf_load_d2(Qr, offQ, ko);
        sb[1] = buf_load_d2(Qr, offQ, ko + q64);
    };
    auto lstore = [&](int buf) {
#pragma unroll
        for (int r = 0; r < 2; ++r) *(d2*)&ldsA[buf][srow + 64 * r][lds_wcol(srow, scol)] = sa[r];
#pragma unroll
        for (int r = 0; r < 2; ++r) *(d2*)&ldsB[buf][srow + 64 * r][lds_wcol(srow, scol)] = sb[r] * sv;
    };
    // PAT > 0: the pass of a wave over a DIAGONAL tile of a symmetric product whose blocks of groups <= PAT (diag_group) lie
    // strictly above the diagonal and are left out -- nothing reads them.  A straight-line body per pattern: the caller
    // switches on the wave's pattern once per pass (diag_dispatch), every other tile runs PAT = 0.
    auto mfma_ktile = [&](int cur) {
        if constexpr (PAT < 3) {
#pragma unroll
            for (int round = 0; round < 2; ++round) {
                d2 a[4] = {}, b[2] = {};
                if (round == 0) __builtin_amdgcn_s_setprio(0);
#pragma unroll
                for (int mi = 0; mi < 4; ++mi)
                    if (diag_group(mi, 0) > PAT) a[mi] = *(const d2*)&ldsA[cur][wr * 64 + mi * 16 + fr][round * 8 + lds_rq(fr, fq)];
#pragma unroll
                for (int nj = 0; nj < 2; ++nj)
                    if (diag_group(3, nj) > PAT) b[nj] = *(const d2*)&ldsB[cur][wc * 32 + nj * 16 + fr][round * 8 + lds_rq(fr, fq)];
#pragma unroll
                for (int t = 0; t < 2; ++t)
#pragma unroll
                    for (int mi = 0; mi < 4; ++mi)
#pragma unroll
                        for (int nj = 0; nj < 2; ++nj)
                            if (diag_group(mi, nj) > PAT)
                                acc[mi][nj] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[mi][t], b[nj][t], acc[mi][nj], 0, 0, 0);
            }
        }
        __builtin_amdgcn_s_setprio(2);   // the short non-MFMA phase goes first: it is what the partners wait for
    };
    gload(kb);
    lstore(0);
    __syncthreads();
    int cur = 0, kt = kb;
    bool first = true;
    while (kt < ke) {
        int ce = ke;                                       // end of this chunk
        if (kc > 0) { const int e = (kt / kc + 1) * kc; ce = e < ke ? e : ke; }
        for (; kt < ce - 1; ++kt) {                        // the hot loop
            gload(kt + 1);
            mfma_ktile(cur);
            lstore(cur ^ 1);
            __syncthreads();
            cur ^= 1;
        }
        const bool more = ce < ke;                         // last k-tile of the chunk
        unsigned pf0 = 0, pf1 = 0;
        touch(first, pf0, pf1);                            // (before the prefetch: whatever its addresses need reloaded must
        if (more) gload(ce);                               //  not wait behind the loads issued here)
        mfma_ktile(cur);
        if (more) lstore(cur ^ 1);
        asm volatile("" :: "v"(pf0), "v"(pf1));            // the touch loads have landed (and their registers are free) from here
        flush(first, !more);
        if (more) acc_clear(acc);
        first = false;
        __syncthreads();
        cur ^= 1;
        kt = ce;
    }
    __builtin_amdgcn_s_setprio(0);
}

// Workgroup g of an LP:
//   phase 1 (data-parallel): tiles g, g + nwg, ... of the first ntiles_dp = floor(ntiles/nwg)*nwg tiles, whole k-range
//            each.  Every workgroup walks k from 0 in lockstep, so the ~64 workgroups of an XCD (one 8x8 super-block
//            of tiles) hit each other's A panels in that XCD's L2.  With a canonical chunk (p.kc) the accumulators
//            are added into the C tile at every chunk boundary and restart from zero.
//   phase 2 (stream-K): the remaining tiles' k-range in chunks of p.sk k-tiles, claimed through one
//            device word per LP: the data-parallel tiles do not all finish together (stamps at C3: 1876 .. 2025 us
//            after launch), so chunks go to whoever is free.  Slab c holds chunk c; gemm_nt_fixup_kernel adds a
//            tile's slabs in chunk order -- the same sums in the same order as phase 1's flushes.
struct Round2K {
    const double* A; long long lda;
    const double* s;          // dinv: per-k scale applied to the second panel while staging
    double* C; long long ldc;
    int KT;
    int ntiles;
    const int2* tile_list;    // (ti, tj) per tile (device pointer, shared by a batch)
    int diag_pad_from;        // rows/cols >= this on the diagonal are written as 1.0 (-1: off)
    double* ws;               // chunk slabs of the remainder tiles: round2_slabs() tiles of TILE*TILE doubles
    int nwg;                  // workgroups launched per LP
    unsigned int* sk_claim;   // the device word through which the chunks of the remainder tiles are claimed (workgroups that finish
                              //   their data-parallel tiles early take more of them); slabs are indexed by chunk, so the sums do
                              //   not depend on who computed what
    int kc;                   // summation chunk of a data-parallel tile in k-tiles (0: plain running sum over the whole k-range)
    int sk;                   // stream-K unit in k-tiles (== kc up to KT = 256: one canonical chunking for every tile)
    double* C2;               // nullable: the final value of every tile is stored here too (same ldc)
    BatchK bk;
    long long astride;        // bytes between the members' A: bk.stride, or 0 for the A a batch shares
};
// LP blockIdx.z of a lockstep batch: per-LP pointers shifted (the tile list is shared)
__device__ __forceinline__ Round2K batch_shift(const Round2K& p0) {
    Round2K p = p0;
    p.A = (const double*)((const char*)p0.A + batch_lp(p0.bk) * p0.astride);
    p.s = batch_ptr(p0.s, p0.bk);
    p.C = batch_ptr(p0.C, p0.bk); p.ws = batch_ptr(p0.ws, p0.bk); p.sk_claim = batch_ptr(p0.sk_claim, p0.bk);
    p.C2 = batch_ptr(p0.C2, p0.bk);
    return p;
}
__global__ __launch_bounds__(512) __attribute__((amdgpu_waves_per_eu(4, 4))) void gemm_nt_streamk_w8_kernel(const Round2K p0) {
    if (batch_done(p0.bk)) return;
    const Round2K p = batch_shift(p0);
    __shared__ __attribute__((aligned(16))) double ldsA[2][TILE][LDS_STRIDE];
    __shared__ __attribute__((aligned(16))) double ldsB[2][TILE][LDS_STRIDE];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    int wr, wc;                                       // 2 x 4 waves: 64 rows x 32 columns each
    wave_part(wave, wr, wc);
    const int fr = lane & 15, fq = lane >> 4;
    const int srow = tid >> 3, scol = (tid & 7) * 2;  // staging: 64 rows per pass
    const int g = p.bk.xcd_major ? (int)blockIdx.y : xcd_remap(blockIdx.x, gridDim.x);
    const int KT = p.KT;
    const int ntiles_dp = (p.ntiles / p.nwg) * p.nwg;
    // C tile (ti, tj) as a buffer; this lane's element of MFMA block (mi, nj), register r sits at
    //   offC + ((mi*16 + 4r)*ldc + nj*16) * 8   (wave-uniform second term)
    const unsigned rowC = (unsigned)(p.ldc * (long long)sizeof(double));
    const unsigned offC = (unsigned)(wr * 64 + fq) * rowC + (unsigned)((wc * 32 + fr) * sizeof(double));
    auto c_rsrc = [&](int ti, int tj) { return make_rsrc(p.C + (long long)(ti * TILE) * p.ldc + tj * TILE, (unsigned)TILE * rowC); };
    auto store_tile = [&](const d4 (&acc)[4][2], int ti, int tj) {
        double* cb = p.C + (long long)(ti * TILE + wr * 64 + fq) * p.ldc + (tj * TILE + wc * 32 + fr);
        tile_store<4, 2>(cb, p.ldc, acc, 1.0, 0.0, p.diag_pad_from >= 0 && ti == tj, ti * TILE + wr * 64 + fq,
                         p.diag_pad_from, fr, fq, wc * 32 - wr * 64);
    };
    // C tile += chunk sum.  Two rounds of 16 values per lane: the registers of
    // the staging and fragment values, dead at this point, hold the C values on their way in.
    auto add_tile = [&](const d4 (&acc)[4][2], int ti, int tj, bool final_copy) {
        const __amdgpu_buffer_rsrc_t cr = c_rsrc(ti, tj);
        const __amdgpu_buffer_rsrc_t cr2 = make_rsrc((final_copy ? p.C2 : p.C) + (long long)(ti * TILE) * p.ldc + tj * TILE, (unsigned)TILE * rowC);
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            double cv[2][4][2];
#pragma unroll
            for (int m2 = 0; m2 < 2; ++m2)
#pragma unroll
                for (int r = 0; r < 4; ++r)
#pragma unroll
                    for (int nj = 0; nj < 2; ++nj)
                        cv[m2][r][nj] = buf_load_d(cr, offC, (unsigned)((2 * h + m2) * 16 + 4 * r) * rowC + nj * 128);
#pragma unroll
            for (int m2 = 0; m2 < 2; ++m2)
#pragma unroll
                for (int r = 0; r < 4; ++r)
#pragma unroll
                    for (int nj = 0; nj < 2; ++nj)
                    {
                        const double v = cv[m2][r][nj] + acc[2 * h + m2][nj][r];
                        buf_store_d(cr, offC, (unsigned)((2 * h + m2) * 16 + 4 * r) * rowC + nj * 128, v);
                        if (final_copy) buf_store_d(cr2, offC, (unsigned)((2 * h + m2) * 16 + 4 * r) * rowC + nj * 128, v);
                    }
        }
    };
    // Touches every 128-B line of this wave's 64 x 32 part of the C tile (lane l: row l, columns 0 and 16), one k-tile
    // before add_tile reads it: the tile was written a chunk ago and has left the L2 since (A streams through it), so
    // the flush would otherwise pay two memory round trips (~6.5 us per flush measured, ~1.5 with the lines in L2).
    auto touch_tile = [&](int ti, int tj, unsigned& pf0, unsigned& pf1) {
        const __amdgpu_buffer_rsrc_t cr = c_rsrc(ti, tj);
        const unsigned off = (unsigned)(wr * 64 + lane) * rowC + (unsigned)(wc * 32 * sizeof(double));
        pf0 = __builtin_amdgcn_raw_buffer_load_b32(cr, (int)off, 0, 0);
        pf1 = __builtin_amdgcn_raw_buffer_load_b32(cr, (int)off, 128, 0);
    };
    const unsigned rowA = (unsigned)(p.lda * (long long)sizeof(double));
    const unsigned offP = (unsigned)srow * rowA + (unsigned)(scol * sizeof(double));     // both panels are rows of A
    const unsigned offS = (unsigned)(scol * sizeof(double));
    const unsigned p64 = 64u * rowA;
    auto a_rsrc = [&](int t) { return make_rsrc(p.A + (long long)(t * TILE) * p.lda, (unsigned)TILE * rowA); };
    const __amdgpu_buffer_rsrc_t Sr = make_rsrc(p.s, (unsigned)KT * (unsigned)(BK * sizeof(double)));
    for (int tile = g; tile < ntiles_dp; tile += p.nwg) {
        const int ti = p.tile_list[tile].x, tj = p.tile_list[tile].y;
        d4 acc[4][2];
        acc_clear(acc);
        tile_pass_w8(ldsA, ldsB, a_rsrc(ti), p64, a_rsrc(tj), p64, Sr, offP, offP, offS, 0, KT, acc, srow, scol, wr, wc, fr, fq,
                            p.kc, [&](bool first, bool last) {
                                if (first) store_tile(acc, ti, tj); else add_tile(acc, ti, tj, last && p.C2 != nullptr);
                            },
                            [&](bool first, unsigned& pf0, unsigned& pf1) { if (!first) touch_tile(ti, tj, pf0, pf1); });
    }
    if (ntiles_dp == p.ntiles) return;
    __shared__ int s_claim;
    const int ch_tiles = p.sk;
    const int cpt = (KT + ch_tiles - 1) / ch_tiles;          // stream-K units per tile
    const int nchunks = (p.ntiles - ntiles_dp) * cpt;
    for (;;) {
        if (tid == 0) s_claim = (int)atomicAdd(p.sk_claim, 1u);
        __syncthreads();
        const int ch = __builtin_amdgcn_readfirstlane(s_claim);
        __syncthreads();
        if (ch >= nchunks) break;
        // chunk-major order: the units in flight together are the same k-range of different tiles, which share the
        // row panels of A in L2 (tile-major order would have every unit load two panels of its own)
        const int nrem = p.ntiles - ntiles_dp;
        const int q = ch / nrem, rt = ch - q * nrem;
        const int kb = q * ch_tiles, ke = kb + ch_tiles < KT ? kb + ch_tiles : KT;
        const int ti = p.tile_list[ntiles_dp + rt].x, tj = p.tile_list[ntiles_dp + rt].y;
        d4 acc[4][2];
        acc_clear(acc);
        tile_pass_w8(ldsA, ldsB, a_rsrc(ti), p64, a_rsrc(tj), p64, Sr, offP, offP, offS, kb, ke, acc, srow, scol, wr, wc, fr, fq,
                            0, [&](bool, bool) {
            if (cpt == 1) { store_tile(acc, ti, tj); return; }   // the chunk is the whole tile
            const __amdgpu_buffer_rsrc_t wr_ = make_rsrc(p.ws + ((long long)rt * cpt + q) * (TILE * TILE), (unsigned)(TILE * TILE * sizeof(double)));
            const unsigned offW = (unsigned)(((wr * 64 + fq) * TILE + wc * 32 + fr) * sizeof(double));
#pragma unroll
            for (int mi = 0; mi < 4; ++mi)
#pragma unroll
                for (int r = 0; r < 4; ++r)
#pragma unroll
                    for (int nj = 0; nj < 2; ++nj)
                        buf_store_d(wr_, offW, (unsigned)(((mi * 16 + 4 * r) * TILE + nj * 16) * sizeof(double)), acc[mi][nj][r]);
        }, [](bool, unsigned&, unsigned&) {});
    }
}

// Adds the chunk slabs of every stream-K (remainder) tile in chunk order.  grid = remainder tiles x FIX_SPLIT:
// a tile can have dozens of slabs, so its 16K elements are spread over FIX_SPLIT workgroups (8 rows each) to
// keep this pass off the critical path.
constexpr int FIX_SPLIT = 16;
__global__ __launch_bounds__(256) void gemm_nt_fixup_kernel(const Round2K p0) {
    if (batch_done(p0.bk)) return;
    const Round2K p = batch_shift(p0);
    const int ntiles_dp = (p.ntiles / p.nwg) * p.nwg;
    const int bx = p.bk.xcd_major ? (int)blockIdx.y : (int)blockIdx.x;
    const int rt = bx / FIX_SPLIT, part = bx % FIX_SPLIT;
    const int cpt = (p.KT + p.sk - 1) / p.sk;                // slabs [rt*cpt, (rt+1)*cpt), one per stream-K unit
    const int ti = p.tile_list[ntiles_dp + rt].x, tj = p.tile_list[ntiles_dp + rt].y;
    constexpr int PER = TILE * TILE / FIX_SPLIT;
    const double* slab0 = p.ws + (long long)rt * cpt * (TILE * TILE);
    for (int e = part * PER + threadIdx.x * 2; e < (part + 1) * PER; e += 512) {
        d2 sum = *(const d2*)(slab0 + e);
        for (int q = 1; q < cpt; ++q) sum += *(const d2*)(slab0 + (long long)q * (TILE * TILE) + e);
        const int r = e / TILE, c = e - r * TILE;
        const int row = ti * TILE + r, col = tj * TILE + c;
        double* cp = p.C + (long long)row * p.ldc + col;
        d2 v = sum;
        if (p.diag_pad_from >= 0) {
            if (row == col && row >= p.diag_pad_from) v[0] = 1.0;
            if (row == col + 1 && row >= p.diag_pad_from) v[1] = 1.0;
        }
        *(d2*)cp = v;
        if (p.C2) *(d2*)(p.C2 + (long long)row * p.ldc + col) = v;
    }
}

// ---------------------------------------------------------------------------------------------------------
// A.D.A^T as (tile, chunk) UNITS with an in-launch combine.
// The contraction of every lower tile is cut into the canonical chunks (units_chunking); a workgroup computes `upc`
// consecutive chunks of ONE tile, writes each chunk sum to that chunk's slab (write-through stores: nothing to wait for),
// and adds the number of chunks it did to the tile's arrival counter.  The workgroup whose add completes the tile adds the
// tile's slabs IN CHUNK ORDER and stores the tile -- the same sums in the same order as a single running pass that flushes
// at every chunk boundary, whatever the decomposition (no separate fix-up launch; the bits of M do not depend on the
// workgroup count, on `upc`, or on who arrives last).  A non-persistent grid, one unit per workgroup, dispatched in list
// order: with a column-group-major list the groups of M complete one after the other WHILE the launch runs, and the
// workgroup that completes a group's last tile bumps that group's word -- what the column-split reduction of M waits for
// (launch_adat with signal_groups).
// Hand-off protocol (MI355X_MICROARCH.md, Workgroup dispatch / inter-workgroup visibility; cdna_hip_programming.md
// Guideline 16 in its counter form): per-XCD L2s are not coherent, so
//   producer : slab stores are WRITE-THROUGH (sc1) -> every storing wave s_waitcnt vmcnt(0) -> workgroup barrier ->
//              ONE lane adds to the tile's counter (relaxed, agent scope);
//   consumer : the workgroup whose add completed the tile (told by the value the add returned) -> that lane's
//              agent-scope acquire + s_waitcnt vmcnt(0) -> workgroup barrier -> EVERY load of the slabs is an sc1 load.
// The finished tile of M is stored write-through as well when group words are signalled: its readers are other
// kernels (the column-split reduction of M, on another stream) that start while this launch is still running -- their
// kernel-start acquire drops stale lines, but nothing would write this XCD's dirty lines back before this launch ends.
constexpr int AUX_SC1 = 16;
struct UnitsK {
    const double* A; long long lda;
    const double* s;
    double* C; long long ldc;
    double* C2;
    int KT, kc, cpt;
    int nbig, ks;             // chunk q covers k-tiles [q*kc, (q+1)*kc) for q < nbig, then pieces of ks k-tiles (units_chunking)
    int ntiles;
    const int2* tile_list;
    const int2* unit_list;
    int nunits, upc;
    int diag_pad_from;
    double* slabs;
    unsigned int* tile_cnt;
    unsigned int* grp_cnt;
    int grp_w;
    BatchK bk;
    long long astride;        // bytes between the members' A: bk.stride, or 0 for the A a batch shares
};
template <bool GRP>
__global__ __launch_bounds__(512) __attribute__((amdgpu_waves_per_eu(4, 4))) void gemm_nt_units_kernel(const UnitsK p0) {
    if (batch_done(p0.bk)) return;
    UnitsK p = p0;
    p.A = (const double*)((const char*)p0.A + batch_lp(p0.bk) * p0.astride);
    p.s = batch_ptr(p0.s, p0.bk); p.C = batch_ptr(p0.C, p0.bk); p.C2 = batch_ptr(p0.C2, p0.bk);
    p.slabs = batch_ptr(p0.slabs, p0.bk); p.tile_cnt = batch_ptr(p0.tile_cnt, p0.bk); p.grp_cnt = batch_ptr(p0.grp_cnt, p0.bk);
    __shared__ __attribute__((aligned(16))) double ldsA[2][TILE][LDS_STRIDE];
    __shared__ __attribute__((aligned(16))) double ldsB[2][TILE][LDS_STRIDE];
    __shared__ unsigned int s_old;
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    int wr, wc;                                       // 2 x 4 waves: 64 rows x 32 columns each
    wave_part(wave, wr, wc);
    const int fr = lane & 15, fq = lane >> 4;
    const int srow = tid >> 3, scol = (tid & 7) * 2;  // staging: 64 rows per pass
    const int b = p.bk.xcd_major ? (int)blockIdx.y : (int)blockIdx.x;
    const int2 un = p.unit_list[b];          // the list is already dealt to the XCDs (deal_units)
    const int tile = un.x, q0 = un.y;
    if (tile < 0) return;                    // padding of an XCD's shorter list
    const int q1 = q0 + p.upc < p.cpt ? q0 + p.upc : p.cpt;
    const int2 tc = p.tile_list[tile];
    const int ti = tc.x, tj = tc.y;
    const int KT = p.KT;
    const unsigned rowA = (unsigned)(p.lda * (long long)sizeof(double));
    const unsigned offP = (unsigned)srow * rowA + (unsigned)(scol * sizeof(double));
    const unsigned offS = (unsigned)(scol * sizeof(double));
    const unsigned p64 = 64u * rowA;
    const __amdgpu_buffer_rsrc_t Pr = make_rsrc(p.A + (long long)(ti * TILE) * p.lda, (unsigned)TILE * rowA);
    const __amdgpu_buffer_rsrc_t Qr = make_rsrc(p.A + (long long)(tj * TILE) * p.lda, (unsigned)TILE * rowA);
    const __amdgpu_buffer_rsrc_t Sr = make_rsrc(p.s, (unsigned)KT * (unsigned)(BK * sizeof(double)));
    // this tile's slabs as ONE buffer: slab q at byte q * 128 KiB
    constexpr unsigned SLAB_BYTES = (unsigned)(TILE * TILE * sizeof(double));
    const __amdgpu_buffer_rsrc_t Wr = make_rsrc(p.slabs + (long long)tile * p.cpt * (TILE * TILE), (unsigned)p.cpt * SLAB_BYTES);
    d4 acc[4][2];
    acc_clear(acc);
    // chunk boundaries: nbig chunks of kc k-tiles, the rest of the contraction in pieces of ks
    auto chunk_begin = [&](int q) { const int b0 = q <= p.nbig ? q * p.kc : p.nbig * p.kc + (q - p.nbig) * p.ks; return b0 < KT ? b0 : KT; };
    const int kb = chunk_begin(q0), ke = chunk_begin(q1);
    const int dpat = ti == tj ? diag_pattern(wr, wc) : 0;
    if (p.cpt == 1) {
        // a contraction of one chunk: the unit is the whole tile, stored directly
        diag_dispatch(dpat, [&]<int PAT>() {
            tile_pass_w8<PAT>(ldsA, ldsB, Pr, p64, Qr, p64, Sr, offP, offP, offS, 0, KT, acc, srow, scol, wr, wc, fr, fq, 0,
                                    [&](bool, bool) {}, [](bool, unsigned&, unsigned&) {});
        });
        const unsigned rowC = (unsigned)(p.ldc * (long long)sizeof(double));
        const unsigned offC = (unsigned)(wr * 64 + fq) * rowC + (unsigned)((wc * 32 + fr) * sizeof(double));
        const __amdgpu_buffer_rsrc_t cr = make_rsrc(p.C + (long long)(ti * TILE) * p.ldc + tj * TILE, (unsigned)TILE * rowC);
        const __amdgpu_buffer_rsrc_t cr2 = make_rsrc((p.C2 ? p.C2 : p.C) + (long long)(ti * TILE) * p.ldc + tj * TILE, (unsigned)TILE * rowC);
        const bool pad = p.diag_pad_from >= 0 && ti == tj;
        const int row0 = ti * TILE + wr * 64 + fq, dd = wc * 32 - wr * 64;
#pragma unroll
        for (int mi = 0; mi < 4; ++mi)
#pragma unroll
            for (int r = 0; r < 4; ++r)
#pragma unroll
                for (int nj = 0; nj < 2; ++nj) {
                    double v = acc[mi][nj][r];
                    if (pad && (mi - nj) * 16 + fq + 4 * r - fr == dd && row0 + mi * 16 + 4 * r >= p.diag_pad_from) v = 1.0;
                    const unsigned so = (unsigned)(mi * 16 + 4 * r) * rowC + nj * 128;
                    buf_store_d_aux<GRP ? AUX_SC1 : 0>(cr, offC, so, v);
                    if (p.C2) buf_store_d_aux<0>(cr2, offC, so, v);
                }
    } else {
        int q = q0;
        const unsigned offW = (unsigned)(((wr * 64 + fq) * TILE + wc * 32 + fr) * sizeof(double));
        diag_dispatch(dpat, [&]<int PAT>() {
        tile_pass_w8<PAT>(ldsA, ldsB, Pr, p64, Qr, p64, Sr, offP, offP, offS, kb, ke, acc, srow, scol, wr, wc, fr, fq, p.kc,
                           [&](bool, bool) {
                               const unsigned sb = (unsigned)q * SLAB_BYTES;
#pragma unroll
                               for (int mi = 0; mi < 4; ++mi)
#pragma unroll
                                   for (int r = 0; r < 4; ++r)
#pragma unroll
                                       for (int nj = 0; nj < 2; ++nj)
                                           buf_store_d_aux<AUX_SC1>(Wr, offW, sb + (unsigned)(((mi * 16 + 4 * r) * TILE + nj * 16) * sizeof(double)),
                                                                    acc[mi][nj][r]);
                               ++q;
                           },
                           [](bool, unsigned&, unsigned&) {});
        });
        // publish: every storing wave drains its stores, then ONE lane adds this unit's chunks to the tile's counter
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        if (tid == 0) s_old = __hip_atomic_fetch_add(p.tile_cnt + tile, (unsigned)(q1 - q0), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __syncthreads();
        if ((int)s_old + (q1 - q0) != p.cpt) return;           // not the last arriver of this tile (workgroup-uniform)
        if (tid == 0) {
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            // every arrival of this launch is in: the word goes back to zero for the next launch (the host then needs no
            // memset per launch; with group words the consumers on other streams make the host clear both kinds)
            if (!GRP) __hip_atomic_store(p.tile_cnt + tile, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        __syncthreads();
        // combine: slabs 0 .. cpt-1 added in chunk order; a thread owns 16 pairs of adjacent elements, 1024 elements apart
        const unsigned rowC = (unsigned)(p.ldc * (long long)sizeof(double));
        const __amdgpu_buffer_rsrc_t cr = make_rsrc(p.C + (long long)(ti * TILE) * p.ldc + tj * TILE, (unsigned)TILE * rowC);
        const __amdgpu_buffer_rsrc_t cr2 = make_rsrc((p.C2 ? p.C2 : p.C) + (long long)(ti * TILE) * p.ldc + tj * TILE, (unsigned)TILE * rowC);
        const unsigned voff = (unsigned)tid * 16u;
        const int cpt = p.cpt;
        for (int i = 0; i < 16; i += 2) {
            d2 sum[2];
#pragma unroll
            for (int a = 0; a < 2; ++a)
                sum[a] = buf_load_d2_aux<AUX_SC1>(Wr, voff, (unsigned)(i + a) * 8192u);
            for (int qb = 1; qb < cpt; qb += 4) {
                d2 v[2][4];
#pragma unroll
                for (int j = 0; j < 4; ++j)
#pragma unroll
                    for (int a = 0; a < 2; ++a)
                        if (qb + j < cpt)
                            v[a][j] = buf_load_d2_aux<AUX_SC1>(Wr, voff, (unsigned)(qb + j) * SLAB_BYTES + (unsigned)(i + a) * 8192u);
#pragma unroll
                for (int j = 0; j < 4; ++j)
#pragma unroll
                    for (int a = 0; a < 2; ++a)
                        if (qb + j < cpt) sum[a] += v[a][j];
            }
#pragma unroll
            for (int a = 0; a < 2; ++a) {
                const int e = tid * 2 + (i + a) * 1024;
                const int r = e >> 7, c = e & 127;
                const int row = ti * TILE + r, col = tj * TILE + c;
                d2 v = sum[a];
                if (p.diag_pad_from >= 0 && ti == tj) {
                    if (row == col && row >= p.diag_pad_from) v[0] = 1.0;
                    if (row == col + 1 && row >= p.diag_pad_from) v[1] = 1.0;
                }
                const unsigned co = (unsigned)r * rowC + (unsigned)(c * sizeof(double));
                buf_store_d2_aux<GRP ? AUX_SC1 : 0>(cr, co, 0u, v);
                if (p.C2) buf_store_d2_aux<0>(cr2, co, 0u, v);
            }
        }
    }
    if (GRP) {   // this tile of M is complete: drain its (write-through) stores, then count it in its column group's word
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        if (tid == 0) (void)__hip_atomic_fetch_add(p.grp_cnt + tj / p.grp_w, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// The device-side wait of a stream: see launch_wait_count.
__global__ __launch_bounds__(64) void wait_count_kernel(const unsigned int* cnt, unsigned int target, const int* done,
                                                        unsigned int* timeout) {
    if (threadIdx.x != 0) return;
    if (done && __hip_atomic_load(done, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0) return;   // the producer returned at once
    for (unsigned int spins = 0; spins < (1u << 21); ++spins) {        // ~1 us per poll: gives up after a few seconds
        if (__hip_atomic_load(cnt, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >= target) return;
        __builtin_amdgcn_s_sleep(16);
    }
    __hip_atomic_store(timeout, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// ---------------------------------------------------------------------------------------------------------
// Host side: chunking rules, the plan, the resources, the launch.
//
// Canonical chunk of the A.D.A^T contraction in k-tiles: 128 columns up to n = 1024 (a small LP has few tiles: more,
// shorter stream-K units fill more CUs), 256 columns (the reference dgemm's KC) up to n = 4096, 1024 columns above.
// A data-parallel tile's flush is a read-modify-write of its C tile (~10 us, and 256 KB of fabric traffic); measured at
// C3 on one box, per launch and distance of the solve's x from the planted vertex:
//   one running sum 5.5e-7 | 1024 columns 2.27 ms, 1.2e-7 | 512 columns 2.34 ms, 7.9e-8 | 256 columns 2.55 ms, 6.3e-8
// (the oracle itself: 6.3e-8).
static int canonical_chunk(int KT) { return KT <= 64 ? 8 : (KT <= 256 ? 16 : 64); }
// Stream-K unit of the round-2 kernel for a contraction of KT k-tiles: the canonical chunk up to KT = 256 (ONE chunking for
// data-parallel and stream-K tiles: M's bits do not depend on the decomposition -- the sizes that run both alone and as
// lockstep batches); above, 16 k-tiles whatever the data-parallel chunk: the launch ends one unit after the ideal time at
// best, and a unit of 64 k-tiles is 0.24 ms (C3: the 16 stream-K tiles cost 0.25 ms for 3 % of the work).  Those tiles are
// then summed in finer blocks than the data-parallel ones (same determinism, the decomposition-independence is given up for
// big LPs).
static int round2_unit(int KT) {
    const int kc = canonical_chunk(KT);
    return KT <= 256 ? kc : (kc < 16 ? kc : 16);
}
// stream-K units per tile (1: no split, the tile is one running sum)
static int round2_cpt(int KT) {
    if (KT <= canonical_chunk(KT)) return 1;
    const int u = round2_unit(KT);
    return (KT + u - 1) / u;
}
// workgroup count of the round-2 kernel for ntiles x KT work on num_cu CUs
static int round2_nwg(int ntiles, int KT, int num_cu) {
    const int cpt = round2_cpt(KT);
    const long long units = (long long)ntiles * cpt;   // (tile, unit) work items
    long long nwg = 2LL * num_cu;              // 2 resident workgroups per CU
    if (nwg > units) nwg = units;
    if (nwg < 1) nwg = 1;
    return (int)nwg;
}
// ... and the number of TILE x TILE slabs its remainder tiles need for that workgroup count
static size_t round2_slabs(int ntiles, int KT, int nwg) {
    const int cpt = round2_cpt(KT);
    const int nrem = ntiles - (ntiles / nwg) * nwg;
    return cpt > 1 ? (size_t)nrem * cpt : 0;
}

// The canonical chunking of the A.D.A^T contraction in the units kernel.  Up to KT = 256 k-tiles (n <= 4096): uniform chunks
// of canonical_chunk(KT) -- the chunking of the round-2 kernel, so that an LP gets the same bits from either (the sizes
// that run alone and as lockstep batches).  Above: chunks of 64 k-tiles (1024 columns), except that the LAST 64 are cut
// into pieces of 16: units are dispatched in chunk order, so the launch ends on quarter-size units -- with 4224 equal units
// on 512 slots the last quarter-full round of 0.25 ms units cost 0.19 ms of a 2.3 ms launch.
// Returns the chunks per tile; chunk q covers k-tiles [q*kc, (q+1)*kc) for q < nbig, then pieces of ks k-tiles.
static int units_chunking(int K, int* kc_out, int* nbig_out, int* ks_out) {
    const int KT = K / BK, kc = canonical_chunk(KT);
    int nbig, ks, cpt;
    if (KT <= kc) { nbig = 1; ks = kc; cpt = 1; }
    else if (KT <= 256 || kc < 32) { ks = kc; cpt = (KT + kc - 1) / kc; nbig = cpt; }
    else {
        nbig = KT / kc - 1;                 // full chunks but the last one
        ks = kc / 4;
        cpt = nbig + (KT - nbig * kc + ks - 1) / ks;
    }
    *kc_out = kc; *nbig_out = nbig; *ks_out = ks;
    return cpt;
}
constexpr int UNITS_MAX_CPT = 256;   // most chunks per tile the units kernel takes (a tile's slabs are one 32-bit buffer)

AdatPlan plan_adat(int mp, int npa, int count, int num_cu, int world, int units_env) {
    AdatPlan a;
    const int nt = mp / TILE;
    a.ntiles = nt * (nt + 1) / 2;
    // workgroups per LP of the round-2 A.D.A^T launch (LPIPM_ADAT_UNITS=0, and contractions whose slabs would not fit):
    // stream-K over the chip's share of one LP; a batch that fills the chip with whole tiles needs no k-split
    if (count == 1) a.nwg = round2_nwg(a.ntiles, npa / BK, num_cu);
    else if ((long long)count * a.ntiles >= 2LL * num_cu) {
        // more tiles than resident workgroups: each LP gets its share of the 2*CUs slots and stream-K
        // balances its tiles over them (no tail round of a few leftover tiles)
        a.nwg = 2 * num_cu / count;
        if (a.nwg < 1) a.nwg = 1;
        if (a.nwg > a.ntiles) a.nwg = a.ntiles;
    } else {
        a.nwg = round2_nwg(a.ntiles, npa / BK, num_cu / count);
        if (a.nwg < a.ntiles) a.nwg = a.ntiles;
    }
    a.slabs = round2_slabs(a.ntiles, npa / BK, a.nwg);
    // A.D.A^T as (tile, chunk) units: every chunk sum goes through its own slab (ntiles x cpt slabs of 128 KiB per LP:
    // 0.55 GB at C3, 38 MB per member at C4) -- up to 4 GiB per LP, beyond that (m = 16384: 34 GB) the round-2 kernel
    // -- and only up to UNITS_MAX_CPT chunks per tile (npa up to ~256000 columns): longer rows take the round-2 kernel too
    int kc, nbig, ks;
    a.cpt = units_chunking(npa, &kc, &nbig, &ks);
    const bool units_fit = a.cpt <= UNITS_MAX_CPT;
    a.units = units_env != 0 && units_fit && (size_t)a.ntiles * a.cpt * TILE * TILE * sizeof(double) <= ((size_t)4 << 30) &&
               (count > 1 || units_env == 2 || a.cpt == 1 || a.ntiles <= 16 || a.ntiles * a.cpt >= 256);
    // (tiny single LPs -- up to 16 tiles -- : one launch and one memset less, 0.042 vs 0.045 ms at 512x1024;
    //  a single LP with few tiles AND several chunks under 256 units -- 700x1500: 21 tiles x 6, 1009x1100: 36 tiles x 5; not
    //  1000x5000, whose 36 tiles x 11 chunks are 396 units -- keeps the round-2 kernel: one workgroup per
    //  tile adding the slabs at the end of a launch that never filled the chip costs more than the 16-way fix-up launch,
    //  0.196 vs 0.151 ms; everywhere else the units kernel is level or ahead -- 4096x8192 2.206 vs 2.22 ms inside a solve,
    //  2048x16384 1.30 vs 1.60 -- carries no spill and leaves out the blocks above the diagonal of the diagonal tiles)
    // one LP split by columns over ranks: the units kernel signals M's column groups one by one, and each group's cross-rank
    // sum runs behind the rest of the launch (the caller's consumer, see launch_adat); its slabs may take up to 32 GiB there
    // (C5: 17 GB per rank)
    if (count == 1 && world > 1 && units_env != 0 && units_fit && nt <= 64 * POTRF_OUTER &&
        (size_t)a.ntiles * a.cpt * TILE * TILE * sizeof(double) <= ((size_t)32 << 30)) a.units = true;
    a.grouped = count == 1 && world > 1 && a.units && nt >= 1 && nt <= 64 * POTRF_OUTER;
    // a single LP: one chunk per unit (parallelism, and column groups that complete while the launch runs); a lockstep
    // batch: two chunks per unit -- whole tiles (one unit = all chunks, its own workgroup adds its slabs) leave the last of
    // 2.25 rounds of tiles a quarter full (C4 shard: 1633 LP/s, against 1706 with one chunk per unit, 1533 / 1521 / 1521 at
    // 2 / 1 / 4 chunks on a slower box)
    a.upc = count == 1 ? 1 : (a.cpt < 2 ? a.cpt : 2);
    if (a.cpt != nbig) a.upc = 1;            // non-uniform chunks: one per unit
    if (a.units && a.slabs < (size_t)a.ntiles * a.cpt) a.slabs = (size_t)a.ntiles * a.cpt;
    return a;
}

void adat_take(AdatRes& r, const AdatPlan& plan, Arena& ar) {
    r.claim = ar.take<unsigned int>(1);
    // arrival counters of the units kernel: one word per tile, then one per column group; cleared by ONE memset per launch
    // (a block of its own, a multiple of 16 bytes)
    r.counter_bytes = (size_t)round_up(((size_t)plan.ntiles + 64) * sizeof(unsigned int), 16);
    r.counters = (unsigned int*)ar.take<uint4>(r.counter_bytes / 16);
    r.group_words = r.counters + plan.ntiles;
    r.wait_timeout = ar.take<unsigned int>(4);
    // chunk slabs (units kernel: every chunk of every tile; round-2 kernel: the stream-K remainder tiles)
    r.slabs = ar.take<double>(plan.slabs * TILE * TILE);
}

// Order in which the lower-triangular 128x128 tiles of M are handed to workgroups.  Workgroups are
// renumbered so that 64 consecutive tiles run on one XCD (one L2): full off-diagonal 8x8 super-blocks
// come first, each exactly one such chunk (16 row panels of A feed 64 tiles); the triangular
// diagonal super-blocks (36 tiles each) follow and are the ones that straddle chunk boundaries.
static std::vector<int2> tile_order(int nt) {
    std::vector<int2> v;
    v.reserve((size_t)nt * (nt + 1) / 2);
    const int ns = (nt + 7) / 8;
    auto emit = [&](int SI, int SJ) {
        for (int ti = SI * 8; ti < nt && ti < SI * 8 + 8; ++ti)
            for (int tj = SJ * 8; tj < SJ * 8 + 8 && tj <= ti; ++tj) v.push_back(make_int2(ti, tj));
    };
    for (int SI = 0; SI < ns; ++SI)
        for (int SJ = 0; SJ < SI; ++SJ) emit(SI, SJ);
    for (int SI = 0; SI < ns; ++SI) emit(SI, SI);
    return v;
}
// The same tiles ordered for a consumer of M's column groups: column group g (tile columns 4g .. 4g+3, one outer panel of
// the factorisation) is one contiguous sub-list; inside it row by row.
static std::vector<int2> tile_order_grouped(int nt, std::vector<int>& off, std::vector<int>& cnt) {
    std::vector<int2> v;
    for (int g = 0; g * POTRF_OUTER < nt; ++g) {
        off.push_back((int)v.size());
        const int c0 = g * POTRF_OUTER, c1 = c0 + POTRF_OUTER < nt ? c0 + POTRF_OUTER : nt;
        for (int ti = c0; ti < nt; ++ti)
            for (int tj = c0; tj < c1 && tj <= ti; ++tj) v.push_back(make_int2(ti, tj));
        cnt.push_back((int)v.size() - off.back());
    }
    return v;
}
// The unit list of a single LP's launch, dealt to the XCDs.  Workgroup b of a launch runs on XCD b % 8 (round-robin
// dispatch), so entry b of the list belongs to XCD b % 8: every XCD gets its OWN tiles (full rounds of 512 tiles: 64
// consecutive tiles of the order = one 8 x 8 super-block sharing 16 row panels of A; the rest in contiguous eighths) and
// walks them chunk by chunk -- the workgroups resident on one XCD (one L2) are one k-range of neighbouring tiles for the
// whole launch, like the data-parallel phase of the round-2 kernel.  Shorter lists are padded with no-op entries.
// Tiles [first, first + nt) of the launch's tile list, in its order; chunks q0, q0 + upc, ... < cpt per tile.
static void deal_units(int first, int nt, int cpt, int upc, std::vector<int2>& out) {
    std::vector<int> own[8];
    const int full = nt / 512 * 512, rest = nt - full;
    for (int i = 0; i < full; ++i) own[(i % 512) / 64].push_back(first + i);
    for (int x = 0; x < 8; ++x)
        for (int i = full + (int)((long long)rest * x / 8); i < full + (int)((long long)rest * (x + 1) / 8); ++i) own[x].push_back(first + i);
    size_t longest = 0;
    for (int x = 0; x < 8; ++x) longest = own[x].size() > longest ? own[x].size() : longest;
    const int nq = (cpt + upc - 1) / upc;
    for (int q = 0; q < nq; ++q)                           // chunk-major inside an XCD's list
        for (size_t i = 0; i < longest; ++i)
            for (int x = 0; x < 8; ++x)
                out.push_back(i < own[x].size() ? make_int2(own[x][i], q * upc) : make_int2(-1, 0));
}

void adat_lists_destroy(AdatRes& r) {
    if (r.tiles) (void)hipFree(r.tiles);
    r.tiles = r.tiles_grouped = r.units = r.units_grouped = nullptr;
    r.nunits = r.nunits_grouped = 0;
    r.list_bytes = 0;
    r.group_first.clear(); r.group_ntiles.clear();
}
hipError_t adat_lists_create(AdatRes& r, const AdatPlan& plan, int mp, int count, hipStream_t st) {
    adat_lists_destroy(r);
    r.counters_dirty = true;
    const int nt = mp / TILE;
    const std::vector<int2> order = tile_order(nt);
    std::vector<int2> units, grouped, units_grp;
    if (plan.units) {
        if (count == 1) deal_units(0, plan.ntiles, plan.cpt, plan.upc, units);
        else                                                   // a batch: an LP's units all run on one XCD (xcd-major grid)
            for (int q = 0; q < plan.cpt; q += plan.upc)
                for (int t = 0; t < plan.ntiles; ++t) units.push_back(make_int2(t, q));
    }
    if (plan.grouped) {         // column-group-major unit list: the groups complete one after the other
        grouped = tile_order_grouped(nt, r.group_first, r.group_ntiles);
        for (size_t g = 0; g < r.group_ntiles.size(); ++g) deal_units(r.group_first[g], r.group_ntiles[g], plan.cpt, 1, units_grp);
    }
    r.nunits = (int)units.size(); r.nunits_grouped = (int)units_grp.size();
    r.list_bytes = (order.size() + grouped.size() + units.size() + units_grp.size() + 1) * sizeof(int2);
    hipError_t e = hipMalloc((void**)&r.tiles, r.list_bytes);
    if (e != hipSuccess) { r.tiles = nullptr; r.list_bytes = 0; return e; }
    r.tiles_grouped = r.tiles + order.size();
    r.units = r.tiles_grouped + grouped.size();
    r.units_grouped = r.units + units.size();
    auto put = [&](int2* dst, const std::vector<int2>& v) {
        return v.empty() ? hipSuccess : hipMemcpyAsync(dst, v.data(), v.size() * sizeof(int2), hipMemcpyHostToDevice, st);
    };
    if ((e = put(r.tiles, order)) != hipSuccess || (e = put(r.tiles_grouped, grouped)) != hipSuccess ||
        (e = put(r.units, units)) != hipSuccess || (e = put(r.units_grouped, units_grp)) != hipSuccess) return e;
    return hipStreamSynchronize(st);   // the host lists must outlive the copies
}

// clears the arrival counters (tiles and groups), or the claim word, of every LP of the batch
static hipError_t clear_words(unsigned int* w, size_t bytes, const Batch& bt, hipStream_t st) {
    char* p = (char*)w + (size_t)bt.first * (size_t)bt.stride;
    return bt.count == 1 ? hipMemsetAsync(p, 0, bytes, st) : hipMemset2DAsync(p, (size_t)bt.stride, 0, bytes, (size_t)bt.count, st);
}

static hipError_t launch_units(const AdatPlan& plan, AdatRes& r, const AdatLaunch& a, bool signal_groups, hipStream_t st,
                               bool second_copy, hipEvent_t armed) {
    hipError_t e;
    // a plain launch finds the counters zero unless something else left them dirty: the last arriver of every tile puts its
    // word back; with group words the consumers on other streams make the host clear both kinds, before every launch
    if ((signal_groups || (plan.cpt > 1 && r.counters_dirty)) && (e = clear_words(r.counters, r.counter_bytes, a.batch, st)) != hipSuccess) return e;
    r.counters_dirty = signal_groups;
    if (armed && (e = hipEventRecord(armed, st)) != hipSuccess) return e;
    const int nunits = signal_groups ? r.nunits_grouped : r.nunits;
    if (plan.ntiles <= 0 || nunits <= 0 || a.K <= 0) return hipSuccess;
    UnitsK k{};
    k.A = a.A; k.lda = a.lda; k.s = a.dinv; k.C = a.M; k.ldc = a.ldm; k.C2 = second_copy ? a.M2 : nullptr;
    k.KT = a.K / BK;
    k.cpt = units_chunking(a.K, &k.kc, &k.nbig, &k.ks);
    if (k.cpt == 1) k.kc = 0;
    k.upc = signal_groups ? 1 : plan.upc;
    if (k.cpt != plan.cpt || (k.upc > 1 && k.nbig != k.cpt)) return hipErrorInvalidValue;   // several chunks per unit: uniform chunking only
    k.ntiles = plan.ntiles; k.nunits = nunits;
    k.tile_list = signal_groups ? r.tiles_grouped : r.tiles; k.unit_list = signal_groups ? r.units_grouped : r.units;
    k.diag_pad_from = a.diag_pad_from; k.slabs = r.slabs; k.tile_cnt = r.counters;
    k.grp_cnt = signal_groups ? r.group_words : nullptr; k.grp_w = POTRF_OUTER; k.bk = batch_k(a.batch);
    k.astride = a.shared_a ? 0 : k.bk.stride;
    const int B = a.batch.count;
    const bool xm = B >= 8 && B % 8 == 0;                  // one LP per XCD at a time (see BatchK)
    k.bk.xcd_major = xm ? 1 : 0;
    const dim3 grid = xm ? dim3(8, nunits, B / 8) : dim3(nunits, 1, B);
    if (signal_groups) hipLaunchKernelGGL(gemm_nt_units_kernel<true>, grid, dim3(512), 0, st, k);
    else               hipLaunchKernelGGL(gemm_nt_units_kernel<false>, grid, dim3(512), 0, st, k);
    return hipGetLastError();
}

// The main kernel and, when tiles are split into stream-K chunks, the deterministic fix-up pass.  Canonical chunked summation
// (see the head of this file): data-parallel tiles store their first chunk and add the others; stream-K tiles are summed by
// the fix-up.  The second copy comes from a tile's last flush / the fix-up.
static hipError_t launch_round2(const AdatPlan& plan, AdatRes& r, const AdatLaunch& a, hipStream_t st, bool second_copy) {
    Round2K k;
    k.A = a.A; k.lda = a.lda; k.s = a.dinv; k.C = a.M; k.ldc = a.ldm; k.KT = a.K / BK;
    k.ntiles = plan.ntiles; k.tile_list = r.tiles; k.diag_pad_from = a.diag_pad_from;
    k.ws = r.slabs; k.nwg = plan.nwg; k.sk_claim = r.claim; k.C2 = second_copy ? a.M2 : nullptr;
    k.bk = batch_k(a.batch);
    k.astride = a.shared_a ? 0 : k.bk.stride;
    const int B = a.batch.count;
    if (plan.ntiles <= 0 || k.KT <= 0) return hipSuccess;
    k.kc = canonical_chunk(k.KT);
    if (k.KT <= k.kc) k.kc = 0;              // a contraction of one chunk: one running sum per tile, and whole tiles as stream-K units
    k.sk = k.kc == 0 ? k.KT : round2_unit(k.KT);
    const int cpt = round2_cpt(k.KT);
    const int nrem = plan.ntiles - (plan.ntiles / plan.nwg) * plan.nwg;
    if (nrem > 0) {
        hipError_t em = clear_words(r.claim, sizeof(unsigned int), a.batch, st);
        if (em != hipSuccess) return em;
    }
    // a batch of a multiple of 8 LPs: one LP per XCD at a time (see BatchK)
    const bool xm = B >= 8 && B % 8 == 0;
    k.bk.xcd_major = xm ? 1 : 0;
    const dim3 grid = xm ? dim3(8, plan.nwg, B / 8) : dim3(plan.nwg, 1, B);
    hipLaunchKernelGGL(gemm_nt_streamk_w8_kernel, grid, dim3(512), 0, st, k);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    if (nrem > 0 && cpt > 1) {
        hipLaunchKernelGGL(gemm_nt_fixup_kernel, xm ? dim3(8, nrem * FIX_SPLIT, B / 8) : dim3(nrem * FIX_SPLIT, 1, B), dim3(256), 0,
                           st, k);
        e = hipGetLastError();
    }
    return e;
}

hipError_t launch_adat(const AdatPlan& plan, AdatRes& r, const AdatLaunch& a, bool signal_groups, hipStream_t st,
                       bool* second_copy, hipEvent_t armed) {
    if (!a.A || !a.dinv || !a.M || !r.tiles || !r.claim) return hipErrorInvalidValue;
    if (a.lda >= (1 << 22) || a.ldm >= (1 << 22)) return hipErrorInvalidValue;   // 128-row panels are 32-bit buffers
    if (signal_groups && !(plan.units && plan.grouped)) return hipErrorInvalidValue;
    // a tile's last flush (round-2: or the fix-up) stores the second copy: a contraction of one chunk has no such flush
    const bool second = a.M2 != nullptr && plan.cpt > 1 && !signal_groups;
    if (second_copy) *second_copy = second;
    return plan.units ? launch_units(plan, r, a, signal_groups, st, second, armed) : launch_round2(plan, r, a, st, second);
}

hipError_t launch_wait_count(const unsigned int* cnt, unsigned int target, const int* done, unsigned int* timeout, hipStream_t st) {
    hipLaunchKernelGGL(wait_count_kernel, dim3(1), dim3(64), 0, st, cnt, target, done, timeout);
    return hipGetLastError();
}

}  // namespace lpipm
