// kernels_pack.hip -- lpipm_upload_device: the caller's strided DEVICE arrays into the zeroed resident image.
//
// Every host upload is a handful of hipMemcpy2DAsync calls out of host memory; a problem that is already in HBM is moved by
// the three kernels here instead, in the layout the solves read (solver.hip, copy_in): A as an mp x npa row-major image of
// doubles per member (or one for a shared-matrix batch), b and c in the members' arenas.  A source element is a double or a
// float (widened, exact); its strides are the caller's, in elements.  Only plain vector loads and stores: no kernel here
// synchronises with anything but its own workgroup.  The images are zeroed beforehand and nothing outside the m x nx block
// (the len entries of a vector) is written, so the padding stays the memset's zero.
// The hosts of these launches have checked every address they form against the caller's allocations.
#include "vec_kernels.hpp"
#include "device_source.hpp"

namespace lpipm {

constexpr int PK_ROWS = 32;      // rows of a tile, every mode
constexpr int PK_WIDE = 128;     // columns of a tile of the row modes: 64 lanes x 2 elements
constexpr int PK_SQ = 32;        // columns of a tile of the LDS-transposed and the gather mode

template <typename T> struct Pair;
template <> struct Pair<double> { using type = double2; };
template <> struct Pair<float> { using type = float2; };

// ---------------------------------------------------------------- A
// grid (column tiles, row tiles of block 0 then of block 1, members), 256 threads.  The mode of a block of rows is chosen on
// the host from its strides and alignment (pack_mode):
//   RowWide  unit column stride, base and pitches multiples of two elements: a wave moves whole row segments, lane l the
//            elements 2l, 2l + 1 of a 128-column tile in one load (16 bytes of double, 8 of float) and one 16-byte store (the
//            image is always 16-byte aligned: npa is a multiple of 16, arenas start on 4096-byte bounds).  Four waves, eight
//            rows each, the eight loads ahead of the stores.
//   Row      the same walk with one element per lane and load (lanes l and l + 64 of the tile): 8-byte stores.
//   Col      unit row stride (a column-major source): through a 32 x 32 LDS tile, rows padded by one double, as
//            k_tall_transpose does, so that both sides move whole 256-byte (float: 128-byte) segments.
//   Gather   any other strides: lane l reads element (i, j0 + l) wherever it is.  Correct, not fast: every load is a
//            transaction of its own.
template <typename T>
__global__ __launch_bounds__(256) void k_pack_matrix(PackMatrix a) {
    using T2 = typename Pair<T>::type;
    __shared__ double tile[PK_SQ][PK_SQ + 1];
    const int t0 = (a.seg[0].rows + PK_ROWS - 1) / PK_ROWS;
    const int s = (int)blockIdx.y >= t0 ? 1 : 0;
    const PackSeg g = a.seg[s];
    const long long i0 = (long long)((int)blockIdx.y - (s ? t0 : 0)) * PK_ROWS;
    const T* src = (const T*)g.src + (long long)blockIdx.z * g.ms;
    double* dst = (double*)((char*)a.dst + (long long)blockIdx.z * a.dstride) + (long long)g.row0 * a.ldd;
    const int tid = threadIdx.x, nx = a.nx;
    if (g.mode == (int)PackMode::RowWide || g.mode == (int)PackMode::Row) {
        const int j0 = blockIdx.x * PK_WIDE;
        if (j0 >= nx) return;
        const int lane = tid & 63, w = tid >> 6;
        constexpr int PER = PK_ROWS / 4;
        if (g.mode == (int)PackMode::RowWide) {
            const int j = j0 + 2 * lane;
            T2 v[PER];
            T last[PER];
#pragma unroll
            for (int k = 0; k < PER; ++k) {
                const long long i = i0 + w + 4 * k;
                v[k] = T2{0, 0}; last[k] = 0;
                if (i < g.rows) {
                    if (j + 1 < nx) v[k] = *(const T2*)(src + i * g.rs + j);
                    else if (j < nx) last[k] = src[i * g.rs + j];
                }
            }
#pragma unroll
            for (int k = 0; k < PER; ++k) {
                const long long i = i0 + w + 4 * k;
                if (i < g.rows) {
                    if (j + 1 < nx) *(double2*)(dst + i * a.ldd + j) = double2{(double)v[k].x, (double)v[k].y};
                    else if (j < nx) dst[i * a.ldd + j] = (double)last[k];
                }
            }
        } else {
            T v[PER][2];
#pragma unroll
            for (int k = 0; k < PER; ++k) {
                const long long i = i0 + w + 4 * k;
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    const int j = j0 + lane + 64 * h;
                    v[k][h] = (i < g.rows && j < nx) ? src[i * g.rs + j] : (T)0;
                }
            }
#pragma unroll
            for (int k = 0; k < PER; ++k) {
                const long long i = i0 + w + 4 * k;
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    const int j = j0 + lane + 64 * h;
                    if (i < g.rows && j < nx) dst[i * a.ldd + j] = (double)v[k][h];
                }
            }
        }
        return;
    }
    const int j0 = blockIdx.x * PK_SQ;
    if (j0 >= nx) return;                       // (the whole workgroup: the grid is as wide as the widest mode needs)
    const int tx = tid & 31, ty = tid >> 5;
    if (g.mode == (int)PackMode::Col) {
        for (int r = ty; r < PK_SQ; r += 8) {   // tile[column][row]: lanes walk the source's contiguous rows
            const long long i = i0 + tx;
            const int j = j0 + r;
            tile[r][tx] = (i < g.rows && j < nx) ? (double)src[i * g.rs + (long long)j * g.cs] : 0.0;
        }
        __syncthreads();
        for (int r = ty; r < PK_ROWS; r += 8) {
            const long long i = i0 + r;
            const int j = j0 + tx;
            if (i < g.rows && j < nx) dst[i * a.ldd + j] = tile[tx][r];
        }
    } else {
        for (int r = ty; r < PK_ROWS; r += 8) {
            const long long i = i0 + r;
            const int j = j0 + tx;
            if (i < g.rows && j < nx) dst[i * a.ldd + j] = (double)src[i * g.rs + (long long)j * g.cs];
        }
    }
}
hipError_t launch_pack_matrix(const PackMatrix& a, bool f32, int members, hipStream_t st) {
    const int t0 = (a.seg[0].rows + PK_ROWS - 1) / PK_ROWS, t1 = (a.seg[1].rows + PK_ROWS - 1) / PK_ROWS;
    if (a.nx <= 0 || t0 + t1 <= 0 || members <= 0) return hipSuccess;
    unsigned gx = 0;
    for (int s = 0; s < 2; ++s) {
        if (a.seg[s].rows <= 0) continue;
        const bool rows = a.seg[s].mode == (int)PackMode::RowWide || a.seg[s].mode == (int)PackMode::Row;
        const int w = rows ? PK_WIDE : PK_SQ;
        const unsigned need = (unsigned)((a.nx + w - 1) / w);
        if (need > gx) gx = need;
    }
    const dim3 grid(gx, (unsigned)(t0 + t1), (unsigned)members);
    if (grid.y > 65535u || grid.z > 65535u) return hipErrorInvalidValue;     // m <= 2^20: 32769 row tiles; at most 4096 members
    if (f32) hipLaunchKernelGGL(k_pack_matrix<float>, grid, dim3(256), 0, st, a);
    else hipLaunchKernelGGL(k_pack_matrix<double>, grid, dim3(256), 0, st, a);
    return hipGetLastError();
}

// ---------------------------------------------------------------- b, c, c0
// grid (element block, segment, member).  Element i of member z's segment comes from src[z * ms + i * stride]; the first
// thread of the first block of segment 0 also moves the member's c0 out of the packed staging array.
template <typename T>
__global__ __launch_bounds__(256) void k_pack_vectors(PackVectors a) {
    const PackVecSeg s = a.seg[blockIdx.y];
    const long long z = blockIdx.z, off = z * a.dstride;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0 && a.c0_dst) *(double*)((char*)a.c0_dst + off) = a.c0_src[z];
    if (!s.dst || i >= s.len) return;
    ((double*)((char*)s.dst + off))[i] = (double)((const T*)s.src)[z * s.ms + (long long)i * s.stride];
}
hipError_t launch_pack_vectors(const PackVectors& a, bool f32, int members, hipStream_t st) {
    int len = 1;                                // (one block per segment at least: c0 rides on segment 0's first)
    for (int s = 0; s < 2; ++s) if (a.seg[s].dst && a.seg[s].len > len) len = a.seg[s].len;
    if (members <= 0 || members > 65535) return members <= 0 ? hipSuccess : hipErrorInvalidValue;
    const dim3 grid((unsigned)((len + 255) / 256), 2, (unsigned)members);
    if (f32) hipLaunchKernelGGL(k_pack_vectors<float>, grid, dim3(256), 0, st, a);
    else hipLaunchKernelGGL(k_pack_vectors<double>, grid, dim3(256), 0, st, a);
    return hipGetLastError();
}

// ---------------------------------------------------------------- the slack hint
// grid (column tiles of the ns hinted columns, row tiles, members), 32 x 8 threads over 32 x 32 elements; the fast index
// follows the source's unit stride (tx_rows: a column-major source).  slack_hint_holds's comparison (batch_plan.hpp): != against
// exact 1.0 / 0.0, so a NaN fails it.  Every mismatching thread stores the same 0: no ordering is needed.
template <typename T>
__global__ __launch_bounds__(256) void k_slack_hint(SlackHint a, int tx_rows) {
    const T* src = (const T*)a.src + (long long)blockIdx.z * a.ms;
    const int tx = threadIdx.x, ty = threadIdx.y;
    bool bad = false;
    for (int r = ty; r < 32; r += 8) {
        const long long i = (long long)blockIdx.y * 32 + (tx_rows ? tx : r);
        const long long j = (long long)blockIdx.x * 32 + (tx_rows ? r : tx);
        if (i < a.m && j < a.ns) {
            const double v = (double)src[i * a.rs + (a.col0 + j) * a.cs];
            bad |= v != (i == j ? 1.0 : 0.0);
        }
    }
    if (bad) *a.word = 0;
}
hipError_t launch_slack_hint(const SlackHint& a, bool f32, int members, hipStream_t st) {
    if (a.m <= 0 || a.ns <= 0 || members <= 0) return hipSuccess;
    const dim3 grid((unsigned)((a.ns + 31) / 32), (unsigned)((a.m + 31) / 32), (unsigned)members);
    if (grid.y > 65535u || grid.z > 65535u) return hipErrorInvalidValue;
    const int tx_rows = a.rs == 1 && a.cs != 1;
    if (f32) hipLaunchKernelGGL(k_slack_hint<float>, grid, dim3(32, 8), 0, st, a, tx_rows);
    else hipLaunchKernelGGL(k_slack_hint<double>, grid, dim3(32, 8), 0, st, a, tx_rows);
    return hipGetLastError();
}

}  // namespace lpipm
