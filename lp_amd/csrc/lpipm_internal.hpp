// lpipm_internal.hpp -- shared declarations of liblpipm.so (host C++ + HIP kernels for gfx950).
// Product code: nothing here may include, link or call anything under oracle/.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cstddef>
#include <vector>
#include <utility>
#include "../../include/lpipm.h"

struct lpipm_ctx;

namespace lpipm {

// ---------------------------------------------------------------- geometry
constexpr int TILE = 128;  // output tile edge of the MFMA NT-GEMM == Cholesky block size NB
constexpr int BK   = 16;   // k-tile depth staged through LDS per barrier
constexpr int NB   = 128;  // Cholesky / TRSV block size (== TILE)

inline uint64_t round_up(uint64_t v, uint64_t q) { return (v + q - 1) / q * q; }

// ---------------------------------------------------------------- measurement knobs
// Every LPIPM_* environment variable the library reads is a MEASUREMENT knob (kernel variants, schedules, widths: several
// of them change the bits of a result).  They are read through this one function, which ignores them unless
// LPIPM_EXPERIMENTAL=1 is set as well: a stray variable in a production (or parity-test) environment cannot change what the
// library computes.  tests/conftest.py refuses to run with LPIPM_EXPERIMENTAL set; tests that exercise a knob set both.
const char* lp_knob(const char* name);

// ---------------------------------------------------------------- what another translation unit may know of a context
struct lpipm_ctx_device { int device; hipStream_t stream; };
lpipm_ctx_device lpipm_ctx_device_of(lpipm_ctx* ctx);      // solver.hip

// ---------------------------------------------------------------- error plumbing
void set_error_detail(const char* what, hipError_t e, const char* file, int line);
#define LP_HIP(expr)                                                        \
    do {                                                                    \
        hipError_t e__ = (expr);                                            \
        if (e__ != hipSuccess) {                                            \
            ::lpipm::set_error_detail(#expr, e__, __FILE__, __LINE__);      \
            return LPIPM_ERR_HIP;                                           \
        }                                                                   \
    } while (0)

// ---------------------------------------------------------------- lockstep batches
// `count` LPs of identical geometry live in identical arenas `stride` BYTES apart and advance in
// lockstep: every launch covers all of them through gridDim.z, a kernel of LP z shifts each of its
// pointers by z*stride.  done (nullable) is LP 0's "finished" word: an LP whose word is non-zero is
// skipped by every kernel, so its iterate stays frozen while the others go on.
// count == 1, stride == 0 is the ordinary single-LP launch.
struct Batch {
    int count = 1;
    long long stride = 0;
    const int* done = nullptr;
    int first = 0;        // a launch may cover only the LPs [first, first + count) of the resident batch (pointers stay LP 0's)
};
inline Batch batch_slice(const Batch& b, int first, int count) { return Batch{count, b.stride, b.done, b.first + first}; }
// The part a kernel needs.  xcd_major (A.D.A^T only, count a multiple of 8): grid = (8, workgroups per LP,
// count / 8) and LP = 8*blockIdx.z + blockIdx.x -- workgroups are dealt to the 8 XCDs round-robin along x,
// so all workgroups of one LP share one XCD's L2 and re-use each other's panels of A.
struct BatchK { long long stride; const int* done; int xcd_major; int first; };
inline BatchK batch_k(const Batch& b) { return BatchK{b.stride, b.done, 0, b.first}; }
#ifdef __HIPCC__
__device__ __forceinline__ long long batch_lp(const BatchK& b) {
    return (long long)b.first + (b.xcd_major ? (long long)blockIdx.z * 8 + blockIdx.x : (long long)blockIdx.z);
}
__device__ __forceinline__ bool batch_done(const BatchK& b) {
    return b.done && *(const int*)((const char*)b.done + batch_lp(b) * b.stride) != 0;
}
template <typename T>
__device__ __forceinline__ T* batch_ptr(T* p, const BatchK& b) {   // null stays null
    return p ? (T*)((char*)p + batch_lp(b) * b.stride) : p;
}
template <typename T>
__device__ __forceinline__ const T* batch_ptr(const T* p, const BatchK& b) {
    return p ? (const T*)((const char*)p + batch_lp(b) * b.stride) : p;
}
#endif

// Bump allocator over one arena (per-LP state).  A first pass with base == nullptr only measures.
struct Arena {
    char* base = nullptr;
    size_t off = 0;
    template <typename T>
    T* take(size_t count) {
        off = (off + 255) & ~(size_t)255;
        T* p = (T*)((uintptr_t)base + off);
        off += (count ? count : 1) * sizeof(T);
        return p;
    }
};

// ---------------------------------------------------------------- NT GEMM (kernels_gemm.hip)
// C(tile ti,tj) = beta*C + alpha * sum_k P[ti*TM+r][k] * Q[tj*TN+c][k], one whole output tile per workgroup.
// Row-major operands with K contiguous ("NT"): the launches of the factorisation
//   trailing update    (P = Q = L21, alpha=-1, beta=1, lower tiles)         Cholesky, :129-131
//   TRSM as GEMM       (P = A21, Q = inv(L11), rectangular tiles)
// output tile of a launch (rows x columns); tile indices count in these units
// T32x128 at K = 128 is the panel solve: its Q must be lower triangular with exact zeros above the diagonal (a 128-block inverse).
enum class TileShape { T128x128, T64x64, T32x128, T32x32 };
struct GemmArgs {
    const double* P; int64_t ldp;
    const double* Q; int64_t ldq;
    double*       C; int64_t ldc;
    int           K;            // multiple of BK
    double        alpha, beta;
    int           ntiles;       // == workgroups per LP
    int           tiles_lower;  // 1: tile index -> lower triangle (row-major), 0: rectangular
    int           ntj;          // rectangular: number of tile columns
    int           skip_upper;   // rectangular, C's origin on the diagonal: tiles whose rows all lie above their columns are not run
    TileShape     tile_shape;   // (a value-initialised GemmArgs has 128x128)
    Batch         batch;        // lockstep batch (every pointer above is per LP)
};
hipError_t launch_gemm_nt(const GemmArgs& a, hipStream_t st);

// ---------------------------------------------------------------- A.D.A^T (kernels_adat.hip)
// M = A . diag(dinv) . A^T, lower 128x128 tiles (newton_equations.rs:54-57).  The module owns everything from the geometry
// to the written M: how a launch is cut up and which of its two kernels runs it (the plan), the device words and slabs the
// kernels need (AdatRes: a part of every LP's arena, and the tile / unit lists), and the launch.
// The plan: a function of mp, npa, the batch count, the CU count, the number of ranks of a column split (world; it matters
// for a single LP only) and the value of LPIPM_ADAT_UNITS -- and of nothing else.  Needs no device.
struct AdatPlan {
    int ntiles = 0;
    bool units = false;                  // the (tile, chunk) units kernel with its in-launch combine; else the round-2 kernel
                                         //   (data-parallel tiles + claimed stream-K chunks + fix-up launch)
    int cpt = 1, upc = 1;                // canonical chunks per tile, chunks per unit
    int nwg = 1;                         // round-2 kernel: workgroups per LP
    size_t slabs = 0;                    // chunk slabs (TILE x TILE doubles each) per LP, whichever kernel
    bool grouped = false;                // one LP split by columns over ranks: a second, column-group-major order whose launch
                                         //   signals M's column groups (POTRF_OUTER tile columns each) one by one
};
AdatPlan plan_adat(int mp, int npa, int count, int num_cu, int world, int units_env);
// What the launches of one resident problem use on the device.  A plain copy shares it and owns nothing (a half-batch view).
struct AdatRes {
    // per LP, in the arena (adat_take)
    unsigned int* claim = nullptr;       // round-2 kernel: the word through which the stream-K chunks are claimed
    unsigned int* counters = nullptr;    // units kernel: arrival words of the tiles, then the group words: one clearable block
    size_t counter_bytes = 0;
    unsigned int* group_words = nullptr;
    unsigned int* wait_timeout = nullptr;   // set by a wait kernel that gave up (a producer that never ran)
    double* slabs = nullptr;
    bool counters_dirty = true;          // the counters may be non-zero: the next plain units launch clears them first (a plain
                                         //   launch leaves them zero itself; launches that signal groups do not)
    // shared by the LPs of a batch: ONE allocation (adat_lists_create), tile orders and unit lists
    int2* tiles = nullptr;               // XCD-aware order, then the same tiles column-group-major (plan.grouped)
    int2* tiles_grouped = nullptr;
    int2* units = nullptr;               // (tile, first chunk) in dispatch order, per order
    int2* units_grouped = nullptr;
    int nunits = 0, nunits_grouped = 0;
    size_t list_bytes = 0;
    std::vector<int> group_first, group_ntiles;   // tile sub-list of every column group
    int ngroups() const { return (int)group_ntiles.size(); }
};
// Takes the claim word, the counter block, the time-out word and the slabs of one LP from its arena.
void adat_take(AdatRes& r, const AdatPlan& plan, Arena& arena);
// Builds and uploads the lists (synchronises st); destroy frees them.  Counters start dirty.
hipError_t adat_lists_create(AdatRes& r, const AdatPlan& plan, int mp, int count, hipStream_t st);
void adat_lists_destroy(AdatRes& r);
// Column group g of a grouped plan, for the consumer of a signalling launch: its tiles (device sub-list, and where they
// start in the grouped order) and the word that reaches `ntiles` when all of them are stored.
struct AdatGroup { const int2* tiles; int first, ntiles; const unsigned int* word; };
inline AdatGroup adat_group(const AdatRes& r, int g) {
    return AdatGroup{r.tiles_grouped + r.group_first[(size_t)g], r.group_first[(size_t)g], r.group_ntiles[(size_t)g], r.group_words + g};
}
struct AdatLaunch {
    const double* A; int64_t lda;        // mp x K, row-major
    const double* dinv;                  // per-column scale
    double* M; int64_t ldm;
    double* M2;                          // nullable second copy of M (same ld)
    int K;                               // columns (multiple of BK)
    int diag_pad_from;                   // rows/cols >= this on the diagonal are written as 1.0
    Batch batch;
    bool shared_a = false;               // A is ONE matrix the whole batch shares (member stride 0; lpipm_upload_lockstep_shared)
};
// Picks the kernel and the unit list, clears the counters when they may be non-zero, launches.  signal_groups (grouped plans):
// column-group-major order, one chunk per unit, and the workgroup that completes a group's last tile bumps the group's word;
// `armed` (nullable) is recorded between the clear and the launch: what a consumer on another stream waits for before it
// polls the words.  *second_copy: whether M2 was written by the launch (only a contraction of several chunks can; never
// when groups are signalled) -- if not, the caller copies.
hipError_t launch_adat(const AdatPlan& plan, AdatRes& r, const AdatLaunch& a, bool signal_groups, hipStream_t st,
                       bool* second_copy, hipEvent_t armed = nullptr);
// One wave that returns when *cnt >= target (or when *done != 0, or after a bounded number of polls, which sets *timeout):
// the device-side wait of a stream for a group word of a running launch on another stream.
hipError_t launch_wait_count(const unsigned int* cnt, unsigned int target, const int* done, unsigned int* timeout, hipStream_t st);

// One output tile (128x128, or 64x64 with edge = 64) of a grouped launch: C = alpha * P[0:E, kb:ke) . Q[0:E, kb:ke)^T
// (k-range in units of BK), each tile with its own operands.
struct GemmTileDesc {
    const double* P; const double* Q; double* C;
    int ldp, ldq, ldc;
    int kt_begin, kt_end;
    double alpha;
};
// descs_dev holds LP 0's pointers; LP z of a batch shifts P, Q, C by z*stride.
hipError_t launch_gemm_grouped(const GemmTileDesc* descs_dev, int ntiles, hipStream_t st, const Batch& bt = Batch{},
                               int edge = 128);

// ---------------------------------------------------------------- factor plan (kernels_trsv.hip)
// The factor L is consumed through explicit inverses of its diagonal SUPER-blocks (up to 1024 wide):
// a triangular solve is then a handful of fully parallel mat-vec launches instead of mp/128
// serialized block steps.  The plan owns the inverse storage and the static launch descriptors.
constexpr int SUPER = 1024;  // default super-block width (multiple of NB)
struct SuperBlock {
    int row0, size;          // first row/column of the diagonal super-block, its width (multiple of NB)
    double* inv;             // size x size row-major: inv(L_ss)   (lower triangular, zeros above)
    double* invT;            // size x size row-major: inv(L_ss)^T (upper triangular, zeros below)
};
// A stage's descriptors whose inputs become final with one outer panel of the factorisation: the 128-block inverses the
// merge of blocks [lo, hi) reads and L[mid..hi, lo..mid] are final once chain step hi - 1 has run.
struct MergeGroup { int first, count, stage, panel; };
// The coupled sweep (FactorPlan::coupled): the coupling between NEIGHBOURING super-blocks is multiplied out once per
// factorisation,
//   H_k = Inv_k^T . L[k+1,k]^T  (s_k x s_k+1, k < nsb - 1)        G_k = Inv_k . L[k,k-1]  (s_k x s_k-1, 1 <= k <= nsb - 2),
// and the block columns of L below the near block are kept transposed as well, so that every step of a sweep is ONE launch of
// row-split mat-vec pieces (the last forward step keeps two: G of the last super-block would wait for the last inverse):
//   F_k: y_k = Inv_k.t_k - G_k.y_k-1        ||  t_j -= L[j,k-1].y_k-1 for every j > k
//   B_k: v_k = Inv_k^T.s_k - H_k.v_k+1      ||  s_i -= L[k+1,i]^T.v_k+1 for every i < k
// The pieces behind || read only vectors finished one launch earlier.  t lives in R, y and s in Y, v goes to R.
// Either sweep can be coupled alone (COUPLE_H / COUPLE_G): without G the forward sweep is the plain recurrence as pieces of
// the same kernel (two launches per step), without H the backward sweep is launch_chol_solve's transposed mat-vec and fold.
// One piece: out[i] = (add >= 0 ? add[i] : 0) + a0 * A0[i,:].w0 (+ a1 * A1[i,:].w1), i < rows; the vectors are element offsets
// into R (.. _y == 0) or the scratch Y (== 1) of the solve, each sum in the lane order and butterfly of gemv_n.
struct SweepPiece {
    const double* A0; const double* A1;     // row-major; A1 == nullptr: one term
    int lda0, lda1, np0, np1;
    int rows, blk0;                          // blk0: the piece's first workgroup in its launch (4 rows per workgroup)
    int w0, w1, add, out;
    unsigned char w0_y, w1_y, add_y, out_y;
    unsigned char tri0;                      // A0 is a triangular inverse, zeros elsewhere: 1 lower, 2 upper (0: full rows)
    double a0, a1;
};
constexpr int COUPLE_H = 1, COUPLE_G = 2;   // the backward sweep through H, the forward sweep through G
struct SweepLaunch { int first, count, blocks; };          // pieces [first, first + count), workgroups
// What is enqueued once the inverse of super-block k is and block column k of L is final: the transposed copy of
// L[rows >= lt_row0, column k] (lt: s_k x lt_ld, null: none) and one grouped GEMM for H_k and G_k.
struct CoupleStep { double* lt; int lt_row0, lt_ld; int first, count; };
struct FactorPlan {
    double* L = nullptr;     // the matrix the plan was created for: factored in place by launch_potrf, read by the solves (LP 0's
    int64_t ld = 0;          //   in a batch; null: a plan made only to be measured or inspected, never launched)
    int mp = 0;
    int merge_edge = 128;    // output tile edge of the merge GEMMs (32 / 64: latency-bound, 128: flop-bound)
    int super_w = SUPER;     // width of the diagonal super-blocks whose inverses are formed: wider = fewer, fully
                             // parallel solve steps, but the merge GEMMs cost flops (a batch that already fills
                             // the chip prefers 512)
    std::vector<SuperBlock> sbs;
    GemmTileDesc* descs_dev = nullptr;           // grouped-GEMM tiles of all merge stages (own allocation, shared by a batch)
    unsigned int* pipe_flags = nullptr;          // the pipelined chain step's hand-off words, 8 per 128-block, zero between launches
                                                 //   (kernels_potrf.hip; behind the descriptors in descs_dev's allocation)
    std::vector<std::pair<int, int>> stages;     // (first descriptor, count) per launch, in order
    std::vector<MergeGroup> groups;              // the stages cut by outer panel (stage by stage, panels ascending inside one)
    double* tpart = nullptr;                     // gemv_t slabs of the backward sweep
    double* tws = nullptr;                       // workspace of the merges (T^T of every merge)
    // the coupled sweep (kernels_trsv.hip): storage from the arena, descriptors behind the merges' in descs_dev
    int coupled = 0;                             // COUPLE_H | COUPLE_G: which sweeps are coupled
    int couple_edge = 32;                        // output tile edge of the coupling GEMMs
    std::vector<double*> H, G;                   // per super-block (null where there is none)
    std::vector<CoupleStep> couple;              // per super-block
    std::vector<SweepPiece> pieces;              // host copy of pieces_dev
    SweepPiece* pieces_dev = nullptr;
    std::vector<std::vector<SweepLaunch>> fwd;   // launches of forward step k
    std::vector<SweepLaunch> bwd;                // launches of the backward sweep, in order
    // 128-block k of the factorisation -> where its inverse / transposed inverse go, and their ld
    double* blk_inv(int k) const;
    double* blk_invT(int k) const;
    int blk_ld(int k) const;
};
// Takes the inverse storage for an mp x mp factor living at (L, ld) -- recorded in the plan: every launcher below takes the
// plan alone and works on that matrix -- from the arena (which must be zeroed: the never-written halves of the triangular
// inverses are read as zeros) and, when `build`, uploads the merge descriptors.  build == false: sizing pass, nothing is allocated.
// scratch_of (nullable): a plan of the same mp, widths and arena that is never in use at the same time as this one; the new
// plan then takes only the inverse storage from the arena and works in that plan's merge workspace and gemv_t slabs.
// coupled (COUPLE_H | COUPLE_G): lay out and describe the coupled backward / forward sweep as well (ignored with a single
// super-block).  couple_edge: output tile edge of the coupling GEMMs (32, 64 or 128).
hipError_t factor_plan_create(FactorPlan& plan, double* L, int64_t ld, int mp, Arena& arena, bool build, hipStream_t st,
                              int super_w = SUPER, int merge_edge = 128, const FactorPlan* scratch_of = nullptr,
                              int coupled = 0, int couple_edge = 32);
void factor_plan_destroy(FactorPlan& plan);
// Bytes of the coupling blocks and transposed block columns a coupled plan of this shape takes from its arena.
size_t factor_coupling_bytes(int mp, int super_w, int coupled);
// The coupling work of super-block k (CoupleStep), on `st`.
hipError_t launch_couple_step(const FactorPlan& plan, int k, hipStream_t st);

// ---------------------------------------------------------------- Cholesky (kernels_potrf.hip)
// In-place blocked lower Cholesky of the plan's mp x mp row-major matrix (mp multiple of NB), followed by
// the inverses of its diagonal super-blocks.  info (device int32): 0, or 1 + index of the
// first non-positive pivot.
// Look-ahead for the trailing updates of a single factorisation: `side` is a second stream (CU-masked, so that the chain
// always finds free CUs), ev_chain / ev_rest one event per outer panel.  nullptr: everything on `st`.
struct PotrfLookahead {
    hipStream_t side = nullptr;
    std::vector<hipEvent_t> ev_chain, ev_rest;
    hipEvent_t ev_join = nullptr;   // behind the last thing the side stream was given
    int min_nb = 32;         // 128-blocks from which the look-ahead is used (default: m >= 4096; LPIPM_LOOKAHEAD=1: 12)
};
// With the look-ahead on, the side stream idles for most of every outer panel's chain.  Behind each rest-update it also gets
// the merges of the super-block inverses whose inputs that panel completed (FactorPlan::groups), and what the caller
// attaches here: work that needs nothing but finished panels.  `at` enqueues on `side` and is called once with sb = -1 behind
// the first rest-update, then with sb = k as soon as the inverse of super-block k is enqueued there (k ascending; block
// columns of L up to the end of that super-block are final).  Never called when the look-ahead does not apply;
// `calls` counts the calls made.
struct PotrfBeside {
    hipError_t (*at)(void* self, int sb, hipStream_t side) = nullptr;
    void* self = nullptr;
    int calls = 0;
};
hipError_t launch_potrf(const FactorPlan& plan, int32_t* info, hipStream_t st, const Batch& bt = Batch{},
                        const PotrfLookahead* la = nullptr, bool clear_info = true, PotrfBeside* beside = nullptr);

constexpr int POTRF_OUTER = 4;   // 128-blocks per outer panel (also the width of the column groups of A.D.A^T, kernels_adat.hip)

// ---------------------------------------------------------------- triangular solves (kernels_trsv.hip)
// R[r] <- L^-T L^-1 R[r] for the plan's factor, r < nrhs (1|2); R is nrhs x mp (row stride mp); Yscratch: nrhs x mp.
// steps: the forward steps [fwd_begin, fwd_end) (fwd_end < 0: to the last one; the steps before fwd_begin have been run by
// an earlier call on the same R and Yscratch), then the backward sweep unless `backward` is false.
struct SolveSteps { int fwd_begin = 0, fwd_end = -1; bool backward = true; };
// shared_factor: the factor and the plan's inverses belong to the whole batch (a shared-matrix batch's kept first factor):
// they are not offset by the member, and each step runs as the shared group template of launch_gemv_n / launch_gemv_t.
hipError_t launch_chol_solve(const FactorPlan& plan, int nrhs, double* R, double* Yscratch, hipStream_t st,
                             const Batch& bt = Batch{}, const SolveSteps& steps = SolveSteps{}, bool shared_factor = false);

// ---------------------------------------------------------------- many right-hand sides (kernels_trsm.hip)
// Z = B . L^-T for the factor L of `plan`, order n = plan.mp: row r of Z solves L.z = B[r,:]^T.  B: rows x cols
// (cols <= n, zeros assumed beyond), row-major.  Z: round_up(rows, 16) x n, ld ldz (a multiple of 4), written whole -- rows
// past `rows` as zeros.  One launch, one workgroup per 16 rows, fixed-order sums.
// bt: the members of a lockstep batch, each with its own L, inverses (the plan's are member 0's) and Z, and its own B unless
// shared_b says that B is one block for all of them (it is then not offset).  Finished members' Z stays untouched; member z's
// Z has the bits of a single launch on that member's L.  Without a member dimension (count 1, first 0, no done words) the
// launch is the single kernel's.
hipError_t launch_trsm_lt(const double* B, int64_t ldb, int rows, int cols, const FactorPlan& plan, double* Z, int64_t ldz, hipStream_t st, const Batch& bt = Batch{}, bool shared_b = false);

// ---------------------------------------------------------------- QR arms (kernels_qr.hip)
// EquationSolverType::{Inverse, LeastSquares}: Householder QR of the full mp x mp matrix whose LOWER
// triangle is in M (the upper one is filled in first); reflectors below the diagonal, R on and above,
// tau[mp].  info: 0, or 1 + index of a zero column / zero R diagonal.
hipError_t launch_qr_factor(double* M, int64_t ld, int mp, double* tau, int32_t* info, hipStream_t st);
// R[q] <- R^-1 Q^T R[q] in place, q < nrhs (row stride mp); mp <= 16384
hipError_t launch_qr_solve(const double* M, int64_t ld, int mp, const double* tau, int nrhs, double* R,
                           int32_t* info, hipStream_t st);

// ---------------------------------------------------------------- GEMV (kernels_gemv.hip)
// The three passes over A.  shared_a (as in AdatLaunch): A is ONE matrix that every member of the batch shares
// (lpipm_upload_lockstep_shared) and is not offset by the member (the other operands are); each A element a wave loads
// serves a GROUP of members before the next one is read (gridDim.z = groups), so a pass reads A ceil(count / group) times
// instead of count times.  Every output is summed the same way whatever the group (same lane striding and butterfly, same
// row slabs, same chunk slabs): a member's bits do not depend on whether A is shared.  Finished members are skipped and
// their outputs untouched.
// Y[r][i] = (add[r] ? add[r][i] : 0) + alpha * sum_k A[i][k] * W[r][k],   i < m, k < np
hipError_t launch_gemv_n(const double* A, int64_t lda, int m, int np, int nrhs, const double* W,
                         int64_t ldw, const double* add0, const double* add1, double* Y, int64_t ldy,
                         hipStream_t st, double alpha = 1.0, const Batch& bt = Batch{}, bool shared_a = false);
// Upart[s][r][k] = sum_{i in row split s} A[i][k] * V[r][i];  consumers sum the splits in order.
constexpr int GEMVT_ROWS = 128;
// np: columns processed (multiple of 2); slab: stride between slabs (0 = np)
hipError_t launch_gemv_t(const double* A, int64_t lda, int mp, int np, int nrhs, const double* V,
                         int64_t ldv, double* Upart, hipStream_t st, int64_t slab = 0, const Batch& bt = Batch{},
                         bool shared_a = false);
// One read of A for both products of the residual pair: AxPart[ch][i] = sum over column chunk ch of A[i][k] W[k]
// (gemv_dual_chunks(np) slabs of mp doubles: consumers add them in order) and the row-split slabs of A^T.V as gemv_t.
int gemv_dual_chunks(int np);
hipError_t launch_gemv_dual(const double* A, int64_t lda, int mp, int np, const double* W, const double* V, double* AxPart,
                            double* Upart, int64_t slab, hipStream_t st, const Batch& bt = Batch{}, bool shared_a = false);
// Rho[q] = R0[q] - M.V[q] (q < nrhs) for a symmetric mp x mp M whose LOWER triangle is stored (one read of it);
// slabs: symv_slab_doubles(mp) doubles of scratch.  The residual of the refinement step of the Cholesky solve.
size_t symv_slab_doubles(int mp);
hipError_t launch_symv_residual(const double* M, int64_t ld, int mp, int nrhs, const double* V, int64_t ldv, const double* R0,
                                int64_t ldr, double* Rho, int64_t ldo, double* slabs, hipStream_t st, const Batch& bt = Batch{});
// slack structure [I; 0] of the last ns columns (never stored), see kernels_gemv.hip
hipError_t launch_slack_n(int ns, int nx, int nrhs, const double* W, int64_t ldw, double* Y, int64_t ldy, hipStream_t st,
                          const Batch& bt = Batch{});
hipError_t launch_slack_t(int ns, int nx, int nrhs, int nsplit, const double* V, int64_t ldv, double* Upart, int64_t slab,
                          hipStream_t st, const Batch& bt = Batch{});
// both slack terms of the dual pass in one launch: slack_n into chunk slab 0 of AxPart and slack_t (one vector) into Upart
hipError_t launch_slack_dual(int ns, int nx, int nsplit, const double* W, const double* V, double* AxPart, double* Upart,
                             int64_t slab, hipStream_t st, const Batch& bt = Batch{});
hipError_t launch_slack_diag(int ns, int nx, const double* d, double* M, int64_t ldm, hipStream_t st,
                             const Batch& bt = Batch{});
// U[r][k] = sum_s Upart[s][r][k]   (stand-alone reduce; the solver fuses this into its consumers)
hipError_t launch_gemv_t_reduce(const double* Upart, int nsplit, int nrhs, int np, double* U,
                                int64_t ldu, hipStream_t st);

// ---------------------------------------------------------------- equilibration (kernels_scale.hip)
// Power-of-two row and column scaling of the resident matrix (lpipm_set_scaling): int32 exponents kr[mp], kc[np] per exponent
// set -- one set per member of a batch whose members own their matrices, ONE for a single LP and for a shared-matrix batch
// (estride 0) -- and the slabs of the maxima pass, all in one allocation of the context that exists only while scaling is on.
struct ScaleBuf {
    int32_t* kr = nullptr;       // set 0's row exponents; set z's are estride elements * z further
    int32_t* kc = nullptr;
    long long estride = 0;
    double* rslab = nullptr;     // [set][column chunk][mp] row maxima of a chunk of columns
    double* cslab = nullptr;     // [set][row block][npa] column maxima of a block of rows
    int sets = 0;
};
size_t scale_buf_bytes(int mp, int np, int npa, int sets);
ScaleBuf scale_buf_place(void* base, int mp, int np, int npa, int sets);   // base: scale_buf_bytes, exponents zeroed
// `passes` passes of maxima + exponent update over the stored block(s) A (mp x npa, of which m x nx count; ns structural
// slack columns), then the scaling of A in place.  bt: the matrices, one per exponent set (count == 1 for a shared one).
hipError_t launch_equilibrate(const ScaleBuf& s, double* A, int m, int mp, int nx, int npa, int ns, int passes, hipStream_t st,
                              const Batch& bt);
// b[i] <- ldexp(b[i], kr[i]) (i < m), c[j] <- ldexp(c[j], kc[j]) (j < nc) for every member of bt; b or c may be null.
hipError_t launch_scale_vectors(const ScaleBuf& s, double* b, int m, double* c, int nc, hipStream_t st, const Batch& bt);
// x[j] <- ldexp(x[j], kc[j]) (j < n) for every member of bt: the scaled problem's solution in the caller's units.
hipError_t launch_unscale_x(const ScaleBuf& s, double* x, int n, hipStream_t st, const Batch& bt);

// ---------------------------------------------------------------- probe (kernels_probe.hip)
hipError_t launch_mfma_probe(int iters, double* sink, int blocks, hipStream_t st);

}  // namespace lpipm
