// solver.hip -- the device-resident interior-point loop behind the C ABI (include/lpipm.h).
//
// Host side of InteriorPoint::solve_normal_form (interior_point/mod.rs:199-240): A is uploaded
// once; every iteration is a fixed sequence of kernel launches on the ctx's stream with all
// scalars on device; the host reads back one 96-byte status record per iteration to decide
// termination exactly as mod.rs:230-235 does.  There is no CPU fallback: every numerical step is
// a HIP kernel, and a missing/unusable device is an error.
//
// Algebraic reuse that leaves results identical to the reference (same inputs, same arithmetic):
//   * (p, q) = sym_solve(c, b) is computed once per iteration; the reference recomputes it for the
//     corrector with the same factor and inputs (feasible_point.rs:149 -> newton_equations.rs:187);
//   * r_P, r_D of the next get_delta (feasible_point.rs:122-123) are the vectors whose norms the
//     indicators just took (residual.rs:22-26) at the same point;
//   * the predictor's two sym_solve calls share one pass over A per GEMV and one 2-RHS solve.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <cmath>
#include <vector>
#include <string>
#include <optional>
#include <thread>
#include <atomic>
#include <chrono>
#include "vec_kernels.hpp"
#include "batch_plan.hpp"
#include "device_source.hpp"

using namespace lpipm;

namespace lpipm {
static thread_local std::string g_err_detail;
void set_error_detail(const char* what, hipError_t e, const char* file, int line) {
    char buf[512];
    snprintf(buf, sizeof(buf), "%s -> %s (%s:%d)", what, hipGetErrorString(e), file, line);
    g_err_detail = buf;
}
}  // namespace lpipm

namespace lpipm { extern long long* g_diag_stamps; }
namespace lpipm {
const char* lp_knob(const char* name) {
    const char* master = getenv("LPIPM_EXPERIMENTAL");
    return (master && master[0] == '1') ? getenv(name) : nullptr;
}
}  // namespace lpipm
enum { T_VEC = 0, T_ADAT, T_POTRF, T_TRSV, T_GEMV, T_NTAGS };

namespace {   // the parts of a context: local to this file
// What one stream of solver work owns on the host: a context has one, and so has each of its half-batch views.  Made by
// stream_res_create, released by stream_res_destroy; nobody else creates or frees a member.
struct StreamRes {
    hipStream_t st = nullptr;
    hipEvent_t ev_begin = nullptr, ev_end = nullptr;
    hipEvent_t ev_status = nullptr;    // recorded behind the status copy of an iteration
    std::vector<hipEvent_t> events;    // phase marks (prof_mark), created as they are needed
    std::vector<int> mark_tags;
    size_t nmarks = 0;
    StatusRec* status_host = nullptr;  // pinned, status_cap records
    size_t status_cap = 0;
    unsigned int* timeout_host = nullptr;   // pinned mirror of AdatRes::wait_timeout, read with the status record
    double* x_pinned = nullptr;        // pinned bounce buffer of the solution (a D2H copy into the caller's pageable array takes
    size_t x_pinned_cap = 0;           //   the runtime's staged path: ~40 us more per solve than pinned + memcpy)
    uint32_t seq_counter = 0;          // sequence numbers of the status records (VecArgs::status_seq)
    bool spin_status = false;          // this solve waits for an iteration by watching the records' sequence words (wait_status)
};

// The padded geometry of a resident problem: what the two allocations and their layouts are a function of.  Two uploads
// with equal geometries share them.  nxp, mk: tall only (zero otherwise); nsplit and nblk follow from the others.
struct Geometry {
    int mp = 0, np = 0, npa = 0, nxp = 0, mk = 0, B = 0, nsplit = 0, nblk = 0;
    int mep = 0;                 // tall_eq only: the `eq` rows padded to 128, the order of S (mk is then that of the `ub` rows alone)
    int mpv = 0, npv = 0;        // the paddings of the row and column VECTORS: mp and np, but on the bounded form those of m + nb and n + nb
    int nbp = 0;                 // bounded form only: the bounded columns padded to 256 (what the index lists and ratio vectors are sized by)
    bool box = false;
    int nfp = 0;                 // general bounds only: the free columns padded to 256 (their index list)
    bool gen = false;            // general bounds (lpipm_upload_bounds): the arena holds sigma, t and the free columns' lists and net vector
    bool shared = false, keep = false, tall = false, tall_eq = false;
    int coupled = 0;             // the factor plans lay out the coupled sweep (coupled_for)
    bool operator==(const Geometry&) const = default;
};

// One symmetric system of the iteration, complete: the matrix, the plan that factors it in place and solves with it, its
// pivot-failure word, and the one A.D.A^T launch that builds it (plan, device resources, operand) with what follows it on the
// diagonal.  Laid out by layout_system, its operand bound by bind_systems, built by build_system.  The uploading context owns
// the FactorPlan (lpipm_ctx::plans) and the allocations: a plain copy shares everything and owns nothing.
struct NormalSystem {
    double* M = nullptr;                 // n x n (ld), lower triangle; null: this problem has no such system
    int n = 0; int64_t ld = 0;
    const FactorPlan* factor = nullptr;  // created for (M, ld): the launchers take it alone
    int32_t* info = nullptr;             // where its failed pivot is kept
    AdatPlan ap; AdatRes res;            // of the launch that builds it (kernels_adat.hip)
    bool twin = false;                   // the kept first system: built by the working system's launch (its A, ap and res) into this M
    // the build's operand: M = A.diag(dinv).A^T over K columns, diagonal entries from diag_pad_from on written as 1
    const double* A = nullptr; int64_t lda = 0; const double* dinv = nullptr; int K = 0, diag_pad_from = 0; bool shared_a = false;
    int ns = 0, nx = 0; const double* d = nullptr;     // ... and its diagonal add-on: M[i][i] += d[nx + i], i < ns (d null: none)
};
enum { SYS_WORK = 0, SYS_FIRST, SYS_SCHUR, SYS_COUNT };

// The resident problem: geometry, device pointers and launch arguments.  Every pointer points into an allocation of the
// context that uploaded it (arena, a_shared, the factor plans; the tile and unit lists belong to each system's `res`, made by
// adat_lists_create and freed by adat_lists_destroy), so a plain copy of this struct shares the device state and owns
// nothing: that is what a half-batch view holds (make_view).
struct Problem {
    bool has_problem = false;
    Geometry geo;                // what the fields below and the allocations were laid out for (set_geometry)
    uint64_t m = 0, n = 0;
    int mp = 0, np = 0, nblk = 1, nsplit = 1;
    int ns = 0, nx = 0, npa = 0;   // slack columns (not stored), structural columns, their padded count = lda of A
    // per-LP device state lives in one arena; a lockstep batch of B LPs has B of them, bstride bytes apart
    char* arena = nullptr;
    size_t arena_bytes = 0, bstride = 0;
    int B = 1;
    // lpipm_upload_lockstep_shared: ONE A for the whole batch, outside the arenas (mp x npa, zeros beyond n and m); every
    // pass over A serves all members (the *_shared GEMV launches, A.D.A^T with A's member stride 0)
    bool shared_a = false;
    double* a_shared = nullptr;
    size_t a_shared_bytes = 0;
    Batch bt;                    // what the solve path hands to every launcher (count, stride, done flags)
    Batch bt_head;               // same with the done test always on: the speculatively enqueued head of an iteration
    // SYS_WORK: M = A.D.A^T, or, tall, K (res.ngroups() > 0: one LP split by columns over ranks, M is reduced column group by
    // column group behind the running launch).  SYS_FIRST: the kept first-iteration twin M1 (keep).  SYS_SCHUR: S (tall_eq).
    NormalSystem sys[SYS_COUNT];
    double* tau = nullptr;               // Householder scalars of the QR arms
    double *A = nullptr, *Y = nullptr, *ATpart = nullptr, *xout = nullptr;
    double *M0 = nullptr, *R0 = nullptr, *Rho = nullptr, *symv_ws = nullptr;   // refinement of the Cholesky solve
    // The first iteration's factor (see lpipm_ctx::first_valid): a second M with a second factor plan's inverses and a copy
    // of the pivot-failure word, at the end of every LP's arena (sys[SYS_FIRST]).  keep: this layout has them.
    bool keep = false;
    // A shared-matrix batch keeps ONE such set for all its members, behind A in a_shared (layout_shared), built once
    // from `ones` -- iteration 1's dinv, exact 1.0 over the np columns -- ahead of the first solve (ensure_shared_factor).
    bool shared_factor = false;
    double* ones = nullptr;
    // The tall inequality form (lpipm_upload_ub_tall; kernels_tall.hip): a pure-`ub` LP whose Newton system is reduced to the
    // nxp x nxp matrix K = X^T.W_s.X + E_x.  The working system is then K (ld nxp), built from Xt, and nothing in the arena is
    // m x m.  The row-split slabs of A^T.v are npa wide (tv.npa), not np.
    // A batch of tall LPs over ONE X (lpipm_upload_lockstep_shared_ub_tall: tall && shared_a) keeps X and Xt once, in a_shared;
    // every member's arena then holds its vectors, W_s, E_x, T, G, U_s, its own K with its factor plan's inverses and its slabs.
    // A batch whose members own their matrices (lpipm_upload_lockstep_ub_tall: tall && !shared_a, B arenas) has the single
    // tall LP's arena per member, X_i and Xt_i included.
    bool tall = false;
    double* Xt = nullptr;        // nxp x mk, row-major, zero padded: X^T of the resident (scaled) X
    TallArgs tv{};
    // A tall LP with `me` equality rows (lpipm_upload_ub_eq_tall; tall is set as well): the image is lpipm_upload_ub_eq's, rows
    // of X then rows of A_eq; Xt and K are those of the `ub` rows alone.  Once per iteration, behind K's factorisation,
    // Zt = A_eq.L^-T (mep x nxp, padding rows zero) and S = Zt.Zt^T (mep x mep, diagonal padded with ones from me) with its
    // own factor plan and A.D.A^T plan (`ones_k`: its dinv).  H, tv.Ve: the work vectors of the solve on S; ZtPart: the
    // row-split slabs of Zt^T.v_e.
    // A batch of such LPs over ONE image (lpipm_upload_lockstep_shared_ub_eq_tall: tall_eq && shared_a): [X; A_eq] and Xt are
    // resident once, in a_shared; every member's arena holds, behind its K, its own Zt, S with its plan's inverses, H, Ve, ZtPart,
    // the words and slabs of the launch that builds S, and its own ones_k (launch_adat moves dinv with the member).
    bool tall_eq = false;
    int me = 0;
    double *Zt = nullptr, *H = nullptr, *ZtPart = nullptr, *ones_k = nullptr;
    // The bounded form (lpipm_upload_bounded; kernels_box.hip): nb of the structural columns have an upper bound.  m and n are
    // then those of the explicit LP, ma + nb and na + nb, and so are the lengths and paddings in `va`; the image, the passes
    // over it and the working system stay those of the ma x na slack form (mp, np, npa, nsplit).  solW, solR: what the pass
    // A.W reads and what the solve works in -- va.W and va.R on every other form, bx.Wb and bx.Rs here.
    bool box = false;
    int nb = 0;
    uint64_t ma = 0, na = 0;     // rows and columns of the resident slack form (== m, n unless box)
    BoxArgs bx{};
    double *solW = nullptr, *solR = nullptr;
    bool from_parts = false;     // uploaded as ub / eq blocks (lpipm_upload_ub_eq): b and c are not in the caller's slack form
    bool owned_tall = false;     // lpipm_upload_lockstep_ub_tall: a tall batch (of any count) whose members own X_i, Xt_i and K
    // Equilibration (lpipm_set_scaling): the exponents and the maxima slabs, in an allocation of their own that exists only
    // for a problem uploaded with scaling on.  scale_passes > 0: the resident A, b and c are the scaled ones.
    int scale_passes = 0;
    void* scale_mem = nullptr;
    size_t scale_bytes = 0;
    ScaleBuf sc;
    double* gs = nullptr;        // 8 doubles: sums / minima that must be reduced across ranks (n-split mode)
    VecArgs va{};
};
}  // namespace

struct lpipm_ctx {
    int device = 0;
    int num_cu = 256;
    StreamRes rs;
    Problem p;
    FactorPlan plans[SYS_COUNT]; // of p.sys[i] (NormalSystem::factor): they own descriptor and piece lists, so they stay here
    // Buffers of the stand-alone potrf / solve entries (lpipm_k_potrf and the like): the padded matrix plan.L with its plan,
    // a pristine copy, right-hand sides, scratch, pivot word, Householder scalars.  kbuf_ensure alone makes them, for an order mp.
    struct KernelScratch {
        std::vector<void*> allocs;
        FactorPlan plan;
        double *M0 = nullptr, *R = nullptr, *Y = nullptr, *tau = nullptr;
        int32_t* info = nullptr; int mp = 0;
        bool chol_valid = false;     // plan.L holds a Cholesky factor (lpipm_k_potrf ran last)
    } k;
    // Iteration 1 of every solve starts from x = z = 1 (k_blind_start), so its dinv is exactly 1 and its normal matrix is
    // A.A^T (+ I on the slack rows): that matrix, its factor, the inverses and the pivot-failure word depend on A alone.  The
    // Cholesky arm of a resident problem therefore factors iteration 1 into a second system (Problem::sys[SYS_FIRST])
    // and every later solve on the same upload starts from it instead of running A.D.A^T and the factorisation again.
    bool first_cache = true;     // lpipm_set_first_factor_cache
    int scaling = 0;             // lpipm_set_scaling: equilibration passes of every later upload (0: none)
    bool first_valid = false;    // sys[SYS_FIRST] holds iteration 1 of this upload (every member's); dropped by any upload.  A
                                 //   half-batch view holds the parent's value for the length of one solve
    bool first_done = false;     // the last solve of this context (or view) got through its iteration 1
    // lpipm_get_duals[_device]: the arena holds the final iterate of the last solve, and last_ret every member's return code of
    // it.  Up from a solve that returned Ok until anything changes what the iterate means (invalidate_duals).  A half-batch
    // view writes its members' codes into its parent's record.
    bool duals_valid = false;
    std::vector<int32_t> last_ret;
    lpipm_ctx* parent = nullptr; // of a half-batch view: the context whose batch it covers
    // what building a shared-matrix batch's one factor took, until the solve it preceded reports it (lpipm_phase_times)
    double build_adat_ms = 0.0, build_potrf_ms = 0.0;
    uint64_t build_launches = 0;
    // lpipm_update_lockstep_vectors: the members' new b, c and c0 packed in one pinned block, and its image on the device.
    // Made on first use, grown when a call needs more, freed by lpipm_destroy; nobody else touches them.
    double* stage_host = nullptr;
    double* stage_dev = nullptr;
    size_t stage_cap = 0;        // doubles, each side
    int* hint_dev = nullptr;     // lpipm_upload_device: the word k_slack_hint writes.  Made on first use, freed by lpipm_destroy
    int units_env = 1;                   // LPIPM_ADAT_UNITS=0: the round-2 kernel (data-parallel tiles + fix-up launch) everywhere
    PotrfLookahead la;                   // trailing updates of one factorisation beside the next panel's chain (launch_potrf)
    // a lockstep batch as two half-batches driven by two host threads on two streams (solve_lockstep): views of this
    // context that share its arena (every pointer is LP 0's; a view's launches cover the LPs [bt.first, bt.first + B))
    bool is_view = false;
    int halves_env = 1;                  // LPIPM_HALVES=0: one stream for the whole batch
    bool pred_done = false;              // the last residual launch also ran the next iteration's k_pred_setup
    std::vector<lpipm_ctx*> halves;
    int refine = 0;              // set from the environment by lpipm_create.  0 (default): plain solves; LPIPM_REFINE=2: every
                                 //   solve of every iteration refined; =1: only from mu / mu_0 <= refine_below() on.
                                 //   Built because ~1 % of the C4 members took a poor last step (alpha 0.987 for 0.99995) and
                                 //   one iteration more than the oracle; measured on all 256 members, no mode removes such
                                 //   members -- each variant has its own one or two, always among the members whose last
                                 //   d_tau is ill-determined in fp64 (tests/golden/make_c4_members.py, margin()): the oracle
                                 //   does the same under a permutation of its columns.  Refinement costs 7-20 % and is off.
    // profiling
    int profiling = 0;           // 0 off, 1 every phase, 2 only the A.D.A^T launches (2 events per iteration)
    double tag_ms[T_NTAGS] = {0, 0, 0, 0, 0};
    uint64_t gemv_passes = 0;
    lpipm_phase_times times{};
    // batch mode: extra contexts (own stream + buffers) driven by host threads, see lpipm_solve_batch
    std::vector<lpipm_ctx*> workers;
    int batch_concurrency = 0;   // 0 = auto
    int lockstep_max = -1;       // lpipm_solve_batch: -1 auto, 0 never group same-shape members, > 0 largest group
    // n-split mode (one LP split by columns over ranks; BASELINE config C5): the collective is the caller's
    bool colsplit = false;
    int rank = 0, world = 1;
    lpipm_allreduce_fn coll = nullptr;
    void* coll_user = nullptr;
    bool coll_on_stream = false;  // the callback enqueues the reduction on the ctx's stream itself (no drain before the call)
    hipStream_t st_c = nullptr;  // communication stream: the column groups of M are packed, reduced and unpacked here, behind the
    hipEvent_t ev_c0 = nullptr, ev_c1 = nullptr;   //   group words of the A.D.A^T launch that is still running on the solver's stream
    double* mpack = nullptr;     // contiguous image of the lower block-triangle of M for its all-reduce
    size_t mpack_count = 0;
};

static void destroy_views(lpipm_ctx* c);      // half-batch views of a lockstep batch (solve_lockstep)
// The iterate in the arena no longer belongs to a completed solve of the resident b and c (lpipm_get_duals: LPIPM_ERR_NO_PROBLEM).
static void invalidate_duals(lpipm_ctx* c) { c->duals_valid = false; }
namespace lpipm { lpipm_ctx_device lpipm_ctx_device_of(lpipm_ctx* c) { return lpipm_ctx_device{c->device, c->rs.st}; } }

// Cross-rank reduction of `count` doubles at a device pointer, ordered after everything enqueued on the ctx's stream
// so far.  Default contract: the stream is drained first and the callee returns when the result is in place.
// lpipm_set_collective_on_stream(ctx, 1): nothing is drained -- the callee enqueues the reduction ON the stream it is
// given (ncclAllReduce(..., stream)) and returns at once; stream order does the rest, and the M panels' reduction
// overlaps whatever the host enqueues next.
static int ctx_allreduce(lpipm_ctx* c, double* ptr, uint64_t count, int op, hipStream_t on = nullptr) {
    if (!c->colsplit || c->world <= 1) return LPIPM_OK;
    if (!c->coll) return LPIPM_ERR_BAD_ARGUMENT;
    hipStream_t st = on ? on : c->rs.st;             // (the M groups are reduced on the communication stream, see enqueue_head)
    if (!c->coll_on_stream) LP_HIP(hipStreamSynchronize(st));
    if (c->coll(c->coll_user, ptr, count, op, (void*)st) != 0) {
        g_err_detail = "the all-reduce callback of lpipm_set_collective reported a failure";
        return LPIPM_ERR_HIP;
    }
    return LPIPM_OK;
}
static int xrank_fn(void* self, double* ptr, int count, int op) { return ctx_allreduce((lpipm_ctx*)self, ptr, (uint64_t)count, op); }

// ------------------------------------------------------------------------------------------------
static int free_list(std::vector<void*>& v) {
    for (void* p : v) (void)hipFree(p);
    v.clear();
    return 0;
}
template <typename T>
static int dalloc(std::vector<void*>& list, std::vector<size_t>* sizes, T** out, size_t count, hipStream_t st) {
    void* p = nullptr;
    const size_t bytes = (count ? count : 1) * sizeof(T);
    LP_HIP(hipMalloc(&p, bytes));
    list.push_back(p);
    if (sizes) sizes->push_back(bytes);
    LP_HIP(hipMemsetAsync(p, 0, bytes, st));
    *out = (T*)p;
    return LPIPM_OK;
}
#define LP_TRY(expr) do { int rc__ = (expr); if (rc__ != LPIPM_OK) return rc__; } while (0)

// ---- StreamRes: created for `count` status records, its status array grown, destroyed -- here and nowhere else
static void stream_res_destroy(StreamRes& r) {
    if (r.st) (void)hipStreamSynchronize(r.st);
    for (hipEvent_t e : r.events) (void)hipEventDestroy(e);
    if (r.ev_begin) (void)hipEventDestroy(r.ev_begin);
    if (r.ev_end) (void)hipEventDestroy(r.ev_end);
    if (r.ev_status) (void)hipEventDestroy(r.ev_status);
    if (r.timeout_host) (void)hipHostFree(r.timeout_host);
    if (r.status_host) (void)hipHostFree(r.status_host);
    if (r.x_pinned) (void)hipHostFree(r.x_pinned);
    if (r.st) (void)hipStreamDestroy(r.st);
    r = StreamRes{};
}
// At least `count` zeroed status records (coherent and mapped: the kernels write them directly, bind_status_pinned).
static int stream_res_grow_status(StreamRes& r, size_t count) {
    if (count <= r.status_cap) return LPIPM_OK;
    if (r.status_host) (void)hipHostFree(r.status_host);
    r.status_host = nullptr; r.status_cap = 0;
    LP_HIP(hipHostMalloc((void**)&r.status_host, count * sizeof(StatusRec), hipHostMallocCoherent | hipHostMallocMapped));
    std::memset(r.status_host, 0, count * sizeof(StatusRec));
    r.status_cap = count;
    return LPIPM_OK;
}
static int stream_res_create(StreamRes& r, size_t count) {
    if (hipStreamCreateWithFlags(&r.st, hipStreamNonBlocking) != hipSuccess || stream_res_grow_status(r, count) != LPIPM_OK ||
        hipHostMalloc((void**)&r.timeout_host, sizeof(unsigned int)) != hipSuccess ||
        hipEventCreate(&r.ev_begin) != hipSuccess || hipEventCreate(&r.ev_end) != hipSuccess ||
        hipEventCreateWithFlags(&r.ev_status, hipEventDisableTiming) != hipSuccess) {
        (void)hipGetLastError();
        stream_res_destroy(r);
        g_err_detail = "failed to create stream / pinned status / events";
        return LPIPM_ERR_HIP;
    }
    *r.timeout_host = 0;
    return LPIPM_OK;
}

static void prof_mark(lpipm_ctx* c, int tag, bool adat_bracket = false) {
    if (!c->profiling || (c->profiling == 2 && !adat_bracket)) return;
    if (c->rs.nmarks == c->rs.events.size()) {
        hipEvent_t e;
        if (hipEventCreate(&e) != hipSuccess) return;
        c->rs.events.push_back(e);
        c->rs.mark_tags.push_back(0);
    }
    c->rs.mark_tags[c->rs.nmarks] = tag;
    (void)hipEventRecord(c->rs.events[c->rs.nmarks], c->rs.st);
    ++c->rs.nmarks;
}
// Adds up the intervals between the first `upto` marks (all of them by default); call when those events have
// completed.  Later marks (the speculatively enqueued head of the next iteration) move to the front.
static void prof_collect(lpipm_ctx* c, size_t upto = (size_t)-1) {
    if (!c->profiling) return;
    if (upto > c->rs.nmarks) upto = c->rs.nmarks;
    for (size_t i = 1; i < upto; ++i) {
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, c->rs.events[i - 1], c->rs.events[i]) == hipSuccess)
            c->tag_ms[c->rs.mark_tags[i]] += ms;
    }
    for (size_t i = upto; i < c->rs.nmarks; ++i) {
        std::swap(c->rs.events[i - upto], c->rs.events[i]);
        c->rs.mark_tags[i - upto] = c->rs.mark_tags[i];
    }
    c->rs.nmarks -= upto;
}

// ------------------------------------------------------------------------------------------------
extern "C" void lpipm_default_opts(lpipm_opts* o) {  // interior_point/mod.rs:50-60
    if (!o) return;
    o->tol = 1e-8; o->alpha0 = 0.99995; o->max_iter = 1000; o->ip = 1;
    o->solver_type = LPIPM_SOLVER_CHOLESKY; o->disp = 0;
}

extern "C" const char* lpipm_strerror(int s) {  // error.rs:10-28
    switch (s) {
        case LPIPM_OK: return "Ok";
        case LPIPM_UNCONSTRAINED:
            return "The problem is unconstrained, meaning the solution is the all-zeros vector if `c` is nonnegative, or unbounded otherwise.";
        case LPIPM_NUMERICAL_PROBLEM:
            return "The solver encountered numerical problems it could not recover from. Likely causes are linearly dependent constraints or variables whose scale differs by multiple orders of magnitude.";
        case LPIPM_INVALID_PARAMETER: return "A parameter was set to an invalid value";
        case LPIPM_INCOMPATIBLE_DIMENSIONS: return "The dimensions of your cost- and constraint arrays do not align.";
        case LPIPM_INFEASIBLE: return "The solver finished successfully, it appears that the problem is infeasible.";
        case LPIPM_UNBOUNDED: return "The solver finished successfully, it appears that your problem is unbounded.";
        case LPIPM_ITERATION_LIMIT:
            return "The solver failed to converge within the maximum number of iterations.";
        case LPIPM_ERR_HIP: return "HIP runtime error (see lpipm_last_error_detail)";
        case LPIPM_ERR_NO_PROBLEM: return "no problem uploaded on this context";
        case LPIPM_ERR_UNSUPPORTED: return "not supported by the HIP backend yet";
        case LPIPM_ERR_BAD_ARGUMENT: return "bad argument";
        default: return "unknown status";
    }
}
extern "C" const char* lpipm_last_error_detail(void) { return g_err_detail.c_str(); }

extern "C" int lpipm_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

// linear_program.rs:125-169
extern "C" int lpipm_problem_build(uint64_t n, uint64_t m_ub, const double* A_ub, const double* b_ub,
                                   uint64_t m_eq, const double* A_eq, const double* b_eq, const double* c,
                                   double* A_out, double* b_out, double* c_out, uint64_t* n_slack_out) {
    if (m_ub + m_eq == 0) return LPIPM_UNCONSTRAINED;                       // :134-136
    if (!c || !A_out || !b_out || !c_out || !n_slack_out) return LPIPM_ERR_BAD_ARGUMENT;
    if ((m_ub && (!A_ub || !b_ub)) || (m_eq && (!A_eq || !b_eq))) return LPIPM_ERR_BAD_ARGUMENT;
    const uint64_t m = m_ub + m_eq, ns = n + m_ub;
    for (uint64_t i = 0; i < m; ++i) {                                       // :145-156
        const double* src = i < m_ub ? A_ub + i * n : A_eq + (i - m_ub) * n;
        double* dst = A_out + i * ns;
        for (uint64_t j = 0; j < n; ++j) dst[j] = src[j];
        for (uint64_t j = 0; j < m_ub; ++j) dst[n + j] = (i == j) ? 1.0 : 0.0;
    }
    for (uint64_t i = 0; i < m; ++i) b_out[i] = i < m_ub ? b_ub[i] : b_eq[i - m_ub];  // :157-158
    for (uint64_t j = 0; j < ns; ++j) c_out[j] = j < n ? c[j] : 0.0;                  // :159-160
    *n_slack_out = m_ub;                                                               // :161
    return LPIPM_OK;
}

extern "C" int lpipm_create(int device, lpipm_ctx** out) {
    if (!out) return LPIPM_ERR_BAD_ARGUMENT;
    *out = nullptr;
    int ndev = 0;
    LP_HIP(hipGetDeviceCount(&ndev));
    if (device < 0 || device >= ndev) {
        g_err_detail = "device index out of range (no usable HIP device?)";
        return LPIPM_ERR_HIP;
    }
    LP_HIP(hipSetDevice(device));
    lpipm_ctx* c = new lpipm_ctx();
    c->device = device;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) == hipSuccess) c->num_cu = prop.multiProcessorCount;
    if (stream_res_create(c->rs, 1) != LPIPM_OK) {
        delete c;
        return LPIPM_ERR_HIP;
    }
    // LPIPM_REFINE (see lpipm_ctx::refine) is read ONCE, here: the arena layout depends on it (M0, R0, Rho and the symv slabs
    // exist only for a refining context: 134 MB at C3, 2 GB at m = 16384, per member of a lockstep batch)
    { const char* e = lp_knob("LPIPM_REFINE"); c->refine = !e ? 0 : (e[0] == '2' ? 2 : (e[0] == '1' ? 1 : 0)); }
    // LPIPM_ADAT_UNITS: 0 = the round-2 kernel everywhere, 2 = the units kernel for every single LP whose slabs fit (measurement /
    // test knob); default 1 = units kernel for lockstep batches, for the column-split reduction and for most single LPs, the
    // 4096x8192 headline included -- plan_adat has the rule, its exceptions (few tiles with several chunks) and the figures
    // (first measured per launch, units vs round-2: 512x1024 0.042 / 0.045 ms, 1024x2048 0.102 / 0.097, 2048x4096 0.469 / 0.458,
    // 4096x8192 2.47 / 2.39 standalone and 2.32 / 2.25 inside a solve; C4 lockstep shard 1732 vs 1674 LP/s)
    { const char* e = lp_knob("LPIPM_ADAT_UNITS"); c->units_env = !e ? 1 : (e[0] == '0' ? 0 : (e[0] == '2' ? 2 : 1)); }
    { const char* e = lp_knob("LPIPM_HALVES"); c->halves_env = (e && e[0] == '0') ? 0 : 1; }
    // Side stream for the look-ahead of the factorisation's trailing updates (launch_potrf; used from m = 4096, see there for
    // the measurements; LPIPM_LOOKAHEAD=0 switches it off, =1 lowers the threshold to m = 1536).  CU-masked (bit i = CU i/8 of XCC i%8): the first R CUs of every XCC stay free for the chain
    // stream's kernels -- the diagonal-block kernel needs a CU to itself (150 KB of LDS) and would otherwise wait for a
    // side-stream tile to drain.  LPIPM_LOOKAHEAD_CUS=R sets R (default 8; 0: an unmasked low-priority stream).
    {
        const char* on = lp_knob("LPIPM_LOOKAHEAD");
        int R = 8;
        if (const char* e = lp_knob("LPIPM_LOOKAHEAD_CUS")) { const int v = atoi(e); if (v >= 0 && v <= 16) R = v; }
        if (on && on[0] == '1') c->la.min_nb = 3 * POTRF_OUTER;
        if (!(on && on[0] == '0') && c->num_cu == 256) {
            uint32_t mk[8] = {0, 0, 0, 0, 0, 0, 0, 0};
            for (int i = 0; i < 256; ++i) if ((i / 8) >= R) mk[i / 32] |= 1u << (i % 32);
            int lo = 0, hi = 0;
            (void)hipDeviceGetStreamPriorityRange(&lo, &hi);      // lo = least priority (numerically largest)
            hipError_t e = R > 0 ? hipExtStreamCreateWithCUMask(&c->la.side, 8, mk) : hipStreamCreateWithPriority(&c->la.side, hipStreamNonBlocking, lo);
            constexpr int NEV = 64;              // outer panels of the largest factorisation (m <= 32768)
            for (int i = 0; i < 2 * NEV && e == hipSuccess; ++i) {
                hipEvent_t ev = nullptr;
                e = hipEventCreateWithFlags(&ev, hipEventDisableTiming);
                if (e == hipSuccess) (i < NEV ? c->la.ev_chain : c->la.ev_rest).push_back(ev);
            }
            if (e == hipSuccess) e = hipEventCreateWithFlags(&c->la.ev_join, hipEventDisableTiming);
            if (e != hipSuccess) {
                (void)hipGetLastError();
                if (c->la.ev_join) { (void)hipEventDestroy(c->la.ev_join); c->la.ev_join = nullptr; }
                for (hipEvent_t ev : c->la.ev_chain) (void)hipEventDestroy(ev);
                for (hipEvent_t ev : c->la.ev_rest) (void)hipEventDestroy(ev);
                c->la.ev_chain.clear(); c->la.ev_rest.clear();
                if (c->la.side) (void)hipStreamDestroy(c->la.side);
                c->la.side = nullptr;
            }
        }
    }
    *out = c;
    return LPIPM_OK;
}

extern "C" void lpipm_destroy(lpipm_ctx* c) {
    if (!c) return;
    for (lpipm_ctx* w : c->workers) lpipm_destroy(w);
    c->workers.clear();
    destroy_views(c);
    (void)hipSetDevice(c->device);
    if (c->rs.st) (void)hipStreamSynchronize(c->rs.st);      // before the buffers go
    if (c->p.arena) (void)hipFree(c->p.arena);
    if (c->p.a_shared) (void)hipFree(c->p.a_shared);
    if (c->p.scale_mem) (void)hipFree(c->p.scale_mem);
    if (c->stage_dev) (void)hipFree(c->stage_dev);
    if (c->stage_host) (void)hipHostFree(c->stage_host);
    if (c->hint_dev) (void)hipFree(c->hint_dev);
    for (NormalSystem& s : c->p.sys) adat_lists_destroy(s.res);
    free_list(c->k.allocs);
    if (c->mpack) (void)hipFree(c->mpack);
    if (c->st_c) { (void)hipStreamSynchronize(c->st_c); (void)hipStreamDestroy(c->st_c); }
    if (c->ev_c0) (void)hipEventDestroy(c->ev_c0);
    if (c->ev_c1) (void)hipEventDestroy(c->ev_c1);
    for (FactorPlan& f : c->plans) factor_plan_destroy(f);
    factor_plan_destroy(c->k.plan);
    if (c->la.side) { (void)hipStreamSynchronize(c->la.side); (void)hipStreamDestroy(c->la.side); }
    for (hipEvent_t e : c->la.ev_chain) (void)hipEventDestroy(e);
    for (hipEvent_t e : c->la.ev_rest) (void)hipEventDestroy(e);
    if (c->la.ev_join) (void)hipEventDestroy(c->la.ev_join);
    stream_res_destroy(c->rs);
    delete c;
}

// Output tile edge of the inverse-merge GEMMs: 64 (a stage of one LP is a few dozen latency-bound tiles: factorisation
// 422 -> 358 us at m = 512, 719 -> 547 at 1024, 2556 -> 2398 at 4096; a batch that fills the chip is indifferent).
// LPIPM_MERGE_EDGE=128 restores the 128x128 tiles (measurement knob, scripts/potrf_sizes.py).
// Width of the diagonal super-blocks whose explicit inverses feed the triangular solves: a function of the problem
// size alone, so that an LP goes through exactly the same arithmetic alone and as a member of a lockstep batch (the
// two paths are bit-identical, tests/test_gpu_c4_members.py).  512 up to m = 2048: the last doubling level of the
// inverse (1024) costs a flop-bound batch more than the two solve steps it saves, and a single small LP about as much
// as it gains.  LPIPM_SUPER=<multiple of 128> overrides it (measurement knob).
static int super_for(int mp) {
    if (const char* e = lp_knob("LPIPM_SUPER")) { const int w = atoi(e); if (w >= NB && w % NB == 0 && w <= 4096) return w; }
    return mp <= 2048 ? 512 : SUPER;
}
// Which sweeps of the triangular solves run coupled (kernels_trsv.hip): a function of the shape alone, never of the
// schedule.  One LP that owns its factor -- no batch, no shared matrix, no column split, not the tall form -- from m = 4096
// (two super-blocks at least; factor_plan_create drops it for one): the backward sweep.  The coupled forward sweep is built
// and tested but off: its blocks G_k cost the chain more beside it than the two launches they save in the corrector's solve
// (profiles/solve_coupled.md).  LPIPM_SOLVE_COUPLED=1 turns both on at any m, =2 the backward and =3 the forward sweep
// alone, =0 both off (measurement knob; tests/test_gpu_coupled_sweep.py).
static int coupled_for(int mp, bool single) {
    if (!single) return 0;
    if (const char* e = lp_knob("LPIPM_SOLVE_COUPLED")) {    // 2 / 3: the backward / the forward sweep alone (the A/B of the parts)
        if (e[0] == '1') return COUPLE_H | COUPLE_G;
        if (e[0] == '0') return 0;
        if (e[0] == '2') return COUPLE_H;
        if (e[0] == '3') return COUPLE_G;
    }
    return mp >= 4096 ? COUPLE_H : 0;
}
static int couple_edge_for() {
    // 32x32 tiles, like the merges: the products run beside the chain, which every side-stream workgroup slows, so the
    // shortest launch wins (C3, it/s: parent 264.96, 128-edge 259.5, 64-edge 264.1, 32-edge 265.96; profiles/solve_coupled.md)
    if (const char* e = lp_knob("LPIPM_COUPLE_EDGE")) { const int v = atoi(e); return (v == 128 || v == 64) ? v : 32; }
    return 32;
}
static int merge_edge_for(int) {
    // 32x32 merge tiles: a stage is one round of tiles on the chain (factorisation m = 512: 194 -> 177 us, 1024: 364 -> 346,
    // 4096: 1865 -> 1854; the lockstep C4 batch is indifferent: 1745 LP/s either way)
    if (const char* e = lp_knob("LPIPM_MERGE_EDGE")) { const int v = atoi(e); return (v == 128 || v == 64) ? v : 32; }
    return 32;
}

// Making a problem resident: request -> geometry -> the two allocations and their layouts -> copy-in.
// What the caller asks to be resident: `count` LPs of one shape (count == 1: the ordinary upload); b, c, c0 one entry per LP.
// The matrix comes one per member (A[i], lda), as the batch's one matrix (shared: A[0]), or as two blocks of
// nx = n - n_slack columns (parts: m_ub rows of A_ub, then m - m_ub rows of A_eq; n_slack == m_ub, true by construction, and c
// holds only the nx structural costs).  Parts of a single LP carry its b, split the same way (b is null); parts of a shared
// batch are its one matrix and b[i] = [b_ub_i; b_eq_i] comes per member.  A tall batch whose members own their matrices
// (owned) is in parts too -- no slack column is stored, c holds the structural costs -- with member i's rows in A[i].
struct UploadParts { uint64_t m_ub = 0; const double* A_ub = nullptr; uint64_t lda_ub = 0; const double* b_ub = nullptr;
                     const double* A_eq = nullptr; uint64_t lda_eq = 0; const double* b_eq = nullptr; };
struct Upload {
    uint64_t count = 1, m = 0, n = 0;
    uint64_t n_slack = 0;                // the structural hint of lpipm_upload_slack, for every member alike (verified by upload_impl)
    const double* const* A = nullptr;
    uint64_t lda = 0;
    std::optional<UploadParts> parts;
    const double *const *b = nullptr, *const *c = nullptr;
    const double* c0 = nullptr;          // nullable: all zero
    bool shared = false;                 // one matrix for all `count` LPs
    bool tall = false;                   // parts with `ub` rows only: the tall inequality form, of the LP or of every member over one X
    bool tall_eq = false;                // tall with `eq` rows as well (one LP, or a batch over one image): the Schur complement on K's factor
    uint64_t me = 0;                     //   its `eq` rows (m - parts.m_ub > 0)
    bool owned = false;                  // tall, a batch whose members own their matrices: X_i = A[i] (lda), b[i] per member; parts holds m_ub only
    bool hint_verified = false;          // the caller has checked the hint on these very matrices (batch_impl): it is not repeated
    bool keep_ok = true;                 // false: solved once (lpipm_solve_batch) or never through the kept factor (column split)
    bool colsplit = false;               // lpipm_upload_nsplit: this rank's columns of a column-split LP
    // lpipm_upload_bounded: parts with nb > 0 bounded structural columns.  m and n stay those of the slack form without the
    // bound rows; bidx (nb, ascending), binv (n entries) and ub (the nb finite bounds) are the caller's host arrays.
    bool box = false;
    uint64_t nb = 0;
    const int *bidx = nullptr, *binv = nullptr;
    const double* ub = nullptr;
    bool upper_bad = false;              // an upper[j] that is NaN or -inf: refused behind the shape
    // lpipm_upload_bounds: the bounded request in the primed variables x_j = t_j + sigma_j x'_j (ub = upper - lower, c = sigma c,
    // c0 = c0 + c.t are the caller's host arrays already), with nf free columns fidx (ascending; finv: n entries) that are not in
    // bidx, sigma and tshift (n entries each: +1 and 0 on the slack columns) and cminus (-c'_j of the free columns, nf entries).
    bool gen = false;
    uint64_t nf = 0;
    const int *fidx = nullptr, *finv = nullptr;
    const double *sigma = nullptr, *tshift = nullptr, *cminus = nullptr;
    bool reflects = false, shifts = false;   // some sigma_j is -1; some t_j is not zero
    int bounds_code = LPIPM_OK;          // what the bounds themselves are refused with, behind the shape
    // lpipm_upload_device: A, b and c are in DEVICE memory, laid out as this descriptor says.  The request is otherwise the
    // equivalent host entry's; its pointers above stand for "given" / "null" only (check_upload) and are never read through.
    const lpipm_device_problem* dev = nullptr;
};
// Which requests are legal, and what the others get.  Every argument of a dense request is looked at before its shape; of a
// request in parts the shape comes first (m == 0 is Unconstrained whatever the blocks are, linear_program.rs:134-136), ahead
// of everything but a batch's count and vector arrays, and a batch's members are looked at last.
static int check_upload(const lpipm_ctx* c, const Upload& u) {
    const bool count_ok = u.count >= 1 && u.count <= 4096;
    if (!u.parts) {
        if (!c || !count_ok || !u.A || !u.b || !u.c || u.lda < u.n) return LPIPM_ERR_BAD_ARGUMENT;
        for (uint64_t i = 0; i < u.count; ++i)
            if (!u.c[i] || !u.b[i] || (!u.shared && !u.A[i])) return LPIPM_ERR_BAD_ARGUMENT;
        if (u.shared && !u.A[0]) return LPIPM_ERR_BAD_ARGUMENT;
        if (u.m == 0) return LPIPM_UNCONSTRAINED;  // linear_program.rs:134-136
        if (u.n == 0 || u.n_slack > u.n || u.n_slack > u.m) return LPIPM_ERR_BAD_ARGUMENT;
    } else {
        const UploadParts& q = *u.parts;
        const uint64_t nx = u.n - u.n_slack, m_eq = u.m - q.m_ub;
        const bool batch = u.shared || u.owned;
        if (batch && (!count_ok || !u.b || !u.c || (u.owned && !u.A))) return LPIPM_ERR_BAD_ARGUMENT;
        if (u.m == 0) return LPIPM_UNCONSTRAINED;  // linear_program.rs:134-136
        if ((!batch && !u.c[0]) || nx == 0) return LPIPM_ERR_BAD_ARGUMENT;
        if (u.owned) { if (u.lda < nx) return LPIPM_ERR_BAD_ARGUMENT; }
        else if (q.m_ub && (!q.A_ub || q.lda_ub < nx || (!u.shared && !q.b_ub))) return LPIPM_ERR_BAD_ARGUMENT;
        if (m_eq && (!q.A_eq || q.lda_eq < nx || (!u.shared && !q.b_eq))) return LPIPM_ERR_BAD_ARGUMENT;
        if (!c) return LPIPM_ERR_BAD_ARGUMENT;
        if (u.tall_eq && q.m_ub == 0) return LPIPM_ERR_UNSUPPORTED;     // no `ub` row: not a tall LP (lpipm_upload_ub_eq is its entry)
        if (u.tall && (c->world > 1 || c->refine > 0)) return LPIPM_ERR_UNSUPPORTED;   // a column-split context; the refined solves
        if (u.upper_bad) return LPIPM_ERR_BAD_ARGUMENT;
        if (u.bounds_code != LPIPM_OK) return u.bounds_code;
        if (u.box && (c->world > 1 || c->refine > 0)) return LPIPM_ERR_UNSUPPORTED;    // likewise
        for (uint64_t i = 0; i < u.count; ++i)
            if (!u.c[i] || (u.b && !u.b[i]) || (u.owned && !u.A[i])) return LPIPM_ERR_BAD_ARGUMENT;
    }
    return u.m > (1u << 20) || u.n > (1u << 24) ? LPIPM_ERR_BAD_ARGUMENT : LPIPM_OK;
}
// The geometry of a request whose hint `n_slack` holds, on a context with these settings: a value, no device needed.
static Geometry geometry_of(const Upload& u, uint64_t n_slack, bool first_cache, int refine) {
    Geometry g;
    g.mp = (int)round_up(u.m, NB); g.np = (int)round_up(u.n, BK); g.npa = (int)round_up(u.n - n_slack, BK);
    if (u.tall) { g.nxp = (int)round_up(g.npa, NB); g.mk = (int)round_up(u.m, BK); }   // the order of K, the contraction of its build
    if (u.tall_eq) { g.tall_eq = true; g.mk = (int)round_up(u.parts->m_ub, BK); g.mep = (int)round_up(u.me, NB); }
    g.B = (int)u.count; g.nsplit = g.mp / GEMVT_ROWS;
    g.mpv = g.mp; g.npv = g.np;
    if (u.box) {     // the system's order, R, Y and the slab count follow m; the row and column vectors follow m + nb and n + nb
        g.box = true; g.mpv = (int)round_up(u.m + u.nb, NB); g.npv = (int)round_up(u.n + u.nb + u.nf, BK); g.nbp = (int)round_up(u.nb, BK);
        g.gen = u.gen; g.nfp = (int)round_up(u.nf, BK);      // (general bounds: the x^- columns lengthen the column vectors only)
    }
    g.nblk = ((g.mpv > g.npv ? g.mpv : g.npv) + 255) / 256;  // (of the larger of m and n: 256 is a multiple of both paddings)
    if (g.nblk > RED_STRIDE) g.nblk = RED_STRIDE;
    g.shared = u.shared; g.tall = u.tall;
    g.keep = u.keep_ok && first_cache && refine <= 0 && !u.tall && !u.box;   // (tall, bounded: the first factor is not kept)
    g.coupled = coupled_for(g.mp, u.count == 1 && !u.shared && !u.tall && !u.colsplit);
    return g;
}
// The geometry into the structs the layouts and the launches read.
static void set_geometry(Problem& p, const Geometry& g) {
    p.geo = g;
    p.mp = g.mp; p.np = g.np; p.npa = g.npa; p.B = g.B; p.nsplit = g.nsplit; p.nblk = g.nblk; p.shared_a = g.shared; p.tall = g.tall;
    p.tv = TallArgs{};
    if (g.tall) { p.tv.npa = g.npa; p.tv.nxp = g.nxp; p.tv.mk = g.mk; }     // (tv.nx: the padded geometry may be shared by several nx)
    p.tall_eq = g.tall_eq; p.tv.mep = g.mep;                                 // (tv.ms, tv.me: likewise)
    p.box = g.box; p.bx = BoxArgs{};
    if (g.box) { p.bx.nps = g.np; p.bx.mps = g.mp; }                         // (bx.nb, na, ma: likewise)
    VecArgs& v = p.va;
    v.np = g.npv; v.mp = g.mpv; v.nblk = g.nblk; v.nsplit = g.nsplit; v.bcount = g.B; v.bfirst = 0; v.refine_below = refine_below();
}
// The plan of the launch that builds a system of `order` rows by a contraction over `contraction` columns, for each of B
// members.  The dense M = A.D.A^T: the batch's plan.  single_bits -- a tall system, K from Xt (nxp rows over the mk padded rows
// of X) or S from Zt (mep rows over nxp): every member's matrix must have the bits the single LP's has.  The units kernel gives
// them whatever the count; the round-2 kernel (which a single LP of a few tiles with several chunks takes) only with the single
// LP's own workgroup count once the contraction is longer than 4096 (round2_unit): the batch then runs that very plan.
static AdatPlan adat_plan_of(int order, int contraction, int B, bool single_bits, int num_cu, int world, int units_env) {
    if (!single_bits) return plan_adat(order, contraction, B, num_cu, world, units_env);
    const AdatPlan single = plan_adat(order, contraction, 1, num_cu, 1, units_env);
    return single.units ? plan_adat(order, contraction, B, num_cu, 1, units_env) : single;     // (B == 1: `single` either way)
}

// Device state is laid out by functions that take p's geometry and an Arena: one pass over a measuring arena sizes an
// allocation, a second pass over the real one places it.  Out: p's device pointers and the factor plans they refer to.
static void bind_status_pinned(lpipm_ctx* c, bool allow);
// The vectors and status words of one LP, dense or tall.
static void layout_vectors(Problem& p, Arena& ar) {
    VecArgs& v = p.va;
    const size_t mp = (size_t)v.mp, np = (size_t)v.np;       // the vectors' paddings (bounded form: of m + nb, n + nb) ...
    const size_t mps = (size_t)p.mp, nps = (size_t)p.np;     // ... and those of the system and the passes over the image
    v.b = ar.take<double>(mp); v.c = ar.take<double>(np);
    v.x = ar.take<double>(np); v.y = ar.take<double>(mp); v.z = ar.take<double>(np);
    v.dinv = ar.take<double>(np); v.xs = ar.take<double>(np); v.r1 = ar.take<double>(np); v.rD = ar.take<double>(np);
    v.p = ar.take<double>(np); v.u = ar.take<double>(np); v.dx = ar.take<double>(np); v.dz = ar.take<double>(np);
    v.dxdz = ar.take<double>(np);
    v.rP = ar.take<double>(mp); v.rP2 = ar.take<double>(mp); v.q = ar.take<double>(mp); v.dy = ar.take<double>(mp);
    // chunk slabs of A.x: sized by the count the launches use (the STORED columns npa -- gemv_dual_chunks is not monotone:
    // 256-column chunks below 4096 columns, 1024-column chunks from there on, so np's count can be the smaller one)
    // (tall: those of the npa stored columns)
    const int ch_a = gemv_dual_chunks(p.npa), ch_n = gemv_dual_chunks((int)nps);
    v.Ax = ar.take<double>(mps * (size_t)(p.tall || ch_a > ch_n ? ch_a : ch_n));
    v.W = ar.take<double>(2 * np); v.R = ar.take<double>(2 * mp);
    p.Y = ar.take<double>(2 * (p.tall ? (size_t)p.tv.nxp : mps));
    p.ATpart = ar.take<double>((size_t)p.nsplit * 2 * (p.tall ? (size_t)p.npa : nps));   // (tall: the slabs of A^T.v are npa wide)
    v.ATpart = p.ATpart;
    p.solW = v.W; p.solR = v.R;
    if (p.box) {     // the index lists, the three kept ratio vectors, W and the solve's right-hand sides
        BoxArgs& bx = p.bx;
        const size_t nbp = (size_t)p.geo.nbp;
        bx.bidx = ar.take<int>(nbp); bx.binv = ar.take<int>(nps);
        bx.Dt = ar.take<double>(nps); bx.Rx = ar.take<double>(nbp); bx.Rw = ar.take<double>(nbp);
        bx.Wb = ar.take<double>(2 * nps); bx.Rs = ar.take<double>(2 * mps);
        p.solW = bx.Wb; p.solR = bx.Rs;
        if (p.geo.gen) {     // general bounds: sigma and t, and with free columns their lists and the net vector -- O(n + nf)
            bx.Sg = ar.take<double>(nps); bx.Tj = ar.take<double>(nps);
            if (p.geo.nfp > 0) { bx.fidx = ar.take<int>((size_t)p.geo.nfp); bx.finv = ar.take<int>(nps); bx.Xn = ar.take<double>(nps); }
        }
    }
    v.S = ar.take<double>(64); v.red = ar.take<double>((size_t)RED_SLOTS * RED_STRIDE);
    v.status = ar.take<StatusRec>(1); v.potrf_info = ar.take<int32_t>(1);
    v.flags = ar.take<int>(1); v.done = ar.take<int>(1); v.skip_refine = ar.take<int>(1);
}
// The kept first factor, on 4096-byte bounds: mp x mp doubles of M, two s x s inverses per diagonal super-block of width s,
// and one page for the pivot-failure word -- first_factor_bytes(mp) in all, a function of mp alone.  Its plan works in the
// first plan's merge workspace and gemv_t slabs: the two are never in use at the same time.  The last block of an LP's arena,
// or, once for a shared-matrix batch, of the shared allocation (the plan's inverses are then the batch's; workspace and
// slabs stay the first plan's, per member).
static size_t first_factor_bytes(int mp, int super_w, int coupled) {
    size_t bytes = (size_t)mp * mp * sizeof(double) + 4096;
    bytes += factor_coupling_bytes(mp, super_w, coupled);   // its own coupling blocks
    for (int r0 = 0; r0 < mp; r0 += super_w) { const size_t s = (size_t)(mp - r0 < super_w ? mp - r0 : super_w); bytes += 2 * s * s * sizeof(double); }
    return bytes;
}
// The plans of the launches that build the systems of p's geometry on context c (what layout_problem sizes their slabs by).
static void plan_builds(Problem& p, const lpipm_ctx* c) {
    const Geometry& g = p.geo;
    p.sys[SYS_WORK].ap = g.tall ? adat_plan_of(g.nxp, g.mk, g.B, true, c->num_cu, 1, c->units_env)
                                : adat_plan_of(g.mp, g.npa, g.B, false, c->num_cu, c->world, c->units_env);
    p.sys[SYS_SCHUR].ap = g.tall_eq ? adat_plan_of(g.mep, g.nxp, g.B, true, c->num_cu, 1, c->units_env) : AdatPlan{};
}
// One system of order n into an arena: its matrix, then the storage of its factor plan, which is created for that matrix.
// merge_for: the member count the merge tiles are chosen for; scratch_of: see factor_plan_create.
static int layout_system(NormalSystem& s, FactorPlan& plan, int n, Arena& ar, bool build, hipStream_t st, int merge_for, int coupled, const FactorPlan* scratch_of = nullptr) {
    s.n = n; s.ld = n; s.M = ar.take<double>((size_t)n * n);
    LP_HIP(factor_plan_create(plan, s.M, n, n, ar, build, st, super_for(n), merge_edge_for(merge_for), scratch_of, coupled, couple_edge_for()));
    s.factor = &plan;
    return LPIPM_OK;
}
static int layout_first_factor(Problem& p, FactorPlan* plans, Arena& ar, bool build, hipStream_t st) {
    NormalSystem& s = p.sys[SYS_FIRST];
    ar.off = (size_t)round_up(ar.off, 4096);
    const size_t begin = ar.off;
    LP_TRY(layout_system(s, plans[SYS_FIRST], p.mp, ar, build, st, p.B, p.geo.coupled, &plans[SYS_WORK]));
    s.info = ar.take<int32_t>(1); s.twin = true;
    ar.off = (size_t)round_up(ar.off, 4096);
    return ar.off - begin == first_factor_bytes(p.mp, super_for(p.mp), p.geo.coupled) ? LPIPM_OK : LPIPM_ERR_BAD_ARGUMENT;   // (the documented size)
}
// The arena of one LP; every LP of a lockstep batch gets the same layout, `bstride` bytes after the previous LP's.
// refine: whether the context refines its solves.  Tall (Problem::tall): the vectors of the dense layout, X and its transpose, the nxp x nxp matrix K with its factor plan, and
// the work vectors of the reduced solve.  Nothing grows as m^2: no M, M0 or kept first factor.
// A member of a shared batch (p.shared_a) has the same arena without A (tall: X and Xt): layout_shared.  A member of a tall
// batch that owns its matrix has the single tall LP's arena.
// tall_eq: behind K and its plan, Zt, S with its plan, the work vectors of the Schur solve, the slabs of Zt^T.v_e, the
// vector of ones and the words and slabs of the launch that builds S -- in every member's arena of a batch as well.
// The systems' A.D.A^T plans are set (relayout); plans: lpipm_ctx::plans.
static int layout_problem(Problem& p, FactorPlan* plans, int refine, Arena& ar, bool build, hipStream_t st) {
    TallArgs& t = p.tv;
    NormalSystem &work = p.sys[SYS_WORK], &schur = p.sys[SYS_SCHUR];
    const size_t mp = (size_t)p.mp, np = (size_t)p.va.np, nxp = (size_t)t.nxp;       // (np: of xout, a column vector)
    p.A = p.shared_a ? nullptr : ar.take<double>(mp * p.npa);
    p.Xt = p.shared_a || !p.tall ? nullptr : ar.take<double>(nxp * (size_t)t.mk);
    layout_vectors(p, ar);
    p.Zt = p.H = p.ZtPart = p.ones_k = nullptr; t.Ve = nullptr;
    if (p.tall) {
        t.Ws = ar.take<double>((size_t)t.mk); t.Ex = ar.take<double>(nxp);
        t.T = ar.take<double>(2 * mp); t.G = ar.take<double>(2 * nxp); t.Us = ar.take<double>(2 * mp);
        LP_TRY(layout_system(work, plans[SYS_WORK], t.nxp, ar, build, st, 1, 0));
        if (p.tall_eq) {
            const size_t mep = (size_t)t.mep;
            p.Zt = ar.take<double>(mep * nxp);
            LP_TRY(layout_system(schur, plans[SYS_SCHUR], t.mep, ar, build, st, 1, 0));
            t.Ve = ar.take<double>(2 * mep); p.H = ar.take<double>(2 * mep);
            p.ZtPart = ar.take<double>(mep / GEMVT_ROWS * 2 * nxp); p.ones_k = ar.take<double>(nxp);
            adat_take(schur.res, schur.ap, ar);
        }
    } else LP_TRY(layout_system(work, plans[SYS_WORK], p.mp, ar, build, st, p.B, p.geo.coupled));
    work.info = schur.info = p.va.potrf_info;    // (a failed pivot of S lands in the word K's does)
    p.M0 = p.R0 = p.Rho = p.symv_ws = nullptr;
    if (refine > 0 && !p.tall) {     // only the refined solves read the matrix itself
        p.M0 = ar.take<double>(mp * mp); p.R0 = ar.take<double>(2 * mp); p.Rho = ar.take<double>(2 * mp);
        p.symv_ws = ar.take<double>(symv_slab_doubles(p.mp));
    }
    p.tau = ar.take<double>(p.tall ? 1 : mp); p.gs = ar.take<double>(8); p.xout = ar.take<double>(np);
    adat_take(work.res, work.ap, ar);
    p.keep = p.geo.keep;
    p.shared_factor = p.keep && p.shared_a;      // one set for the batch, outside the arenas (layout_shared)
    p.ones = nullptr;
    if (p.keep && !p.shared_factor) LP_TRY(layout_first_factor(p, plans, ar, build, st));
    return LPIPM_OK;
}
// The shared allocation of a shared-matrix batch: the one A, mp x npa like an arena's, zero padding (tall: behind X its transpose,
// nxp x mk), then the one kept first factor (p.shared_factor) and the vector of ones, np doubles rounded up to 4096 bytes.
static int layout_shared(Problem& p, FactorPlan* plans, Arena& sh, bool build, hipStream_t st) {
    p.A = sh.take<double>((size_t)p.mp * p.npa);
    if (p.tall) p.Xt = sh.take<double>((size_t)p.tv.nxp * p.tv.mk);
    if (!p.shared_factor) return LPIPM_OK;
    LP_TRY(layout_first_factor(p, plans, sh, build, st));
    p.ones = sh.take<double>((size_t)p.np);
    sh.off = (size_t)round_up(sh.off, 4096);
    return LPIPM_OK;
}
// Both allocations of the context, made anew for geometry g.
static int relayout(lpipm_ctx* c, const Geometry& g) {
    Problem& p = c->p;
    hipStream_t st = c->rs.st;
    LP_HIP(hipStreamSynchronize(st));
    if (p.arena) { LP_HIP(hipFree(p.arena)); p.arena = nullptr; }
    if (p.a_shared) { LP_HIP(hipFree(p.a_shared)); p.a_shared = nullptr; p.a_shared_bytes = 0; }
    for (int i = 0; i < SYS_COUNT; ++i) { adat_lists_destroy(p.sys[i].res); factor_plan_destroy(c->plans[i]); p.sys[i] = NormalSystem{}; }
    p.has_problem = false;
    set_geometry(p, g);
    plan_builds(p, c);
    Arena measure;
    LP_TRY(layout_problem(p, c->plans, c->refine, measure, false, st));
    p.bstride = round_up(measure.off, 4096);
    p.arena_bytes = p.bstride * (size_t)g.B; p.va.bstride = (long long)p.bstride;
    LP_HIP(hipMalloc((void**)&p.arena, p.arena_bytes));
    LP_HIP(hipMemsetAsync(p.arena, 0, p.arena_bytes, st));
    Arena real{p.arena};
    LP_TRY(layout_problem(p, c->plans, c->refine, real, true, st));
    if (g.shared) {
        Arena sh_measure;
        LP_TRY(layout_shared(p, c->plans, sh_measure, false, st));
        p.a_shared_bytes = sh_measure.off;
        LP_HIP(hipMalloc((void**)&p.a_shared, p.a_shared_bytes));
        LP_HIP(hipMemsetAsync(p.a_shared, 0, p.a_shared_bytes, st));
        Arena sh{(char*)p.a_shared};
        LP_TRY(layout_shared(p, c->plans, sh, true, st));
    }
    for (NormalSystem& s : p.sys) if (s.M && !s.twin) LP_HIP(adat_lists_create(s.res, s.ap, s.n, g.B, st));    // (drains st)
    LP_TRY(stream_res_grow_status(c->rs, (size_t)g.B));
    return LPIPM_OK;
}
// What each system's launch reads, bound once the upload's own sizes are known (a padded geometry serves several m, nx, me);
// the kept first system is the working one's twin.
static void bind_systems(Problem& p) {
    const TallArgs& t = p.tv;
    auto bind = [](NormalSystem& s, const double* A, int lda, const double* dinv, int pad_from, bool shared_a, int ns, int nx, const double* d) {
        s.A = A; s.lda = s.K = lda; s.dinv = dinv; s.diag_pad_from = pad_from; s.shared_a = shared_a; s.ns = ns; s.nx = nx; s.d = d;
    };
    // M = A.D.A^T + diag(D_slack) (newton_equations.rs:54-57).  Tall: K = X^T.diag(W_s).X + diag(E_x), Xt as its A, a contraction
    // over the mk padded rows of X (a batch: the one Xt or every member's own, and every member's own W_s), ones beyond nx
    if (p.tall) bind(p.sys[SYS_WORK], p.Xt, t.mk, t.Ws, t.nx, p.shared_a, t.nx, 0, t.Ex);
    // Bounded: M~ = A.diag(D~).A^T + diag(D~_slack): the dense build with D~ for dinv
    else if (p.box) bind(p.sys[SYS_WORK], p.A, p.npa, p.bx.Dt, (int)p.ma, false, p.ns, p.nx, p.bx.Dt);
    else bind(p.sys[SYS_WORK], p.A, p.npa, p.va.dinv, (int)p.ma, p.shared_a, p.ns, p.nx, p.va.dinv);
    // S = Zt.Zt^T: A = Zt, dinv = ones (every member's own of both), the diagonal padded with ones from me, nothing added
    if (p.tall_eq) bind(p.sys[SYS_SCHUR], p.Zt, t.nxp, p.ones_k, t.me, false, 0, 0, nullptr);
}
// The exponent block of the upload being made: `sets` exponent sets for the padded geometry when the context scales, none
// otherwise (what a previous upload left is freed).  Exponents start at zero.
static int scale_setup(lpipm_ctx* c, int mp, int np, int npa, int sets) {
    Problem& p = c->p;
    const size_t need = c->scaling > 0 ? scale_buf_bytes(mp, np, npa, sets) : 0;
    if (need != p.scale_bytes) {
        LP_HIP(hipStreamSynchronize(c->rs.st));
        if (p.scale_mem) { LP_HIP(hipFree(p.scale_mem)); p.scale_mem = nullptr; }
        p.scale_bytes = 0;
        if (need) LP_HIP(hipMalloc(&p.scale_mem, need));
        p.scale_bytes = need;
    }
    p.scale_passes = c->scaling;
    p.sc = ScaleBuf{};
    if (!need) return LPIPM_OK;
    LP_HIP(hipMemsetAsync(p.scale_mem, 0, need, c->rs.st));
    p.sc = scale_buf_place(p.scale_mem, mp, np, npa, sets);
    return LPIPM_OK;
}
// The caller's arrays onto the stream, into the zeroed allocations.  c0v: c0 per member, made by the caller of this function
// as its own arrays are: everything read here must outlive the asynchronous copies.
static int copy_in(lpipm_ctx* c, const Upload& u, const double* c0v) {
    Problem& p = c->p;
    hipStream_t st = c->rs.st;
    const uint64_t nx = (uint64_t)p.nx;
    const size_t D = sizeof(double);
    auto rows = [&](double* dst, const double* src, uint64_t ld, uint64_t nrows) {     // nx columns of each, into A's npa
        return hipMemcpy2DAsync(dst, (size_t)p.npa * D, src, (size_t)ld * D, (size_t)nx * D, (size_t)nrows, hipMemcpyHostToDevice, st);
    };
    auto vec = [&](const void* dst, const double* src, uint64_t count) { return hipMemcpyAsync((void*)dst, src, count * D, hipMemcpyHostToDevice, st); };
    // A: as parts -- rows of A_ub, then rows of A_eq, into the single LP's arena or the batch's one matrix -- or shared, here;
    //    per member (dense, or the owned tall batch's X_i), with the member's vectors below.
    // b: per member below, or in parts of a single LP, each part behind its rows.
    if (u.parts && !u.owned) {
        const UploadParts& q = *u.parts;
        const uint64_t m_ub = q.m_ub, m_eq = u.m - m_ub;
        if (m_ub) {
            LP_HIP(rows(p.A, q.A_ub, q.lda_ub, m_ub));
            if (!u.shared) LP_HIP(vec(p.va.b, q.b_ub, m_ub));
        }
        if (m_eq) {
            LP_HIP(rows(p.A + (size_t)m_ub * p.npa, q.A_eq, q.lda_eq, m_eq));
            if (!u.shared) LP_HIP(vec(p.va.b + m_ub, q.b_eq, m_eq));
        }
    } else if (u.shared) LP_HIP(rows(p.A, u.A[0], u.lda, u.m));
    // c: n entries, or, in parts, the nx structural costs: c = [c; 0], and the arena is zero
    const uint64_t nc = u.parts ? nx : u.n;
    for (uint64_t i = 0; i < u.count; ++i) {
        const size_t off = (size_t)i * p.bstride;
        if (!u.shared && (!u.parts || u.owned)) LP_HIP(rows((double*)((char*)p.A + off), u.A[i], u.lda, u.m));
        if (u.b) LP_HIP(vec((const char*)p.va.b + off, u.b[i], u.m));
        LP_HIP(vec((const char*)p.va.c + off, u.c[i], nc));
        LP_HIP(vec((const char*)(p.va.S + S_C0) + off, &c0v[i], 1));
    }
    if (u.box) {     // b_ext = [b; u_B]; c_ext = [c; 0]: the arena is zero; the index lists
        LP_HIP(vec(p.va.b + u.m, u.ub, u.nb));
        LP_HIP(hipMemcpyAsync((void*)p.bx.bidx, u.bidx, u.nb * sizeof(int), hipMemcpyHostToDevice, st));
        LP_HIP(hipMemcpyAsync((void*)p.bx.binv, u.binv, u.n * sizeof(int), hipMemcpyHostToDevice, st));
    }
    if (u.gen) {     // sigma and t (caller's units); c_ext = [c'; 0; -c'_F] and the free columns' lists
        LP_HIP(vec(p.bx.Sg, u.sigma, u.n));
        LP_HIP(vec(p.bx.Tj, u.tshift, u.n));
        if (u.nf) {
            LP_HIP(vec(p.va.c + u.n + u.nb, u.cminus, u.nf));
            LP_HIP(hipMemcpyAsync((void*)p.bx.fidx, u.fidx, u.nf * sizeof(int), hipMemcpyHostToDevice, st));
            LP_HIP(hipMemcpyAsync((void*)p.bx.finv, u.finv, u.n * sizeof(int), hipMemcpyHostToDevice, st));
        }
    }
    return LPIPM_OK;
}
// ---- a request whose sources are in device memory (Upload::dev) ----
// One source: the farthest element its extents and strides address lies inside the device allocation of the context's
// device that holds its base.  A source of no elements is not looked at.
static int source_inside(const lpipm_ctx* c, const void* ptr, const Dim* dims, int ndims, size_t elem) {
    uint64_t bytes = 0;
    if (!span_bytes(dims, ndims, elem, &bytes)) return LPIPM_ERR_BAD_ARGUMENT;
    if (bytes == 0) return LPIPM_OK;
    if (!ptr) return LPIPM_ERR_BAD_ARGUMENT;
    hipPointerAttribute_t at{};
    if (hipPointerGetAttributes(&at, ptr) != hipSuccess) { (void)hipGetLastError(); return LPIPM_ERR_BAD_ARGUMENT; }   // (pageable host memory)
    if (at.type != hipMemoryTypeDevice || at.device != c->device) return LPIPM_ERR_BAD_ARGUMENT;
    hipDeviceptr_t base = nullptr;
    size_t size = 0;
    if (hipMemGetAddressRange(&base, &size, (hipDeviceptr_t)ptr) != hipSuccess) { (void)hipGetLastError(); return LPIPM_ERR_BAD_ARGUMENT; }
    return inside((uintptr_t)ptr, bytes, (uintptr_t)base, (uint64_t)size) ? LPIPM_OK : LPIPM_ERR_BAD_ARGUMENT;
}
// Every source of the descriptor, over everything a kernel of this upload may read: all n columns of a SLACK matrix (the
// hint test reads the slack block), the members as far as their strides go.
static int sources_inside(const lpipm_ctx* c, const Upload& u) {
    const lpipm_device_problem& d = *u.dev;
    const size_t el = src_elem_bytes(d.src_type);
    const uint64_t mats = member_strided(&d) ? d.count : 1;
    const uint64_t nb = u.m, nc = u.parts ? u.n - u.n_slack : u.n;
    const Dim a[3] = {{mats, d.A.member_stride}, {d.m, d.A.row_stride}, {d.n, d.A.col_stride}};
    const Dim e[2] = {{d.m_eq, d.A_eq.row_stride}, {d.n, d.A_eq.col_stride}};
    const Dim b[2] = {{d.count, d.b.member_stride}, {nb, d.b.stride}}, cc[2] = {{d.count, d.c.member_stride}, {nc, d.c.stride}};
    LP_TRY(source_inside(c, d.A.ptr, mats > 1 ? a : a + 1, mats > 1 ? 3 : 2, el));
    if (d.form == LPIPM_FORM_UB_EQ) LP_TRY(source_inside(c, d.A_eq.ptr, e, 2, el));
    LP_TRY(source_inside(c, d.b.ptr, d.count > 1 ? b : b + 1, d.count > 1 ? 2 : 1, el));
    LP_TRY(source_inside(c, d.c.ptr, d.count > 1 ? cc : cc + 1, d.count > 1 ? 2 : 1, el));
    return LPIPM_OK;
}
// slack_hint_holds on the device: one launch over the hinted columns of every matrix, one word back.
static int device_hint_holds(lpipm_ctx* c, const Upload& u, bool* holds) {
    const lpipm_device_problem& d = *u.dev;
    *holds = false;
    if (u.n_slack == 0 || u.n_slack == u.n) return LPIPM_OK;
    hipStream_t st = c->rs.st;
    if (!c->hint_dev) LP_HIP(hipMalloc((void**)&c->hint_dev, sizeof(int)));
    static const int one = 1;
    LP_HIP(hipMemcpyAsync(c->hint_dev, &one, sizeof(int), hipMemcpyHostToDevice, st));
    const bool own = member_strided(&d);
    const SlackHint h{d.A.ptr, d.A.row_stride, d.A.col_stride, own ? d.A.member_stride : 0, (long long)(u.n - u.n_slack),
                      (int)u.m, (int)u.n_slack, c->hint_dev};
    LP_HIP(launch_slack_hint(h, d.src_type == LPIPM_SRC_F32, own ? (int)d.count : 1, st));
    int word = 0;
    LP_HIP(hipMemcpyAsync(&word, c->hint_dev, sizeof(int), hipMemcpyDeviceToHost, st));
    LP_HIP(hipStreamSynchronize(st));
    *holds = word != 0;
    return LPIPM_OK;
}
// The launch that moves the descriptor's A into p's image(s): the `ub` and `eq` blocks of a request in parts are its two
// blocks of rows, each with the copy mode its own strides and alignment allow.
static PackMatrix pack_matrix_of(const Problem& p, const lpipm_device_problem& d) {
    const bool own = member_strided(&d);
    const size_t el = src_elem_bytes(d.src_type);
    auto block = [&](const lpipm_dev_matrix& M, uint64_t rows, uint64_t row0) {
        PackSeg s;
        if (rows == 0) return s;
        s.src = M.ptr; s.rs = M.row_stride; s.cs = M.col_stride; s.ms = own ? M.member_stride : 0;
        s.rows = (int)rows; s.row0 = (int)row0;
        s.mode = (int)pack_mode((uintptr_t)M.ptr, el, M.row_stride, M.col_stride, M.member_stride, own);
        return s;
    };
    PackMatrix pm;
    pm.seg[0] = block(d.A, d.m, 0);
    if (d.form == LPIPM_FORM_UB_EQ) pm.seg[1] = block(d.A_eq, d.m_eq, d.m);
    pm.dst = p.A; pm.ldd = p.npa; pm.dstride = own ? (long long)p.bstride : 0; pm.nx = p.nx;
    return pm;
}
// copy_in for device sources: one launch for A, one for b, c and c0 of every member; c0 goes through the staging block, as in
// update_lockstep_impl.
static int stage_grow(lpipm_ctx* c, size_t count);
static int copy_in_device(lpipm_ctx* c, const Upload& u, const double* c0v) {
    const lpipm_device_problem& d = *u.dev;
    Problem& p = c->p;
    hipStream_t st = c->rs.st;
    const bool f32 = d.src_type == LPIPM_SRC_F32;
    LP_HIP(launch_pack_matrix(pack_matrix_of(p, d), f32, member_strided(&d) ? (int)u.count : 1, st));
    const size_t count = (size_t)u.count;
    LP_TRY(stage_grow(c, count));
    std::memcpy(c->stage_host, c0v, count * sizeof(double));
    LP_HIP(hipMemcpyAsync(c->stage_dev, c->stage_host, count * sizeof(double), hipMemcpyHostToDevice, st));
    const bool many = u.count > 1;
    PackVectors pv;
    pv.seg[0] = PackVecSeg{d.b.ptr, d.b.stride, many ? d.b.member_stride : 0, (double*)p.va.b, (int)u.m};
    pv.seg[1] = PackVecSeg{d.c.ptr, d.c.stride, many ? d.c.member_stride : 0, (double*)p.va.c, (int)(u.parts ? (uint64_t)p.nx : u.n)};
    pv.c0_src = c->stage_dev; pv.c0_dst = p.va.S + S_C0; pv.dstride = (long long)p.bstride;
    LP_HIP(launch_pack_vectors(pv, f32, (int)u.count, st));
    return LPIPM_OK;
}
static int upload_impl(lpipm_ctx* c, const Upload& u) {
    LP_TRY(check_upload(c, u));
    // The hint is only used if the last n_slack columns of every member (of a shared batch's one matrix) really are [I; 0]
    // (ProblemBuilder::build guarantees it, linear_program.rs:147-156; parts have it by construction): else the upload is dense.
    bool hint = u.parts.has_value() || u.hint_verified;
    if (u.dev) {      // nothing is enqueued, and nothing of the resident problem touched, before the sources are known to be readable
        if (c->world > 1) return LPIPM_ERR_UNSUPPORTED;
        LP_HIP(hipSetDevice(c->device));
        LP_TRY(sources_inside(c, u));
        if (!hint) LP_TRY(device_hint_holds(c, u, &hint));
    } else if (!hint) hint = slack_hint_holds(u.shared ? 1 : u.count, u.m, u.n, u.A, u.lda, u.n_slack);
    const uint64_t n_slack = hint ? u.n_slack : 0, nx = u.n - n_slack;
    LP_HIP(hipSetDevice(c->device));
    destroy_views(c); // half-batch views hold copies of the geometry and of the device pointers
    c->first_valid = false;   // whatever is kept belongs to the matrix that is being replaced
    invalidate_duals(c);
    Problem& p = c->p;
    hipStream_t st = c->rs.st;
    const Geometry g = geometry_of(u, n_slack, c->first_cache, c->refine);
    if (!p.has_problem || !(g == p.geo)) LP_TRY(relayout(c, g));
    else {
        // same padded geometry: clear the whole state, so no stale (possibly non-finite) value of a
        // previous problem can sit in a padding lane
        LP_HIP(hipMemsetAsync(p.arena, 0, p.arena_bytes, st));
        if (p.a_shared) LP_HIP(hipMemsetAsync(p.a_shared, 0, p.a_shared_bytes, st));   // (a smaller m or n than before)
    }
    p.has_problem = false;     // until this upload is complete
    const int count = g.B;
    LP_TRY(scale_setup(c, g.mpv, g.npv, g.npa, u.shared ? 1 : count));      // (exponents per row and column of the vectors' lengths)
    p.ma = u.m; p.na = u.n; p.nb = (int)u.nb;
    p.m = u.m + u.nb; p.n = u.n + u.nb + u.nf; p.ns = (int)n_slack; p.nx = (int)nx;
    if (u.box) { p.bx.nb = (int)u.nb; p.bx.na = (int)u.n; p.bx.ma = (int)u.m; p.bx.nf = (int)u.nf; p.bx.gen = u.gen ? 1 : 0; }
    if (u.tall) p.tv.nx = (int)nx;            // (the padded geometry may be shared by several nx)
    const uint64_t m_ub = u.parts ? u.parts->m_ub : 0;
    p.me = u.tall_eq ? (int)u.me : 0;
    if (u.tall) { p.tv.ms = (int)m_ub; p.tv.me = p.me; }
    p.from_parts = u.parts.has_value(); p.owned_tall = u.owned;
    bind_systems(p);
    p.va.n = (int)p.n; p.va.m = (int)p.m; p.va.n_total = (long long)p.n; p.va.gs = nullptr; c->colsplit = false;   // lpipm_upload_nsplit overrides
    // A single LP's loop ends on the host, so its kernels need not test the done word (one dependent load
    // less at the start of ~100 short kernels) -- except the head of an iteration, which is enqueued before
    // the host has seen the previous status.  In a batch every kernel tests it.
    p.bt = Batch{count, (long long)p.bstride, count > 1 ? p.va.done : nullptr};
    p.bt_head = Batch{count, (long long)p.bstride, p.va.done};
    p.va.done_chk = p.bt.done;
    std::vector<double> c0v((size_t)count, 0.0);          // must outlive the asynchronous copies below
    for (int i = 0; i < count; ++i) c0v[i] = u.c0 ? u.c0[i] : 0.0;
    const std::vector<double> onesv(p.shared_factor ? (size_t)g.np : u.tall_eq ? (size_t)g.nxp : 0, 1.0);     // likewise
    if (p.shared_factor) LP_HIP(hipMemcpyAsync(p.ones, onesv.data(), onesv.size() * sizeof(double), hipMemcpyHostToDevice, st));
    for (int i = 0; i < count && u.tall_eq; ++i)     // the dinv of S = Zt.Zt^T (every member's own: launch_adat moves dinv with the member)
        LP_HIP(hipMemcpyAsync((char*)p.ones_k + (size_t)i * p.bstride, onesv.data(), onesv.size() * sizeof(double), hipMemcpyHostToDevice, st));
    LP_TRY(u.dev ? copy_in_device(c, u, c0v.data()) : copy_in(c, u, c0v.data()));
    // general bounds, on the unscaled image: b' = b - A.t by the pass over A (t is zero on the slack columns, so their block adds
    // nothing), then A' = A.diag(sigma).  Both ahead of the equilibration: the exponents are those of A'.
    if (u.gen && u.shifts) {
        LP_HIP(launch_gemv_n(p.A, p.npa, (int)u.m, p.npa, 1, p.bx.Tj, p.np, p.va.b, nullptr, p.Y, p.mp, st, -1.0, Batch{}, false));
        LP_HIP(hipMemcpyAsync((void*)p.va.b, p.Y, u.m * sizeof(double), hipMemcpyDeviceToDevice, st));
    }
    if (u.gen && u.reflects) { box_reflect(p.bx, p.A, p.npa, (int)nx, st); LP_HIP(hipGetLastError()); }
    if (p.scale_passes > 0) {   // equilibrate what was just copied: the solves see the scaled problem only
        const Batch members{count, (long long)p.bstride, nullptr, 0};
        LP_HIP(launch_equilibrate(p.sc, p.A, (int)u.m, g.mp, (int)nx, g.npa, (int)n_slack, p.scale_passes, st,
                                  u.shared ? Batch{} : members));
        // bounded: the bound rows and their slack columns take their exponents from the bounded columns' (the block stays 1)
        if (u.box) { box_exponents(p.bx, p.sc.kr, p.sc.kc, st); LP_HIP(hipGetLastError()); }
        LP_HIP(launch_scale_vectors(p.sc, (double*)p.va.b, (int)p.m, (double*)p.va.c, (int)p.n, st, members));
    }
    // tall: the resident transpose, from the X the solves see (behind the equilibration: both copies carry its exponents)
    //       (every member's own, in one launch, when the members own their matrices)
    //       (of the `ub` rows alone when there are `eq` rows: K is built from them)
    if (u.tall) LP_HIP(tall_transpose(p.A, g.npa, (int)(u.tall_eq ? m_ub : u.m), (int)nx, p.Xt, g.mk, st, u.shared ? Batch{} : Batch{count, (long long)p.bstride, nullptr, 0}));
    LP_HIP(hipStreamSynchronize(st));   // the caller's arrays, c0v and onesv are free again from here
    p.has_problem = true;
    for (NormalSystem& sy : p.sys) sy.res.counters_dirty = true;
    bind_status_pinned(c, true);
    return LPIPM_OK;
}

extern "C" int lpipm_upload(lpipm_ctx* c, uint64_t m, uint64_t n, const double* A, uint64_t lda,
                            const double* b, const double* cc, double c0) {
    return lpipm_upload_slack(c, m, n, A, lda, b, cc, c0, 0);
}
extern "C" int lpipm_upload_slack(lpipm_ctx* c, uint64_t m, uint64_t n, const double* A, uint64_t lda,
                                  const double* b, const double* cc, double c0, uint64_t n_slack) {
    return upload_impl(c, Upload{.m = m, .n = n, .n_slack = n_slack, .A = &A, .lda = lda, .b = &b, .c = &cc, .c0 = &c0});
}
extern "C" int lpipm_upload_ub_eq(lpipm_ctx* c, uint64_t n, uint64_t m_ub, const double* A_ub, uint64_t lda_ub,
                                  const double* b_ub, uint64_t m_eq, const double* A_eq, uint64_t lda_eq,
                                  const double* b_eq, const double* cc, double c0) {
    return upload_impl(c, Upload{.m = m_ub + m_eq, .n = n + m_ub, .n_slack = m_ub,
                                 .parts = UploadParts{m_ub, A_ub, lda_ub, b_ub, A_eq, lda_eq, b_eq}, .c = &cc, .c0 = &c0});
}
// lpipm_upload_ub_eq's LP with upper bounds on some of its structural columns: the bounded form (kernels_box.hip).  Without a
// finite bound it is lpipm_upload_ub_eq's request itself.  The index lists and the packed bounds live until upload_impl returns.
extern "C" int lpipm_upload_bounded(lpipm_ctx* c, uint64_t n, uint64_t m_ub, const double* A_ub, uint64_t lda_ub,
                                    const double* b_ub, uint64_t m_eq, const double* A_eq, uint64_t lda_eq,
                                    const double* b_eq, const double* cc, double c0, const double* upper) {
    std::vector<int> bidx, binv;
    std::vector<double> ub;
    bool bad = false;
    if (upper && n <= (1u << 24)) {
        binv.assign((size_t)(n + m_ub), -1);
        for (uint64_t j = 0; j < n; ++j) {
            const double uj = upper[j];
            if (uj != uj || (std::isinf(uj) && uj < 0.0)) { bad = true; break; }
            if (std::isinf(uj)) continue;
            binv[(size_t)j] = (int)bidx.size();
            bidx.push_back((int)j);
            ub.push_back(uj);
        }
    }
    if (!bad && bidx.empty()) return lpipm_upload_ub_eq(c, n, m_ub, A_ub, lda_ub, b_ub, m_eq, A_eq, lda_eq, b_eq, cc, c0);
    Upload u{.m = m_ub + m_eq, .n = n + m_ub, .n_slack = m_ub,
             .parts = UploadParts{m_ub, A_ub, lda_ub, b_ub, A_eq, lda_eq, b_eq}, .c = &cc, .c0 = &c0, .keep_ok = false};
    u.box = !bad; u.nb = bad ? 0 : bidx.size(); u.bidx = bidx.data(); u.binv = binv.data(); u.ub = ub.data(); u.upper_bad = bad;
    return upload_impl(c, u);
}
// lpipm_upload_ub_eq's LP with lower_j <= x_j <= upper_j on its structural columns.  Per column: a finite lower
// end is a shift t_j = lower_j (with a finite upper end: the bounded form's column, u'_j = upper_j - lower_j); only an upper end
// is the reflection x_j = upper_j - x'_j; neither is a free column, x_j = x'_j - x^-_j, which keeps ONE stored column.  What
// goes resident is the primed LP (c' = sigma c and c0' = c0 + c.t from here; b' = b - A.t and A' = A.diag(sigma) by upload_impl
// on the device).  With no free column, no reflection and no shift this is lpipm_upload_bounded's request itself.
extern "C" int lpipm_upload_bounds(lpipm_ctx* c, uint64_t n, uint64_t m_ub, const double* A_ub, uint64_t lda_ub,
                                   const double* b_ub, uint64_t m_eq, const double* A_eq, uint64_t lda_eq,
                                   const double* b_eq, const double* cc, double c0, const double* lower, const double* upper) {
    std::vector<int> bidx, binv, fidx, finv;
    std::vector<double> ub, sigma, tshift, cprime, cminus;
    int code = LPIPM_OK;
    double c0p = c0;                                              // c0' = c0 + c.t
    bool reflects = false, shifts = false;
    // (else check_upload refuses the request, by its shape or its null c, before anything is sized or read)
    const bool sized = n <= (1u << 24) && m_ub <= (1u << 20) && cc != nullptr;
    if (sized) {
        const size_t na = (size_t)(n + m_ub);
        binv.assign(na, -1); finv.assign(na, -1); sigma.assign(na, 1.0); tshift.assign(na, 0.0); cprime.assign((size_t)n, 0.0);
        bool crossed = false;
        for (uint64_t j = 0; j < n && code == LPIPM_OK; ++j) {
            const double lj = lower ? lower[j] : 0.0, uj = upper ? upper[j] : INFINITY;
            if (lj != lj || uj != uj || (std::isinf(lj) && lj > 0.0) || (std::isinf(uj) && uj < 0.0)) { code = LPIPM_ERR_BAD_ARGUMENT; break; }
            if (lj > uj) crossed = true;
            const bool has_l = !std::isinf(lj), has_u = !std::isinf(uj);
            if (has_l) {
                tshift[(size_t)j] = lj;
                if (has_u) { binv[(size_t)j] = (int)bidx.size(); bidx.push_back((int)j); ub.push_back(uj - lj); }
            } else if (has_u) { sigma[(size_t)j] = -1.0; tshift[(size_t)j] = uj; reflects = true; }
            else { finv[(size_t)j] = (int)fidx.size(); fidx.push_back((int)j); }
            shifts = shifts || tshift[(size_t)j] != 0.0;
            cprime[(size_t)j] = sigma[(size_t)j] * cc[j];
            c0p += cc[j] * tshift[(size_t)j];
        }
        if (code == LPIPM_OK && crossed) code = LPIPM_INFEASIBLE;     // lower_j > upper_j: no point satisfies the bounds
        if (code == LPIPM_OK && fidx.empty() && !reflects && !shifts)
            return lpipm_upload_bounded(c, n, m_ub, A_ub, lda_ub, b_ub, m_eq, A_eq, lda_eq, b_eq, cc, c0, upper);
        for (int j : fidx) cminus.push_back(-cprime[(size_t)j]);
    }
    const double* cp = sized && code == LPIPM_OK ? cprime.data() : cc;
    Upload u{.m = m_ub + m_eq, .n = n + m_ub, .n_slack = m_ub,
             .parts = UploadParts{m_ub, A_ub, lda_ub, b_ub, A_eq, lda_eq, b_eq}, .c = &cp, .c0 = &c0p, .keep_ok = false};
    u.bounds_code = code;
    if (sized && code == LPIPM_OK) {
        u.box = u.gen = true; u.nb = bidx.size(); u.bidx = bidx.data(); u.binv = binv.data(); u.ub = ub.data();
        u.nf = fidx.size(); u.fidx = fidx.data(); u.finv = finv.data();
        u.sigma = sigma.data(); u.tshift = tshift.data(); u.cminus = cminus.data(); u.reflects = reflects; u.shifts = shifts;
    }
    return upload_impl(c, u);
}
// The request of one tall LP (cc, c0: one entry each).
static Upload tall_request(uint64_t n, uint64_t m_ub, const double* A_ub, uint64_t lda_ub, const double* b_ub, const double* const* cc,
                           const double* c0) {
    return Upload{.m = m_ub, .n = n + m_ub, .n_slack = m_ub, .parts = UploadParts{.m_ub = m_ub, .A_ub = A_ub, .lda_ub = lda_ub, .b_ub = b_ub},
                  .c = cc, .c0 = c0, .tall = true, .keep_ok = false};
}
extern "C" int lpipm_upload_ub_tall(lpipm_ctx* c, uint64_t n, uint64_t m_ub, const double* A_ub, uint64_t lda_ub,
                                    const double* b_ub, const double* cc, double c0) {
    return upload_impl(c, tall_request(n, m_ub, A_ub, lda_ub, b_ub, &cc, &c0));
}
// A tall LP with equality rows.  Without any it is lpipm_upload_ub_tall's request itself.
extern "C" int lpipm_upload_ub_eq_tall(lpipm_ctx* c, uint64_t n, uint64_t m_ub, const double* A_ub, uint64_t lda_ub,
                                       const double* b_ub, uint64_t m_eq, const double* A_eq, uint64_t lda_eq,
                                       const double* b_eq, const double* cc, double c0) {
    if (m_eq == 0) return upload_impl(c, tall_request(n, m_ub, A_ub, lda_ub, b_ub, &cc, &c0));
    return upload_impl(c, Upload{.m = m_ub + m_eq, .n = n + m_ub, .n_slack = m_ub,
                                 .parts = UploadParts{m_ub, A_ub, lda_ub, b_ub, A_eq, lda_eq, b_eq}, .c = &cc, .c0 = &c0,
                                 .tall = true, .tall_eq = true, .me = m_eq, .keep_ok = false});
}
extern "C" int lpipm_upload_lockstep(lpipm_ctx* c, uint64_t count, uint64_t m, uint64_t n, const double* const* A,
                                     const double* const* b, const double* const* cc, const double* c0) {
    return lpipm_upload_lockstep_slack(c, count, m, n, A, b, cc, c0, 0);
}
extern "C" int lpipm_upload_lockstep_slack(lpipm_ctx* c, uint64_t count, uint64_t m, uint64_t n, const double* const* A,
                                           const double* const* b, const double* const* cc, const double* c0, uint64_t n_slack) {
    return upload_impl(c, Upload{.count = count, .m = m, .n = n, .n_slack = n_slack, .A = A, .lda = n, .b = b, .c = cc, .c0 = c0});
}
extern "C" int lpipm_upload_lockstep_shared(lpipm_ctx* c, uint64_t count, uint64_t m, uint64_t n, const double* A, uint64_t lda,
                                            const double* const* b, const double* const* cc, const double* c0) {
    return lpipm_upload_lockstep_shared_slack(c, count, m, n, A, lda, b, cc, c0, 0);
}
extern "C" int lpipm_upload_lockstep_shared_slack(lpipm_ctx* c, uint64_t count, uint64_t m, uint64_t n, const double* A, uint64_t lda,
                                                  const double* const* b, const double* const* cc, const double* c0, uint64_t n_slack) {
    return upload_impl(c, Upload{.count = count, .m = m, .n = n, .n_slack = n_slack, .A = &A, .lda = lda, .b = b, .c = cc, .c0 = c0,
                                 .shared = true});
}
extern "C" int lpipm_upload_lockstep_shared_ub_eq(lpipm_ctx* c, uint64_t count, uint64_t n, uint64_t m_ub, const double* A_ub,
                                                  uint64_t lda_ub, uint64_t m_eq, const double* A_eq, uint64_t lda_eq,
                                                  const double* const* b, const double* const* cc, const double* c0) {
    return upload_impl(c, Upload{.count = count, .m = m_ub + m_eq, .n = n + m_ub, .n_slack = m_ub,
                                 .parts = UploadParts{.m_ub = m_ub, .A_ub = A_ub, .lda_ub = lda_ub, .A_eq = A_eq, .lda_eq = lda_eq}, .b = b, .c = cc, .c0 = c0, .shared = true});
}
extern "C" int lpipm_upload_lockstep_shared_ub_tall(lpipm_ctx* c, uint64_t count, uint64_t n, uint64_t m_ub, const double* A_ub,
                                                    uint64_t lda_ub, const double* const* b, const double* const* cc,
                                                    const double* c0) {
    if (!c) return LPIPM_ERR_BAD_ARGUMENT;       // (this entry alone refuses a null context before it looks at the shape)
    return upload_impl(c, Upload{.count = count, .m = m_ub, .n = n + m_ub, .n_slack = m_ub,
                                 .parts = UploadParts{.m_ub = m_ub, .A_ub = A_ub, .lda_ub = lda_ub}, .b = b, .c = cc, .c0 = c0, .shared = true,
                                 .tall = true, .keep_ok = false});
}
// The same batch with `eq` rows in the one image: every member a tall LP with equality rows.  Without any it is
// lpipm_upload_lockstep_shared_ub_tall's request itself.
extern "C" int lpipm_upload_lockstep_shared_ub_eq_tall(lpipm_ctx* c, uint64_t count, uint64_t n, uint64_t m_ub, const double* A_ub,
                                                       uint64_t lda_ub, uint64_t m_eq, const double* A_eq, uint64_t lda_eq,
                                                       const double* const* b, const double* const* cc, const double* c0) {
    if (m_eq == 0) return lpipm_upload_lockstep_shared_ub_tall(c, count, n, m_ub, A_ub, lda_ub, b, cc, c0);
    return upload_impl(c, Upload{.count = count, .m = m_ub + m_eq, .n = n + m_ub, .n_slack = m_ub,
                                 .parts = UploadParts{.m_ub = m_ub, .A_ub = A_ub, .lda_ub = lda_ub, .A_eq = A_eq, .lda_eq = lda_eq}, .b = b, .c = cc,
                                 .c0 = c0, .shared = true, .tall = true, .tall_eq = true, .me = m_eq, .keep_ok = false});
}
// The request of a tall batch whose members own their matrices (A_ub[i]: m_ub x n, lda_ub).
static Upload owned_tall_request(uint64_t count, uint64_t n, uint64_t m_ub, const double* const* A_ub, uint64_t lda_ub,
                                 const double* const* b, const double* const* cc, const double* c0) {
    return Upload{.count = count, .m = m_ub, .n = n + m_ub, .n_slack = m_ub, .A = A_ub, .lda = lda_ub,
                  .parts = UploadParts{.m_ub = m_ub}, .b = b, .c = cc, .c0 = c0, .tall = true, .owned = true, .keep_ok = false};
}
extern "C" int lpipm_upload_lockstep_ub_tall(lpipm_ctx* c, uint64_t count, uint64_t n, uint64_t m_ub, const double* const* A_ub,
                                             uint64_t lda_ub, const double* const* b, const double* const* cc, const double* c0) {
    if (!c) return LPIPM_ERR_BAD_ARGUMENT;       // (as the shared tall batch: a null context before the shape)
    return upload_impl(c, owned_tall_request(count, n, m_ub, A_ub, lda_ub, b, cc, c0));
}
// The request of the host entry the descriptor stands for, with the descriptor as its source.  The pointer arrays hold the
// descriptor's base pointers, member after member alike: check_upload asks only whether they are null.
struct DeviceRequest { std::vector<const double*> Av, bv, cv; Upload u; };
static int device_request(const lpipm_device_problem* d, DeviceRequest& q) {
    if (!d) return LPIPM_ERR_BAD_ARGUMENT;
    HostEntry entry;
    if (const int rc = entry_of(d, &entry); rc != LPIPM_OK) return rc;
    if (!strides_ok(d)) return LPIPM_ERR_BAD_ARGUMENT;
    if ((d->form != LPIPM_FORM_UB_EQ && d->m_eq != 0) || (d->form != LPIPM_FORM_SLACK && d->n_slack != 0)) return LPIPM_ERR_BAD_ARGUMENT;
    const uint64_t K = d->count, m = d->m, n = d->n;
    const double *A = (const double*)d->A.ptr, *A_eq = (const double*)d->A_eq.ptr, *b = (const double*)d->b.ptr, *cc = (const double*)d->c.ptr;
    q.Av.assign((size_t)K, A); q.bv.assign((size_t)K, b); q.cv.assign((size_t)K, cc);
    const std::vector<const double*>&Av = q.Av, &bv = q.bv, &cv = q.cv;
    Upload& u = q.u;
    switch (entry) {
    case HostEntry::Slack: case HostEntry::LockstepSlack:
        u = Upload{.count = K, .m = m, .n = n, .n_slack = d->n_slack, .A = Av.data(), .lda = n, .b = bv.data(), .c = cv.data(), .c0 = d->c0};
        break;
    case HostEntry::SharedSlack:
        u = Upload{.count = K, .m = m, .n = n, .n_slack = d->n_slack, .A = Av.data(), .lda = n, .b = bv.data(), .c = cv.data(), .c0 = d->c0,
                   .shared = true};
        break;
    case HostEntry::UbEq:
        u = Upload{.m = m + d->m_eq, .n = n + m, .n_slack = m, .parts = UploadParts{m, A, n, b, A_eq, n, b}, .c = cv.data(), .c0 = d->c0};
        break;
    case HostEntry::SharedUbEq:
        u = Upload{.count = K, .m = m + d->m_eq, .n = n + m, .n_slack = m,
                   .parts = UploadParts{.m_ub = m, .A_ub = A, .lda_ub = n, .A_eq = A_eq, .lda_eq = n}, .b = bv.data(), .c = cv.data(), .c0 = d->c0,
                   .shared = true};
        break;
    case HostEntry::UbTall: u = tall_request(n, m, A, n, b, cv.data(), d->c0); break;
    case HostEntry::SharedUbTall:
        u = Upload{.count = K, .m = m, .n = n + m, .n_slack = m, .parts = UploadParts{.m_ub = m, .A_ub = A, .lda_ub = n}, .b = bv.data(),
                   .c = cv.data(), .c0 = d->c0, .shared = true, .tall = true, .keep_ok = false};
        break;
    case HostEntry::LockstepUbTall: u = owned_tall_request(K, n, m, Av.data(), n, bv.data(), cv.data(), d->c0); break;
    default: return LPIPM_ERR_BAD_ARGUMENT;
    }
    u.dev = d;
    return LPIPM_OK;
}
extern "C" int lpipm_upload_device(lpipm_ctx* c, const lpipm_device_problem* d) {
    if (!c) return LPIPM_ERR_BAD_ARGUMENT;
    DeviceRequest q;
    LP_TRY(device_request(d, q));
    return upload_impl(c, q.u);
}

// ------------------------------------------------------------------------------------------------
// Y = add + A.W and Upart = row-split slabs of A^T.V on the stored structural columns, plus the
// identity block of the slack columns
static hipError_t ctx_gemv_n(lpipm_ctx* c, int nrhs, const double* W, const double* add0, const double* add1, double* Y,
                             const Batch& bt, hipStream_t on = nullptr) {
    hipStream_t st = on ? on : c->rs.st;
    ++c->gemv_passes;
    hipError_t e = launch_gemv_n(c->p.A, c->p.npa, (int)c->p.ma, c->p.npa, nrhs, W, c->p.np, add0, add1, Y, c->p.mp, st, 1.0, bt, c->p.shared_a);
    if (e != hipSuccess) return e;
    return launch_slack_n(c->p.ns, c->p.nx, nrhs, W, c->p.np, Y, c->p.mp, st, bt);
}
static hipError_t ctx_gemv_t(lpipm_ctx* c, int nrhs, const double* V, const Batch& bt) {
    ++c->gemv_passes;
    // (tall: slabs npa wide; the slack columns' part of A^T.v is v itself, and the consumers take it from there)
    if (c->p.tall) return launch_gemv_t(c->p.A, c->p.npa, c->p.mp, c->p.npa, nrhs, V, c->p.mp, c->p.ATpart, c->rs.st, c->p.npa, bt, c->p.shared_a);
    hipError_t e = launch_gemv_t(c->p.A, c->p.npa, c->p.mp, c->p.npa, nrhs, V, c->p.mp, c->p.ATpart, c->rs.st, c->p.np, bt, c->p.shared_a);
    if (e != hipSuccess) return e;
    return launch_slack_t(c->p.ns, c->p.nx, nrhs, c->p.nsplit, V, c->p.mp, c->p.ATpart, c->p.np, c->rs.st, bt);
}
// both in one read of A: chunk slabs of A.w into AxPart (gemv_dual_chunks(npa) of them), row-split slabs of A^T.v into ATpart
static hipError_t ctx_gemv_dual(lpipm_ctx* c, const double* W, const double* V, double* AxPart, const Batch& bt) {
    ++c->gemv_passes;
    if (c->p.tall) {   // slabs of A^T.v npa wide (see ctx_gemv_t); w_s into chunk slab 0 of A.w
        hipError_t et = launch_gemv_dual(c->p.A, c->p.npa, c->p.mp, c->p.npa, W, V, AxPart, c->p.ATpart, c->p.npa, c->rs.st, bt, c->p.shared_a);
        if (et != hipSuccess) return et;
        return launch_slack_n(c->p.ns, c->p.nx, 1, W, c->p.np, AxPart, c->p.mp, c->rs.st, bt);
    }
    hipError_t e = launch_gemv_dual(c->p.A, c->p.npa, c->p.mp, c->p.npa, W, V, AxPart, c->p.ATpart, c->p.np, c->rs.st, bt, c->p.shared_a);
    if (e != hipSuccess) return e;
    // the slack terms of both products in one launch: w_s into chunk slab 0, v into row-split slab 0 (zeros into the others)
    return launch_slack_dual(c->p.ns, c->p.nx, c->p.nsplit, W, V, AxPart, c->p.ATpart, c->p.np, c->rs.st, bt);
}

// The switches of the ONE iteration being enqueued: made by whoever enqueues it, handed down by reference, kept nowhere.
struct Iter {
    bool on_first = false;       // it works in the kept first system (iteration 1 of a solve that uses the kept first factor) ...
    bool skip_factor = false;    //   ... which already hold its factor: no A.D.A^T, no factorisation
    bool refine_now = false;     // it refines its solves (host mirror of the LPs' skip_refine words)
};
// The system of that iteration, and whether it is the ONE kept factor of a whole shared-matrix batch.
static NormalSystem& cur_sys(lpipm_ctx* c, const Iter& it) { return c->p.sys[it.on_first ? SYS_FIRST : SYS_WORK]; }
static bool shared_first(const lpipm_ctx* c, const Iter& it) { return it.on_first && c->p.shared_factor; }
// The same `bytes` of every member the context covers, on its stream: copied device to device from src to dst (both in the
// members' arenas, bstride apart, from member bt.first on), device to host into dst (packed, `bytes` apart, from its start), or
// zeroed (src null).  One member: the runtime's plain call, several: its 2-D one -- which of the runtime's kernels runs, and
// shows in a trace, follows from that choice.
static hipError_t member_bytes(lpipm_ctx* c, void* dst, const void* src, size_t bytes, hipMemcpyKind kind = hipMemcpyDeviceToDevice) {
    const size_t off = (size_t)c->p.bt.first * c->p.bstride, pitch = c->p.bstride, B = (size_t)c->p.B;
    const bool to_host = kind == hipMemcpyDeviceToHost;
    char* d = (char*)dst + (to_host ? 0 : off);
    const char* s = src ? (const char*)src + off : nullptr;
    if (B == 1) return s ? hipMemcpyAsync(d, s, bytes, kind, c->rs.st) : hipMemsetAsync(d, 0, bytes, c->rs.st);
    return s ? hipMemcpy2DAsync(d, to_host ? bytes : pitch, s, pitch, bytes, B, kind, c->rs.st) : hipMemset2DAsync(d, pitch, 0, bytes, B, c->rs.st);
}
// The pivot-failure words of the LPs this context covers, between the solver's word and its kept copy (device to device).
// A shared-matrix batch's one kept word goes to every LP (the other direction does not exist: the build wrote it).
static hipError_t copy_info(lpipm_ctx* c, int32_t* dst, const int32_t* src) {
    if (c->p.shared_factor && src == c->p.sys[SYS_FIRST].info) {
        ScatterRows<int32_t> w;
        w.seg[0].dst = dst; w.seg[0].src = src; w.seg[0].ld = 0; w.seg[0].len = 1;
        vec_scatter_rows(w, c->rs.st, c->p.bt);
        return hipGetLastError();
    }
    return member_bytes(c, dst, src, sizeof(int32_t));
}
// Builds system s for the members of bt: its one A.D.A^T launch, then its diagonal add-on.  Nothing else fills an AdatLaunch.
struct BuildOpts {
    const double* dinv = nullptr;    // instead of the system's own (and of its add-on's vector, where that is the same one)
    double* M2 = nullptr;            // a second copy of M, which is factored in place: a refining context's M0 (null otherwise)
    bool signal_groups = false;      // the column-split pipeline (launch_adat, armed with ev_c0): the caller reduces M group by group
                                     //   behind the launch and makes the copy itself; no structural slack there, nothing is added
};
static hipError_t build_system(lpipm_ctx* c, NormalSystem& s, const Batch& bt, const BuildOpts& o = BuildOpts{}) {
    NormalSystem& src = s.twin ? c->p.sys[SYS_WORK] : s;
    hipStream_t st = c->rs.st;
    AdatLaunch a{};
    a.A = src.A; a.lda = src.lda; a.dinv = o.dinv ? o.dinv : src.dinv; a.M = s.M; a.ldm = s.ld; a.M2 = o.M2;
    a.K = src.K; a.diag_pad_from = src.diag_pad_from; a.batch = bt; a.shared_a = src.shared_a;
    bool second_copy = false;
    hipError_t e = launch_adat(src.ap, src.res, a, o.signal_groups, st, &second_copy, o.signal_groups ? c->ev_c0 : nullptr);
    if (e != hipSuccess || o.signal_groups || !src.d) return e;
    const double* d = o.dinv && src.d == src.dinv ? o.dinv : src.d;
    e = launch_slack_diag(src.ns, src.nx, d, s.M, s.ld, st, bt);
    if (e != hipSuccess || !o.M2) return e;
    if (second_copy) return launch_slack_diag(src.ns, src.nx, d, o.M2, s.ld, st, bt);
    vec_copy_lower(s.M, o.M2, s.n, s.n, st, bt);          // the launch could not write it: copied afterwards
    return hipGetLastError();
}

// Tall form with equality rows, once per iteration behind K = L.L^T: Zt = A_eq.L^-T from the `eq` rows of the (scaled) image,
// S = Zt.Zt^T = A_eq.K^-1.A_eq^T by the A.D.A^T module, S = L_S.L_S^T.
// A failed pivot of S lands in the word K's does: dependent equality rows, or more of them than columns, are NumericalProblem.
// factor == false (lpipm_k_tall_schur): S is left as built.
// A batch over one image (lpipm_upload_lockstep_shared_ub_eq_tall): every launch covers the members of bt.  The `eq` rows are
// the one image's (shared_b); Zt, S, their plans' inverses and the pivot word are each member's own, so a failed pivot of K or
// of S ends that member alone.
static int tall_eq_schur(lpipm_ctx* c, bool factor = true) {
    const TallArgs& t = c->p.tv;
    hipStream_t st = c->rs.st;
    const Batch& bt = c->p.bt;
    NormalSystem& S = c->p.sys[SYS_SCHUR];
    LP_HIP(launch_trsm_lt(c->p.A + (size_t)t.ms * c->p.npa, c->p.npa, t.me, c->p.npa, *c->p.sys[SYS_WORK].factor, c->p.Zt, t.nxp, st, bt, c->p.shared_a));
    LP_HIP(build_system(c, S, bt));
    if (!factor) return LPIPM_OK;
    LP_HIP(launch_potrf(*S.factor, S.info, st, bt, nullptr, false, nullptr));
    if (t.me > t.nx) {       // rank(S) <= nx < me: the zero pivot of exact arithmetic, which rounding may have left positive
        tall_eq_singular(c->p.va, t, st);
        LP_HIP(hipGetLastError());
    }
    return LPIPM_OK;
}
// ... and per sym_solve, in place of u_x = K^-1.g (g in G, the `eq` part of r2 behind its ms `ub` entries):
//   w = L^-1.g;  h = r2_e - Zt.w;  v_e = S^-1.h;  w += Zt^T.v_e;  u_x = L^-T.w
// The forward half leaves w in Y, the backward half takes it from there and leaves u_x in G; v_e stays in Ve for the epilogue.
// (The shorter form that keeps the solve on K whole -- y0 = K^-1.g, u_x = y0 + K^-1.A_eq^T.v_e -- was emulated up to 68 x worse
// in x and is not to be built: DESIGN.md 3.10.)
static int tall_eq_reduced_solve(lpipm_ctx* c, int nrhs, const double* r2a, const double* r2b) {
    const TallArgs& t = c->p.tv;
    hipStream_t st = c->rs.st;
    const FactorPlan& fk = *c->p.sys[SYS_WORK].factor;
    const Batch& bt = c->p.bt;
    LP_HIP(launch_chol_solve(fk, nrhs, t.G, c->p.Y, st, bt, SolveSteps{0, -1, false}));
    prof_mark(c, T_TRSV);
    LP_HIP(launch_gemv_n(c->p.Zt, t.nxp, t.me, t.nxp, nrhs, c->p.Y, t.nxp, r2a + t.ms, r2b ? r2b + t.ms : nullptr, t.Ve, t.mep, st, -1.0, bt));
    prof_mark(c, T_GEMV);
    LP_HIP(launch_chol_solve(*c->p.sys[SYS_SCHUR].factor, nrhs, t.Ve, c->p.H, st, bt));
    prof_mark(c, T_TRSV);
    LP_HIP(launch_gemv_t(c->p.Zt, t.nxp, t.mep, t.nxp, nrhs, t.Ve, t.mep, c->p.ZtPart, st, t.nxp, bt));
    prof_mark(c, T_GEMV);
    tall_eq_add_w(c->p.va, t, nrhs, c->p.Y, c->p.ZtPart, st);
    LP_HIP(hipGetLastError());
    prof_mark(c, T_VEC);
    LP_HIP(launch_chol_solve(fk, nrhs, t.G, c->p.Y, st, bt, SolveSteps{(int)fk.sbs.size(), -1, true}));
    return LPIPM_OK;
}
// What an earlier solve on the same upload may have left behind.  v_e is solved in place over all mep entries of Ve,
// of which the pass over Zt writes the first me only: a solve whose K or S lost a pivot, or whose iterate held a NaN, leaves NaN
// in the padding, and the next solve on the same upload -- of the same LP, or of the one new vectors put in its place -- would
// multiply it into Zt^T.v_e (0 * NaN) and end in NumericalProblem at its first iteration.  Ve of every LP this context covers
// goes back to zero ahead of a solve, and ahead of the kernel entries that run the reduced solve.
static int tall_eq_reset(lpipm_ctx* c) {
    if (!c->p.tall_eq) return LPIPM_OK;
    LP_HIP(member_bytes(c, c->p.tv.Ve, nullptr, 2 * (size_t)c->p.tv.mep * sizeof(double)));
    return LPIPM_OK;
}

// Bounded form, likewise: the solves run in place over all mps entries of both rows of Rs, of which the pass A.W writes the
// first ma only (k_blind_start clears the padding of va.R, which on this form the solves do not work in).
static int box_reset(lpipm_ctx* c) {
    if (!c->p.box) return LPIPM_OK;
    LP_HIP(member_bytes(c, c->p.bx.Rs, nullptr, 2 * (size_t)c->p.bx.mps * sizeof(double)));
    return LPIPM_OK;
}

// R = A.W + r2 for the nrhs right-hand sides whose r2 are add0, add1 (newton_equations.rs:220), on the solver's stream or `on`.
// Column split: the addends enter once, after the cross-rank sum of the ranks' products.
static int pass_aw(lpipm_ctx* c, int nrhs, const double* add0, const double* add1, hipStream_t on = nullptr) {
    VecArgs& v = c->p.va;
    if (!c->colsplit) { LP_HIP(ctx_gemv_n(c, nrhs, c->p.solW, add0, add1, c->p.solR, c->p.bt, on)); return LPIPM_OK; }
    LP_HIP(ctx_gemv_n(c, nrhs, v.W, nullptr, nullptr, v.R, c->p.bt, on));
    LP_TRY(ctx_allreduce(c, v.R, (uint64_t)nrhs * c->p.mp, 0, on));
    vec_add_rows((int)c->p.m, nrhs, v.R, c->p.mp, add0, add1, on ? on : c->rs.st);
    return LPIPM_OK;
}

// v = M^-1 r through the Cholesky factor f with one step of iterative refinement against the matrix itself (LPIPM_REFINE, see
// lpipm_ctx::refine):  v0 = L^-T L^-1 r;  rho = r - M.v0 (doubled precision, one read of the lower triangle);  v = v0 + L^-T L^-1 rho.
// R: nrhs x mp, in/out.
static int chol_solve_refined(lpipm_ctx* c, const FactorPlan& f, int nrhs, double* R, hipStream_t st) {
    const Batch& bt = c->p.bt;
    // the refinement's launches skip an LP whose own word says so (a finished one, or one that does not need it yet)
    const Batch br = c->refine == 2 ? bt : Batch{bt.count, bt.stride, c->p.va.skip_refine, bt.first};
    vec_rows_copy(c->p.mp, nrhs, c->p.R0, R, st, br);
    LP_HIP(launch_chol_solve(f, nrhs, R, c->p.Y, st, bt));
    LP_HIP(launch_symv_residual(c->p.M0, c->p.mp, c->p.mp, nrhs, R, c->p.mp, c->p.R0, c->p.mp, c->p.Rho, c->p.mp, c->p.symv_ws, st, br));
    LP_HIP(launch_chol_solve(f, nrhs, c->p.Rho, c->p.Y, st, br));
    vec_rows_add(c->p.mp, nrhs, R, c->p.Rho, st, br);
    LP_HIP(hipGetLastError());
    return LPIPM_OK;
}
// R <- M^-1.R (nrhs x mp, in place) with the dense system of this iteration (newton_equations.rs:151-169), on the solver's stream
// or `on`; the arm is chosen here and nowhere else: QR, the refined Cholesky solve, or the steps given of the Cholesky sweep (all of
// them, unless the first ran beside the chain).
static int normal_solve(lpipm_ctx* c, const Iter& it, const lpipm_opts* o, int nrhs, const SolveSteps& steps = SolveSteps{}, hipStream_t on = nullptr) {
    hipStream_t st = on ? on : c->rs.st;
    double* R = c->p.solR;
    const NormalSystem& sys = cur_sys(c, it);        // (the QR arms and a refining context keep no first factor: the working system)
    if (o->solver_type != LPIPM_SOLVER_CHOLESKY) LP_HIP(launch_qr_solve(sys.M, sys.n, sys.n, c->p.tau, nrhs, R, c->p.va.potrf_info, st));   // :155-166
    else if (it.refine_now) LP_TRY(chol_solve_refined(c, *sys.factor, nrhs, R, st));
    else LP_HIP(launch_chol_solve(*sys.factor, nrhs, R, c->p.Y, st, c->p.bt, steps, shared_first(c, it)));   // :154
    return LPIPM_OK;
}

static int enqueue_residuals(lpipm_ctx* c, int is_init, int ip_next, double tol) {
    VecArgs& v = c->p.va;
    // A.x and A^T.y at the current point (residual.rs:23,25)
    XRank xr{xrank_fn, c};
    if (!(c->colsplit && c->world > 1)) {       // both products in one read of A
        v.ax_chunks = gemv_dual_chunks(c->p.npa);
        const double* x_in = v.x;
        if (c->p.box && c->p.bx.nf > 0) {       // free columns: the pass reads the net vector x' - x^- (the only change to its input)
            box_net(v, c->p.bx, v.x, 0, c->p.bx.Xn, 0, 1, true, c->rs.st);
            x_in = c->p.bx.Xn;
        }
        LP_HIP(ctx_gemv_dual(c, x_in, v.y, v.Ax, c->p.bt));
    } else {
        v.ax_chunks = 1;
        LP_HIP(ctx_gemv_n(c, 1, v.x, nullptr, nullptr, v.Ax, c->p.bt));
        LP_TRY(ctx_allreduce(c, v.Ax, c->p.m, 0));          // n-split: A.x = sum over ranks of A_g.x_g
        LP_HIP(ctx_gemv_t(c, 1, v.y, c->p.bt));
    }
    prof_mark(c, T_GEMV);
    // small LPs: the launch goes on with the next iteration's Dinv / r_hat set-up (enqueue_head then skips it)
    v.status_seq = (int)(++c->rs.seq_counter & 0x7fffffffu);
    if (c->p.tall || c->p.box) {                // kernel by kernel: slabs npa wide, A^T.y of a slack column is y (bounded: the bound block)
        if (c->p.box) box_residuals(v, c->p.bx, c->rs.st);
        else tall_residuals(v, c->p.tv, c->rs.st);
        vec_scalar_indicators(v, is_init, ip_next, tol, c->rs.st);
        c->pred_done = false;
        LP_HIP(hipGetLastError());
        return LPIPM_OK;
    }
    const bool with_pred = !c->colsplit && vec_fused(v);
    LP_TRY(vec_residuals(v, is_init, ip_next, tol, c->rs.st, c->colsplit ? &xr : nullptr, with_pred));
    c->pred_done = with_pred;
    LP_HIP(hipGetLastError());
    return LPIPM_OK;
}

// status records of all LPs of the context -> pinned host array (96 bytes each)
// The status records go straight from the kernels that write them into the context's coherent pinned array
// (VecArgs::status_pinned: payload, system fence, sequence word), and a solve that needs nothing else from the stream at
// that point waits for an iteration by watching the sequence words (wait_status): neither a D2H copy launch nor an event
// record sits between the indicators and the next iteration's A.D.A^T (C2: 4 + 6 us of ~310 per iteration).
// LPIPM_STATUS_COPY=1: copy launch + event as in rounds 1-2.
static void bind_status_pinned(lpipm_ctx* c, bool allow) {
    void* dp = nullptr;
    const char* e = lp_knob("LPIPM_STATUS_COPY");
    const bool on = allow && !(e && e[0] == '1') && c->rs.status_host && hipHostGetDevicePointer(&dp, c->rs.status_host, 0) == hipSuccess;
    (void)hipGetLastError();
    c->p.va.status_pinned = on ? (StatusRec*)dp : nullptr;
}
// Waits until the records of the LPs `idx[0 .. count)` carry the sequence number of the last residual
// launch.  Spins on the pinned records (bounded: ~10 s, then the stream is drained and the records are checked once more).
static int wait_status(lpipm_ctx* c, const int* idx, int count) {
    if (!c->rs.spin_status) { LP_HIP(hipEventSynchronize(c->rs.ev_status)); return LPIPM_OK; }
    const int32_t want = (int32_t)c->p.va.status_seq;
    auto arrived = [&]() {
        for (int k = 0; k < count; ++k) {
            const StatusRec* r = c->rs.status_host + idx[k];
            if (__atomic_load_n(&r->pad_, __ATOMIC_ACQUIRE) != want) return false;
        }
        return true;
    };
    const auto t0 = std::chrono::steady_clock::now();
    for (unsigned spins = 0;; ++spins) {
        if (arrived()) return LPIPM_OK;
        __builtin_ia32_pause();
        if ((spins & 0xffffu) == 0xffffu && std::chrono::steady_clock::now() - t0 > std::chrono::seconds(10)) break;
    }
    LP_HIP(hipStreamSynchronize(c->rs.st));
    if (arrived()) return LPIPM_OK;
    g_err_detail = "the status record of an iteration never reached the host";
    return LPIPM_ERR_HIP;
}
static int copy_status(lpipm_ctx* c) {
    if (!c->p.va.status_pinned)            // (else written by the kernels themselves)
        LP_HIP(member_bytes(c, c->rs.status_host, c->p.va.status, sizeof(StatusRec), hipMemcpyDeviceToHost));
    if (c->colsplit && c->p.sys[SYS_WORK].res.ngroups() > 0)   // a wait kernel that gave up (its producer never ran) says so here
        LP_HIP(hipMemcpyAsync(c->rs.timeout_host, c->p.sys[SYS_WORK].res.wait_timeout, sizeof(unsigned int), hipMemcpyDeviceToHost, c->rs.st));
    return LPIPM_OK;
}

// one IPM iteration: get_delta (feasible_point.rs:110-152), step length (mod.rs:216-221),
// do_step (:222), indicators (:225)
// Head of an iteration: Dinv = x/z and the normal equations M = A.Dinv.A^T (newton_equations.rs:54-57).  It needs
// nothing from the host, and its kernels test the LP's done word, so it may be enqueued BEFORE the host has read
// the status of the previous iteration: the GPU goes straight from one iteration into the big kernel of the
// next instead of idling through the read-back, and if the LP turns out to be finished the two kernels return
// at once.
// n-split: M = sum over the ranks of A_g D_g A_g^T, behind the launch that built this rank's term; a refining context's M0 is
// then the summed matrix.
// grouped (the launch went in column-group-major order, armed with ev_c0): PIPELINED.  The workgroup that completes a
// group's last tile bumps the group's word; on the communication stream a one-wave kernel waits for that word, the
// group's tiles are packed, summed over the ranks (the caller's all-reduce) and unpacked -- while the launch goes on with the
// next groups.  After the last tile only the last group's sum is left (C5: 1/32 .. 1/8 of the 1.08 GB that round 2 reduced in
// one block after the launch).  Element-wise sums: the same values as one reduction of the whole triangle -- bit for bit with two
// ranks; with three or more only if the caller's all-reduce sums an element's terms in an order that does not depend on where
// the element sits in the buffer (a ring all-reduce such as gloo's does not: last-bit differences between the two ways).
// Otherwise: the packed lower triangle in one block on the solver's stream.
static int reduce_system(lpipm_ctx* c, bool grouped) {
    hipStream_t st = c->rs.st;
    NormalSystem& work = c->p.sys[SYS_WORK];
    const Batch& bt = c->p.bt_head;
    if (grouped) {
        hipStream_t sc = c->st_c;
        LP_HIP(hipStreamWaitEvent(sc, c->ev_c0, 0));
        for (int g = 0; g < work.res.ngroups(); ++g) {
            const AdatGroup grp = adat_group(work.res, g);
            double* slice = c->mpack + (size_t)grp.first * TILE * TILE;
            LP_HIP(launch_wait_count(grp.word, (unsigned)grp.ntiles, bt.done, work.res.wait_timeout, sc));
            vec_pack_tiles(work.M, work.n, grp.tiles, grp.ntiles, slice, 0, sc);
            LP_TRY(ctx_allreduce(c, slice, (uint64_t)grp.ntiles * TILE * TILE, 0, sc));
            vec_pack_tiles(work.M, work.n, grp.tiles, grp.ntiles, slice, 1, sc);
        }
        LP_HIP(hipEventRecord(c->ev_c1, sc));
        LP_HIP(hipStreamWaitEvent(st, c->ev_c1, 0));
    } else {
        vec_pack_lower(work.M, work.n, work.n, c->mpack, 0, st);
        LP_TRY(ctx_allreduce(c, c->mpack, c->mpack_count, 0));
        vec_pack_lower(work.M, work.n, work.n, c->mpack, 1, st);
    }
    if (c->refine > 0) vec_copy_lower(work.M, c->p.M0, work.n, work.n, st, bt);   // the summed matrix, for the refined solves
    return LPIPM_OK;
}
static int enqueue_head(lpipm_ctx* c, const Iter& it) {
    hipStream_t st = c->rs.st;
    NormalSystem& work = c->p.sys[SYS_WORK];
    VecArgs vh = c->p.va;
    vh.done_chk = c->p.bt_head.done;
    prof_mark(c, T_VEC);
    if (c->pred_done) c->pred_done = false;       // the residual launch in front of this head has done it (enqueue_residuals)
    else vec_pred_setup(vh, st);
    if (c->p.tall) {     // W_s, E_x and t of the predictor's two right-hand sides (c, b), (r1, r_P); then K instead of M
        tall_setup(vh, c->p.tv, true, 2, vh.c, vh.b, vh.r1, vh.rP, st);
        prof_mark(c, T_VEC, true);
        LP_HIP(build_system(c, work, c->p.bt_head));
        prof_mark(c, T_ADAT, true);
        return LPIPM_OK;
    }
    // bounded: D~ and the ratios from the x / z of k_pred_setup, W of the predictor's two right-hand sides; then M~ with D~
    if (c->p.box) box_setup(vh, c->p.bx, true, 2, vh.c, vh.b, vh.r1, vh.rP, st);
    prof_mark(c, T_VEC, true);
    if (it.skip_factor) return LPIPM_OK;          // iteration 1 on a kept factor: its M is already there, factored
    const bool split = c->colsplit && c->world > 1;
    const bool grouped = split && work.res.ngroups() > 0 && c->st_c;    // (the launch then arms ev_c0 once the group words are zero)
    LP_HIP(build_system(c, cur_sys(c, it), c->p.bt_head, BuildOpts{.M2 = c->p.M0, .signal_groups = grouped}));   // newton_equations.rs:55-57
    if (split) LP_TRY(reduce_system(c, grouped));
    prof_mark(c, T_ADAT, true);
    return LPIPM_OK;
}

// The look-ahead of launch_potrf, if the side stream it needs was created (lpipm_create).
static const PotrfLookahead* lookahead(lpipm_ctx* c) { return c->la.side ? &c->la : nullptr; }

// What the predictor does beside the factorisation's chain, on the look-ahead's side stream (PotrfBeside): its pass A.W needs
// W of k_pred_setup only, and forward step k of its solve needs that right-hand side, the inverse of super-block k and block
// columns of L that are final by then.  R, Y and tpart belong to the solves alone; nothing of the factorisation touches them.
struct PredictorBeside {
    lpipm_ctx* c;
    const Iter& it;
    const lpipm_opts* o;
    int fwd_done = -1;           // the pass is enqueued (>= 0), and the forward steps [0, fwd_done) of the predictor's solve
    int rc = LPIPM_OK;           // what the pass or a step returned (at() itself answers the factorisation in its terms)
    static hipError_t at(void* self, int sb, hipStream_t side) {
        PredictorBeside* b = (PredictorBeside*)self;
        lpipm_ctx* c = b->c;
        b->fwd_done = sb + 1;
        b->rc = sb < 0 ? pass_aw(c, 2, c->p.va.b, c->p.va.rP, side)     // :220
                       : normal_solve(c, b->it, b->o, 2, SolveSteps{sb, sb + 1, false}, side);
        return b->rc == LPIPM_OK ? hipSuccess : hipErrorUnknown;
    }
};

// The factor of this iteration's system.  Dense: the kept first factor as it is (its pivot failure, if it had one, to the solver's
// word); else M's Cholesky factor (:129-131; a single LP: `pb` beside its chain if launch_potrf finds that the look-ahead applies)
// or its QR factorisation (:133-149), the pivot word of a first system kept with the factor it belongs to.  Tall: K's Cholesky
// factor, then with equality rows Zt, S and S's factor; a tall LP has no kept factor, no refinement and no QR arm, so nothing of
// `it` or of the solver type applies to it, here or in sym_solve.
static int factor_system(lpipm_ctx* c, const Iter& it, const lpipm_opts* o, PredictorBeside& pb) {
    VecArgs& v = c->p.va;
    hipStream_t st = c->rs.st;
    const Batch& bt = c->p.bt;
    // (no clearing of the pivot-failure word: k_blind_start and every k_scalar_indicators leave it zero)
    if (c->p.tall) {
        LP_HIP(launch_potrf(*c->p.sys[SYS_WORK].factor, v.potrf_info, st, bt, lookahead(c), false, nullptr));
        if (c->p.tall_eq) LP_TRY(tall_eq_schur(c));
    } else if (it.skip_factor) {
        LP_HIP(copy_info(c, v.potrf_info, c->p.sys[SYS_FIRST].info));
        return LPIPM_OK;
    } else {
        const NormalSystem& sys = cur_sys(c, it);     // (the QR arms keep no first factor: the working system)
        if (o->solver_type == LPIPM_SOLVER_CHOLESKY) {
            PotrfBeside beside{PredictorBeside::at, &pb};
            const bool may_beside = !c->colsplit && bt.count == 1 && c->refine <= 0 && !c->p.box;
            const hipError_t e = launch_potrf(*sys.factor, v.potrf_info, st, bt, lookahead(c), false, may_beside ? &beside : nullptr);
            LP_TRY(pb.rc);
            LP_HIP(e);
        } else LP_HIP(launch_qr_factor(sys.M, sys.n, sys.n, c->p.tau, v.potrf_info, st));
        if (it.on_first) LP_HIP(copy_info(c, c->p.sys[SYS_FIRST].info, v.potrf_info));
    }
    prof_mark(c, T_POTRF);
    return LPIPM_OK;
}

// sym_solve (newton_equations.rs:214-225) for `count` right-hand sides (r1a, r2a), (r1b, r2b) with the factor of factor_system, up
// to where the epilogue forms p, q, u, v.  Dense: R = A.W + r2 (W is set up, so only r2 is read), R <- M^-1.R, the slabs of A^T.R;
// beside_done >= 0: the pass and the forward steps [0, beside_done) of the solve ran beside the factorisation (PredictorBeside).
// Tall: the reduced solve, whose t the set-up kernel has left in T, up to u_x in G, u_s in Us and v_e in Ve.
struct SymRhs { int count; const double *r1a, *r2a, *r1b = nullptr, *r2b = nullptr; };
static int sym_solve(lpipm_ctx* c, const Iter& it, const lpipm_opts* o, const SymRhs& rhs, int beside_done = -1) {
    const VecArgs& v = c->p.va;
    hipStream_t st = c->rs.st;
    const Batch& bt = c->p.bt;
    const int nrhs = rhs.count;
    if (c->p.tall) {
        const TallArgs& t = c->p.tv;
        LP_HIP(ctx_gemv_t(c, nrhs, t.T, bt));                                         // X^T.t
        prof_mark(c, T_GEMV);
        tall_fold_rhs(v, t, nrhs, rhs.r1a, rhs.r1b, st);                              // g = X^T.t - r1_x
        LP_HIP(hipGetLastError());
        prof_mark(c, T_VEC);
        if (c->p.tall_eq) LP_TRY(tall_eq_reduced_solve(c, nrhs, rhs.r2a, rhs.r2b));  // u_x through the Schur complement, v_e
        else LP_HIP(launch_chol_solve(*c->p.sys[SYS_WORK].factor, nrhs, t.G, c->p.Y, st, bt));   // u_x = K^-1 g
        prof_mark(c, T_TRSV);
        ++c->gemv_passes;                                                             // u_s = r2 - X.u_x   (tall_eq: over the `ub` rows)
        LP_HIP(launch_gemv_n(c->p.A, c->p.npa, c->p.tall_eq ? t.ms : (int)c->p.m, c->p.npa, nrhs, t.G, t.nxp, rhs.r2a, rhs.r2b, t.Us, c->p.mp, st, -1.0, bt, c->p.shared_a));
        prof_mark(c, T_GEMV);
        return LPIPM_OK;
    }
    if (beside_done < 0) LP_TRY(pass_aw(c, nrhs, rhs.r2a, rhs.r2b));                  // :220
    prof_mark(c, T_GEMV);
    LP_TRY(normal_solve(c, it, o, nrhs, SolveSteps{beside_done < 0 ? 0 : beside_done, -1, true}));   // :221
    prof_mark(c, T_TRSV);
    LP_HIP(ctx_gemv_t(c, nrhs, c->p.solR, bt));                                       // :223
    prof_mark(c, T_GEMV);
    return LPIPM_OK;
}

// The vector stage behind a sym_solve.  Predictor: (p, q), (u, v) and their dots (:223, delta.rs:29-32,38), Delta (delta.rs:33-37,
// feasible_point.rs:134-136) and the corrector's right-hand side (rhat.rs:37-75; tall: with its t).  Corrector: (u, v), Delta and
// the step length (mod.rs:216-221), the step (feasible_point.rs:76-106).  Small n on one rank: each in one fused launch.
enum class Phase { Predictor, Corrector };
static int epilogue(lpipm_ctx* c, Phase phase, int ip, double alpha0) {
    VecArgs& v = c->p.va;
    const TallArgs& t = c->p.tv;
    hipStream_t st = c->rs.st;
    const bool corr = phase == Phase::Corrector;
    XRank xr_{xrank_fn, c};
    const XRank* xr = c->colsplit ? &xr_ : nullptr;
    if (!c->p.tall && !c->p.box && !xr && vec_fused(v)) {
        if (corr) vec_fused_corrector(v, ip, alpha0, st); else vec_fused_predictor(v, ip, st);
    } else {
        if (c->p.tall) { if (corr) tall_uv_corr(v, t, v.r1, st); else tall_pq_uv(v, t, v.c, v.r1, st); }
        else if (c->p.box) { if (corr) box_uv_corr(v, c->p.bx, v.r1, v.rP2, st); else box_pq_uv(v, c->p.bx, v.c, v.b, v.r1, v.rP, st); }
        else LP_TRY(corr ? vec_uv_corr(v, st, xr) : vec_pq_uv(v, st, xr));
        LP_TRY(vec_delta(v, corr ? 1 : 0, ip, corr ? alpha0 : 1.0, st, xr));
        if (corr) vec_step(v, ip, alpha0, st); else vec_corr_setup(v, ip, st);
        if (c->p.tall && !corr) tall_setup(v, t, false, 1, v.r1, v.rP2, nullptr, nullptr, st);
        if (c->p.box && !corr) box_setup(v, c->p.bx, false, 1, v.r1, v.rP2, nullptr, nullptr, st);
    }
    prof_mark(c, T_VEC);
    return LPIPM_OK;
}

// The residuals and indicators at the new point (mod.rs:225), the status record on its way to the host, ev_status behind it.
static int finish_iteration(lpipm_ctx* c, double tol) {
    LP_TRY(enqueue_residuals(c, 0, 0, tol));
    LP_TRY(copy_status(c));
    prof_mark(c, T_VEC);
    if (!c->rs.spin_status) LP_HIP(hipEventRecord(c->rs.ev_status, c->rs.st));
    return LPIPM_OK;
}

// The rest of the iteration, one sequence for every form, ending with the status record on its way to the host.
static int enqueue_tail(lpipm_ctx* c, const Iter& it, int ip, const lpipm_opts* o) {
    const VecArgs& v = c->p.va;
    PredictorBeside pb{c, it, o};
    LP_TRY(factor_system(c, it, o, pb));
    LP_TRY(sym_solve(c, it, o, SymRhs{2, v.c, v.b, v.r1, v.rP}, pb.fwd_done));   // both calls of solve_newton_equations (:187-188)
    LP_TRY(epilogue(c, Phase::Predictor, ip, o->alpha0));
    LP_TRY(sym_solve(c, it, o, SymRhs{1, v.r1, v.rP2}));                         // corrector: only the second call changes
    LP_TRY(epilogue(c, Phase::Corrector, ip, o->alpha0));
    return finish_iteration(c, o->tol);
}

static int enqueue_iteration(lpipm_ctx* c, const Iter& it, int ip, const lpipm_opts* o) {
    LP_TRY(enqueue_head(c, it));
    return enqueue_tail(c, it, ip, o);
}

// The one kept first factor of a shared-matrix batch (Problem::shared_factor): M1 = A.A^T (+ I on the structural slack rows)
// by ONE A.D.A^T launch for a batch of one member with dinv = the vector of ones, then its factorisation with the merges of
// the inverses, on the serial schedule every member of a batch goes through.  Formed once it equals what each member would
// have formed (the library is deterministic and a member's bits do not depend on its place in a batch).  Run by the parent
// context on its own stream, ahead of the first Cholesky-arm solve after an upload and before any half-batch view is
// dispatched, so two host threads never race to build it; the flag is up only when the build has completed.  The launch uses
// member 0's slabs and counters (through a copy of the A.D.A^T resources: the context's own dirty mark covers every member).
static int ensure_shared_factor(lpipm_ctx* c, const lpipm_opts* o) {
    if (!c || !o || !c->p.has_problem || !c->p.shared_factor || c->first_valid) return LPIPM_OK;
    if (o->solver_type != LPIPM_SOLVER_CHOLESKY || !c->first_cache || c->colsplit || c->refine > 0) return LPIPM_OK;
    if (c->is_view) { g_err_detail = "a half-batch view found the shared first factor unbuilt"; return LPIPM_ERR_HIP; }
    LP_HIP(hipSetDevice(c->device));
    hipStream_t st = c->rs.st;
    const Batch one{1, (long long)c->p.bstride, nullptr, 0};
    const NormalSystem& first = c->p.sys[SYS_FIRST];
    const bool timed = c->profiling != 0;
    hipEvent_t ev[3] = {nullptr, nullptr, nullptr};
    auto drop_events = [&]() { for (hipEvent_t e : ev) if (e) (void)hipEventDestroy(e); };
    if (timed)
        for (hipEvent_t& e : ev)
            if (hipEventCreate(&e) != hipSuccess) { (void)hipGetLastError(); drop_events(); g_err_detail = "failed to create events"; return LPIPM_ERR_HIP; }
    auto enqueue = [&]() -> int {
        if (timed) LP_HIP(hipEventRecord(ev[0], st));
        NormalSystem build = c->p.sys[SYS_WORK];            // the working system's launch with a private dirty mark, into M1
        build.M = first.M; build.res.counters_dirty = true;
        LP_HIP(build_system(c, build, one, BuildOpts{.dinv = c->p.ones}));   // (+ I on the slack rows; nothing refines here)
        if (timed) LP_HIP(hipEventRecord(ev[1], st));
        LP_HIP(launch_potrf(*first.factor, first.info, st, one, nullptr, true, nullptr));
        if (timed) LP_HIP(hipEventRecord(ev[2], st));
        LP_HIP(hipStreamSynchronize(st));
        return LPIPM_OK;
    };
    const int rc = enqueue();
    if (rc == LPIPM_OK && timed) {
        float a_ms = 0.f, p_ms = 0.f;
        (void)hipEventElapsedTime(&a_ms, ev[0], ev[1]);
        (void)hipEventElapsedTime(&p_ms, ev[1], ev[2]);
        c->build_adat_ms = a_ms; c->build_potrf_ms = p_ms;
    }
    drop_events();
    LP_TRY(rc);
    c->build_launches = 1;
    c->first_valid = true;
    return LPIPM_OK;
}

static void print_row(double alpha, const StatusRec& s) {  // mod.rs:228 + indicators.rs:25-33
    printf("%.8f\t%.8f\t%.8f\t%.8f\t%.8f\t%8.3f\n", alpha, s.rho_p, s.rho_d, s.rho_g, s.rho_mu, s.obj);
}

// Where the solutions go: per-member host pointers, or rows of one device buffer.
struct XOut { double* const* host = nullptr; char* dev = nullptr; size_t stride_bytes = 0; };
// What an entry was given for them, and the one place that checks it: exactly one of host rows and device block is there,
// and a row of the block holds the row_len(i) doubles of each of the `count` members.
struct XArgs { double* const* host_rows = nullptr; void* dev = nullptr; uint64_t row_stride = 0; };
template <typename RowLen = uint64_t (*)(uint64_t)>
static int xout_of(const XArgs& a, XOut& xo, uint64_t count = 0, RowLen row_len = nullptr) {
    if ((a.host_rows != nullptr) == (a.dev != nullptr)) return LPIPM_ERR_BAD_ARGUMENT;
    for (uint64_t i = 0; i < count && a.dev; ++i)
        if (row_len(i) > a.row_stride) return LPIPM_ERR_BAD_ARGUMENT;
    xo = XOut{a.host_rows, (char*)a.dev, a.row_stride * sizeof(double)};
    return LPIPM_OK;
}

// The return code a status record stands for, -1 while the LP goes on iterating.
static int status_code(const StatusRec& s) {
    // EquationSolverType::build failure (newton_equations.rs:58-63) and the NaN check on p, q
    // (:190-194) both surface as NumericalProblem from get_delta (mod.rs:215)
    if (s.potrf_info != 0 || (s.flags & FLAG_NAN_PQ)) return LPIPM_NUMERICAL_PROBLEM;
    if (s.status == ST_OPTIMAL) return LPIPM_OK;               // mod.rs:231
    if (s.status == ST_INFEASIBLE) return LPIPM_INFEASIBLE;    // :232
    if (s.status == ST_UNBOUNDED) return LPIPM_UNBOUNDED;      // :233
    return -1;
}
static bool has_x(int code) { return code == LPIPM_OK || code == LPIPM_ITERATION_LIMIT; }

// The members' return codes, objectives and iteration counts (fun, its nullable); set() is the only code that writes them.
// A member that was refused, or whose chunk failed as a whole, has no objective and no iterations: the defaults.
struct Results {
    double* fun = nullptr; uint64_t* its = nullptr; int32_t* status = nullptr;
    void set(uint64_t i, int code, double fun_i = NAN, uint64_t its_i = 0) const { status[i] = code; if (fun) fun[i] = fun_i; if (its) its[i] = its_i; }
};
// Everything a solve hands back, indexed by the member's place k in the resident batch (a half-batch view's member i is
// k = bt.first + i): its results go to res[k], its solution to row rows[k] of x (row k when rows is null); log: the one LP's.
struct SolveOut { XOut x; const uint64_t* rows = nullptr; Results res; lpipm_iter_row* log = nullptr; };

// What differs between the one LP of lpipm_solve[_device] (any solver arm, column split, `disp` table, iteration log) and a
// lockstep batch: made once at the top of solve_members.
enum class Members { One, Lockstep };
struct SolveMode {
    bool batch;        // the checks of a batch apply, and the closing x launch covers every member whatever its outcome
    bool wait_start;   // the host waits for the starting point before it enqueues iteration 1
    bool spin;         // it waits for an iteration by watching the pinned records (wait_status), not on the status event
    bool rows;         // the starting point's record is fetched, and the `disp` table and the iteration log are written from the records
    bool bounce_x;     // x reaches a host row through the pinned bounce buffer: truly asynchronous, one synchronisation for x and status
};

// x / tau (mod.rs:231/238, :165) of the members that have a solution (ret[i]), each to its destination: a row of the device
// block, a host row, or -- the one LP -- the pinned bounce buffer, *bounced then being the host row that buffer is copied to
// once the stream has drained.  In front: one launch that forms x for every LP of a batch (none for a single LP without a
// solution) and, for a scaled problem, the one that takes it back to the caller's units.
static int copy_out_x(lpipm_ctx* c, const SolveMode& md, const std::vector<int>& ret, const SolveOut& out, double** bounced) {
    *bounced = nullptr;
    if (!md.batch && !has_x(ret[0])) return LPIPM_OK;
    StreamRes& rs = c->rs;
    hipStream_t st = rs.st;
    const XOut& xo = out.x;
    XRank xrf{xrank_fn, c};
    LP_TRY(vec_final_x(c->p.va, c->p.xout, st, c->colsplit ? &xrf : nullptr));
    LP_HIP(hipGetLastError());
    if (c->p.scale_passes > 0)          // (fun is the scaled vectors' product: the same number)
        LP_HIP(launch_unscale_x(c->p.sc, c->p.xout, (int)c->p.n, st, Batch{c->p.B, (long long)c->p.bstride, nullptr, c->p.bt.first}));
    if (c->p.box && c->p.bx.gen) {      // general bounds: the structural values in the caller's variables (fun already is: c0 holds c.t)
        box_caller_units(c->p.va, c->p.bx, c->p.xout, BOX_OUT_X, st);
        LP_HIP(hipGetLastError());
    }
    const size_t xbytes = c->p.n * sizeof(double);
    for (int i = 0; i < c->p.B; ++i) {
        if (!has_x(ret[(size_t)i])) continue;
        const uint64_t k = (uint64_t)(c->p.bt.first + i), row = out.rows ? out.rows[k] : k;
        const char* src = (const char*)c->p.xout + (size_t)k * c->p.bstride;
        if (xo.dev) LP_HIP(hipMemcpyAsync(xo.dev + row * xo.stride_bytes, src, xbytes, hipMemcpyDeviceToDevice, st));
        else if (!xo.host[row]) continue;
        else if (!md.bounce_x) LP_HIP(hipMemcpyAsync(xo.host[row], src, xbytes, hipMemcpyDeviceToHost, st));
        else {
            if (rs.x_pinned_cap < c->p.n) {
                if (rs.x_pinned) (void)hipHostFree(rs.x_pinned);
                rs.x_pinned = nullptr; rs.x_pinned_cap = 0;
                LP_HIP(hipHostMalloc((void**)&rs.x_pinned, xbytes));
                rs.x_pinned_cap = c->p.n;
            }
            LP_HIP(hipMemcpyAsync(rs.x_pinned, src, xbytes, hipMemcpyDeviceToHost, st));
            *bounced = xo.host[row];
        }
    }
    return copy_status(c);
}

// lpipm_phase_times of the solve that has just drained (a phase's time is that of the launch, which covers all members), with
// what building the shared first factor ahead of it took, if it was built.  replay: iteration 1 started from a kept factor.
static void report_times(lpipm_ctx* c, uint64_t loop_iterations, bool replay) {
    if (c->profiling) {
        float ms = 0.f;
        (void)hipEventElapsedTime(&ms, c->rs.ev_begin, c->rs.ev_end);
        c->times.total_ms = ms;
        c->times.adat_ms = c->tag_ms[T_ADAT] + c->build_adat_ms; c->times.potrf_ms = c->tag_ms[T_POTRF] + c->build_potrf_ms;
        c->times.trsv_ms = c->tag_ms[T_TRSV]; c->times.gemv_ms = c->tag_ms[T_GEMV]; c->times.vec_ms = c->tag_ms[T_VEC];
        // launches of the kernel (each covers all B members): iteration 1 on a kept factor made none
        c->times.adat_launches = loop_iterations - (replay && loop_iterations > 0 ? 1 : 0) + c->build_launches;
        c->times.iterations = loop_iterations;         // iterations of the loop (= the slowest member's count)
        // the speculatively enqueued head of the iteration after the last holds no GEMV pass: every counted pass ran
        c->times.gemv_passes = c->gemv_passes;
    }
    c->build_adat_ms = c->build_potrf_ms = 0.0; c->build_launches = 0;    // reported (or not asked for)
}

// The interior-point loop (solve_normal_form, mod.rs:199-240) for the B >= 1 LPs that c -- a context or a half-batch view --
// covers; member i's return code, objective (NAN without a solution) and iteration count go to out.res, its solution to its
// row of out.x.  One loop for both kinds of members; SolveMode has what differs.
// Members::Lockstep: B LPs of one shape resident at once (upload_impl with count = B), every launch of the iteration covering
// all of them (gridDim.z = B).  The ~100 dependent launches per iteration -- the latency floor of a small LP -- are then paid
// once per B LPs.  LPs finish at different iterations: k_scalar_indicators sets an LP's `done` word on the conditions that end
// the reference's loop (mod.rs:215, :231-233) and every later kernel skips it, so its iterate stays what it was; the host
// mirrors the same decisions from the status records to count iterations and pick the return codes.
static int solve_members(lpipm_ctx* c, const lpipm_opts* o, Members members, const SolveOut& out) {
    if (!c || !o) return LPIPM_ERR_BAD_ARGUMENT;
    if (!c->is_view) invalidate_duals(c);                 // up again when this solve returns Ok (a view's parent: solve_lockstep)
    const bool batch = members == Members::Lockstep;
    // wait_start.  A single LP: the host needs the starting point's indicators only for the `disp` table, for the selective
    // refinement's first decision and for the phase marks: otherwise the first iteration is enqueued without a round trip to
    // the host (~25 us per solve; profiling 2 brackets A.D.A^T only: no mark yet).  A batch: nothing of the starting point is
    // read by the host; it waits there whenever it profiles.
    // spin.  Only a loop that speculates on records the kernels write themselves can.  A single LP with every phase bracketed
    // -- profiling 1 -- : the last mark of an iteration is recorded BEHIND the indicators kernel and has to have completed when it
    // is read: the event wait stays; profiling 2's two marks sit in front of it.  A batch keeps it in both profiling modes.
    const SolveMode md{.batch = batch, .wait_start = batch ? c->profiling != 0 : (o->disp || c->refine == 1 || c->profiling == 1),
                       .spin = !c->colsplit && c->p.va.status_pinned != nullptr && (batch ? !c->profiling : c->profiling != 1),
                       .rows = !batch, .bounce_x = !batch};
    if (!(o->alpha0 > 0.0) || !(o->alpha0 < 1.0) || !(o->tol > 0.0)) return LPIPM_INVALID_PARAMETER;   // InteriorPointBuilder::build, mod.rs:118-128
    if (md.batch) {
        if (o->solver_type != LPIPM_SOLVER_CHOLESKY) return LPIPM_ERR_UNSUPPORTED;      // the QR arms are single-LP
        if (!c->p.has_problem) return LPIPM_ERR_NO_PROBLEM;
        if (c->colsplit) return LPIPM_ERR_UNSUPPORTED;
    } else {
        if (o->solver_type < 0 || o->solver_type > 2) return LPIPM_INVALID_PARAMETER;
        if (!c->p.has_problem) return LPIPM_ERR_NO_PROBLEM;
        if (c->p.B != 1) return LPIPM_ERR_BAD_ARGUMENT;   // a lockstep batch is solved by solve_lockstep
        if (o->solver_type != LPIPM_SOLVER_CHOLESKY && c->p.mp > 16384) return LPIPM_ERR_UNSUPPORTED;  // QR solve keeps the rhs in LDS
        if (o->solver_type != LPIPM_SOLVER_CHOLESKY && (c->p.tall || c->p.box)) return LPIPM_ERR_UNSUPPORTED;   // the reduced forms: Cholesky arm only
    }
    LP_HIP(hipSetDevice(c->device));
    LP_TRY(ensure_shared_factor(c, o));                   // (a view finds it built: solve_lockstep)
    const int B = c->p.B;
    VecArgs& v = c->p.va;
    StreamRes& rs = c->rs;
    hipStream_t st = rs.st;
    for (int t = 0; t < T_NTAGS; ++t) c->tag_ms[t] = 0.0;   // profiling (lpipm_set_profiling)
    c->times = lpipm_phase_times{}; rs.nmarks = 0; c->gemv_passes = 0;
    uint64_t loop_iterations = 0;
    if (c->profiling) LP_HIP(hipEventRecord(rs.ev_begin, st));

    vec_blind_start(v, st);                               // feasible_point.rs:24-31
    LP_TRY(tall_eq_reset(c));
    LP_TRY(box_reset(c));
    prof_mark(c, T_VEC);
    LP_TRY(enqueue_residuals(c, 1, o->ip ? 1 : 0, o->tol));  // feasible_point.rs:32, mod.rs:206
    if (md.rows) LP_TRY(copy_status(c));
    prof_mark(c, T_VEC);
    if (md.wait_start) {
        LP_HIP(hipStreamSynchronize(st));
        prof_collect(c);
    }
    if (md.rows && o->disp) {                             // mod.rs:208-211
        printf("alpha     \trho_p     \trho_d     \trho_g     \trho_mu    \tobj       \n");
        print_row(1.0, *rs.status_host);
    }
    // (selective mode: at the starting point mu / mu_0 = 1, so no member of a batch refines its first iteration)
    bool refine_now = c->refine == 2 || (md.rows && c->refine == 1 && rs.status_host->rho_mu <= refine_below());
    // the head of iteration k+1 goes out before the status of iteration k is read (see enqueue_head); not when the
    // iteration contains host-side collectives
    const bool speculate = !c->colsplit;
    rs.spin_status = md.spin;
    std::vector<int> ret((size_t)B, -1), act((size_t)B);        // -1: still iterating; act[0 .. running): those members, ascending
    std::vector<uint64_t> its((size_t)B, 0);
    for (int i = 0; i < B; ++i) act[(size_t)i] = i;
    int running = B, ip = o->ip ? 1 : 0;
    bool head_out = false;
    // The kept first factor (lpipm_ctx::first_valid): the Cholesky arm of a resident problem whose layout has the buffers.
    // Iteration 1 works in them; when they are valid it neither forms nor factors its matrix.  The flag is down from here
    // until iteration 1 has completed, so a solve that fails before that leaves nothing that counts as kept.
    // A shared-matrix batch's one factor is complete before any solve reads it (ensure_shared_factor) and no solve writes it:
    // every member of every solve replays it, the first solve included, and its flag stays up.
    const bool use_first = o->solver_type == LPIPM_SOLVER_CHOLESKY && c->first_cache && c->p.keep && !c->colsplit && c->refine <= 0;
    const bool replay = use_first && c->first_valid;
    if (use_first && c->p.shared_factor && !replay) { g_err_detail = "the shared first factor is not built"; return LPIPM_ERR_HIP; }
    c->first_done = false;
    if (use_first && !c->p.shared_factor) c->first_valid = false;
    const Iter ahead{};          // the head that is enqueued ahead of its iteration: never iteration 1's, and a head refines nothing
    for (uint64_t iteration = 1; iteration <= o->max_iter && running > 0; ++iteration) {   // mod.rs:213
        const bool on_first = use_first && iteration == 1;
        const Iter it{.on_first = on_first, .skip_factor = on_first && replay, .refine_now = refine_now};
        if (!speculate) {
            LP_TRY(enqueue_iteration(c, it, ip, o));
            LP_HIP(hipStreamSynchronize(st));
            prof_collect(c);
        } else {
            if (!head_out) LP_TRY(enqueue_head(c, it));
            LP_TRY(enqueue_tail(c, it, ip, o));
            const size_t marks = rs.nmarks;
            head_out = iteration < o->max_iter;
            if (head_out) LP_TRY(enqueue_head(c, ahead));  // next iteration's A.D.A^T, before this one's status is read
            // the members that were still running when this iteration was enqueued write a record; the others are skipped
            LP_TRY(wait_status(c, act.data(), running));
            prof_collect(c, marks);
        }
        ++loop_iterations;
        if (iteration == 1) { c->first_done = true; if (use_first) c->first_valid = true; }
        if (c->colsplit && c->p.sys[SYS_WORK].res.ngroups() > 0 && *rs.timeout_host != 0) {
            g_err_detail = "a column group of A.D.A^T did not complete within the wait kernel's bound";
            LP_HIP(hipStreamSynchronize(st));
            return LPIPM_ERR_HIP;
        }
        ip = 0;                                                    // mod.rs:223
        // the refinement launches of the next iteration are enqueued if ANY running member asks for them; which members
        // they touch is each member's own device word (k_scalar_indicators), the same decision as when it is solved alone
        bool any_refines = false;
        int still = 0;
        for (int k = 0; k < running; ++k) {
            const int i = act[(size_t)k];
            const StatusRec s = rs.status_host[i];
            const int code = status_code(s);
            if (md.rows && code != LPIPM_NUMERICAL_PROBLEM) {      // (get_delta fails before the row of its iteration exists)
                if (o->disp) print_row(s.alpha, s);
                if (out.log) {
                    lpipm_iter_row& r = out.log[iteration - 1];
                    r.alpha = s.alpha; r.rho_p = s.rho_p; r.rho_d = s.rho_d; r.rho_A = s.rho_A;
                    r.rho_g = s.rho_g; r.rho_mu = s.rho_mu; r.obj = s.obj;
                }
            }
            if (code >= 0) { ret[(size_t)i] = code; its[(size_t)i] = iteration; continue; }
            act[(size_t)still++] = i;
            any_refines = any_refines || (c->refine == 1 && s.rho_mu <= refine_below());
        }
        running = still;
        refine_now = c->refine == 2 || any_refines;
    }
    for (int i = 0; i < B; ++i)
        if (ret[(size_t)i] < 0) { ret[(size_t)i] = LPIPM_ITERATION_LIMIT; its[(size_t)i] = o->max_iter; }   // mod.rs:237-239
    double* bounced = nullptr;
    LP_TRY(copy_out_x(c, md, ret, out, &bounced));
    if (c->profiling) LP_HIP(hipEventRecord(rs.ev_end, st));
    LP_HIP(hipStreamSynchronize(st));
    if (bounced) std::memcpy(bounced, rs.x_pinned, c->p.n * sizeof(double));
    report_times(c, loop_iterations, replay);
    lpipm_ctx* rec = c->is_view ? c->parent : c;          // the return codes lpipm_get_duals goes by
    if (!c->is_view) { c->last_ret.assign((size_t)B, LPIPM_ERR_NO_PROBLEM); c->duals_valid = true; }
    for (int i = 0; i < B && rec; ++i) rec->last_ret[(size_t)(c->p.bt.first + i)] = ret[(size_t)i];
    for (int i = 0; i < B; ++i)
        out.res.set((uint64_t)(c->p.bt.first + i), ret[(size_t)i], has_x(ret[(size_t)i]) ? rs.status_host[i].obj : NAN, its[(size_t)i]);
    return LPIPM_OK;
}

// One LP: the return code is the LP's own, and *fun stays untouched when it has no solution.
struct SingleOut { double* x_host = nullptr; void* x_dev = nullptr; double* fun = nullptr; uint64_t* its = nullptr; lpipm_iter_row* log = nullptr; };
static int solve_single(lpipm_ctx* c, const lpipm_opts* o, const SingleOut& s) {
    double fun = NAN;
    uint64_t its = 0;
    int32_t code = LPIPM_OK;
    LP_TRY(solve_members(c, o, Members::One, SolveOut{.x = XOut{.host = &s.x_host, .dev = (char*)s.x_dev},
                                                      .res = Results{&fun, &its, &code}, .log = s.log}));
    if (s.fun && has_x(code)) *s.fun = fun;
    if (s.its) *s.its = its;
    return code;
}
extern "C" int lpipm_solve(lpipm_ctx* c, const lpipm_opts* o, double* x_slack_out, double* fun_out,
                           uint64_t* iterations_out, lpipm_iter_row* log) {
    if (!x_slack_out) return LPIPM_ERR_BAD_ARGUMENT;
    return solve_single(c, o, {.x_host = x_slack_out, .fun = fun_out, .its = iterations_out, .log = log});
}
extern "C" int lpipm_solve_device(lpipm_ctx* c, const lpipm_opts* o, void* x_dev_out, double* fun_out,
                                  uint64_t* iterations_out, lpipm_iter_row* log) {
    return solve_single(c, o, {.x_dev = x_dev_out, .fun = fun_out, .its = iterations_out, .log = log});
}

// ------------------------------------------------------------------------------------------------
// ---- half-batch views -------------------------------------------------------------------------------------------------
static void destroy_views(lpipm_ctx* c) {
    for (lpipm_ctx* v : c->halves) {
        (void)hipSetDevice(v->device);
        stream_res_destroy(v->rs);         // all that a view owns
        delete v;
    }
    c->halves.clear();
}
// A view of the LPs [first, first + count) of c's resident batch: a copy of the problem (the same device state: every pointer
// stays LP 0's; its systems carry their plans), and its own stream, events and pinned status records.
static lpipm_ctx* make_view(const lpipm_ctx* c, int first, int count) {
    lpipm_ctx* v = new lpipm_ctx();
    if (stream_res_create(v->rs, (size_t)count) != LPIPM_OK) { delete v; return nullptr; }
    v->is_view = true;
    v->device = c->device; v->num_cu = c->num_cu; v->refine = c->refine;
    v->p = c->p;
    for (NormalSystem& s : v->p.sys) s.res.counters_dirty = true;     // whatever the parent's state: this view's stream has not launched yet
    v->p.B = count;
    v->p.bt = Batch{count, (long long)c->p.bstride, c->p.va.done, first};
    v->p.bt_head = v->p.bt;
    v->p.va.bcount = count; v->p.va.bfirst = first; v->p.va.done_chk = c->p.va.done;
    bind_status_pinned(v, c->p.va.status_pinned != nullptr);
    return v;
}

// A batch of at least 16 members is solved as TWO half-batches, each by its own host thread on its own stream (views of the
// context): the halves drift out of phase, and one half's A.D.A^T (MFMA-bound, fills the chip) runs beside the other half's
// factorisation chain, solves and passes over A (latency- and HBM-bound).  Every member goes through exactly the kernels
// and arguments of the one-stream path: the results are bit-identical (tests/test_gpu_c4_members.py).  Measured on the C4
// shard (32 x 1024x2048): +3 .. +6.5 % (profiles/r03_rejected_experiments.txt has the variants).  Not while profiling (the
// phase marks are per stream) and not for the views themselves.
static int solve_lockstep(lpipm_ctx* c, const lpipm_opts* o, const SolveOut& out) {
    if (!c || !o || !out.res.status) return LPIPM_ERR_BAD_ARGUMENT;      // (out.x is xout_of's: one destination is there)
    if (!c->is_view) invalidate_duals(c);
    if (c->is_view || !c->halves_env || c->profiling || c->p.B < 16 || !c->p.has_problem || c->colsplit)
        return solve_members(c, o, Members::Lockstep, out);
    LP_HIP(hipSetDevice(c->device));
    if (c->halves.empty()) {
        const int h = c->p.B / 2;
        lpipm_ctx* a = make_view(c, 0, h);
        lpipm_ctx* b = a ? make_view(c, h, c->p.B - h) : nullptr;
        if (!a || !b) {
            if (a) { c->halves.push_back(a); destroy_views(c); }
            return solve_members(c, o, Members::Lockstep, out);
        }
        a->parent = b->parent = c;
        c->halves.push_back(a); c->halves.push_back(b);
    }
    c->last_ret.assign((size_t)c->p.B, LPIPM_ERR_NO_PROBLEM);
    LP_TRY(ensure_shared_factor(c, o));             // one factor for the batch: built here, once, before both halves
    c->build_adat_ms = c->build_potrf_ms = 0.0; c->build_launches = 0;   // (nothing is profiled on this path)
    LP_HIP(hipStreamSynchronize(c->rs.st));         // the upload (or whatever else the caller enqueued) precedes both halves
    // the kept first factor: the halves work with the parent's switch and validity, and it is valid afterwards only if both
    // got through their iteration 1 and returned Ok (a shared-matrix batch's one factor is only read: it stays valid)
    const bool use_first = c->first_cache && c->p.keep && !c->p.shared_factor;
    for (lpipm_ctx* v : c->halves) { v->first_cache = c->first_cache; v->first_valid = c->first_valid; }
    if (use_first) c->first_valid = false;
    int rc[2] = {LPIPM_OK, LPIPM_OK};
    auto run = [&](int k) { rc[k] = solve_members(c->halves[(size_t)k], o, Members::Lockstep, out); };
    std::thread other(run, 1);
    run(0);
    other.join();
    if (use_first && rc[0] == LPIPM_OK && rc[1] == LPIPM_OK && c->halves[0]->first_done && c->halves[1]->first_done) c->first_valid = true;
    c->duals_valid = rc[0] == LPIPM_OK && rc[1] == LPIPM_OK;
    return rc[0] != LPIPM_OK ? rc[0] : rc[1];
}

extern "C" int lpipm_get_resident_bytes(const lpipm_ctx* c, uint64_t* bytes_out) {
    if (!c || !bytes_out) return LPIPM_ERR_BAD_ARGUMENT;
    size_t lists = 0;
    for (const NormalSystem& s : c->p.sys) lists += s.res.list_bytes;
    *bytes_out = c->p.has_problem ? (uint64_t)(c->p.arena_bytes + c->p.a_shared_bytes + lists + c->p.scale_bytes) : 0;
    return LPIPM_OK;
}
extern "C" int lpipm_solve_lockstep(lpipm_ctx* c, const lpipm_opts* o, double* const* x_slack_out, double* fun_out,
                                    uint64_t* iterations_out, int32_t* status_out) {
    XOut xo;
    LP_TRY(xout_of({.host_rows = x_slack_out}, xo));
    return solve_lockstep(c, o, SolveOut{.x = xo, .res = Results{fun_out, iterations_out, status_out}});
}
extern "C" int lpipm_solve_lockstep_device(lpipm_ctx* c, const lpipm_opts* o, void* x_dev_out, uint64_t row_stride,
                                           double* fun_out, uint64_t* iterations_out, int32_t* status_out) {
    // (a row's length is the resident problem's: this entry looks at its context before its destination, the others after)
    if (!c) return LPIPM_ERR_BAD_ARGUMENT;
    XOut xo;
    LP_TRY(xout_of({.dev = x_dev_out, .row_stride = row_stride}, xo, 1, [&](uint64_t) { return c->p.n; }));
    return solve_lockstep(c, o, SolveOut{.x = xo, .res = Results{fun_out, iterations_out, status_out}});
}

// A shard of independent LPs on one device: what the four lpipm_solve_batch* entries ask of batch_impl.  Dense members: A[i] is
// m[i] x n[i] in slack form (lda = n[i]), with member i's structural hint n_slack[i] (lpipm_upload_slack; nullable = all 0).
// Tall members (lpipm_solve_batch_ub_tall): pure-`ub` LPs in the tall inequality form -- A[i] is m[i] x n[i] with lda = n[i],
// b[i] has m[i] entries, c[i] the n[i] structural costs, x n[i] + m[i] entries; no hint.
struct BatchRequest {
    bool tall = false;                   // the members' form
    uint64_t count = 0;
    const uint64_t *m = nullptr, *n = nullptr, *n_slack = nullptr;
    const double *const *A = nullptr, *const *b = nullptr, *const *c = nullptr;
    const double* c0 = nullptr;          // nullable: all zero
    // _slack and _ub_tall, which take either destination of x, refuse a call without one before anything else; the other two
    // entries let a call of no members and no destination through to batch_impl's own checks (nothing to do: Ok)
    bool x_always = false;
    bool has_lens() const { return n && (!tall || m); }
    uint64_t row_len(uint64_t i) const { return n[i] + (tall ? m[i] : 0); }     // doubles of member i's x
};

// Bytes member i of a batch request would occupy in a lockstep batch of 32 of its shape: the real layout (a measuring pass
// of layout_problem over its geometry), not a formula that drifts from it.  No kept first factor: a chunk is uploaded, solved
// once and replaced.  n_slack: the member's verified hint -- its slack columns are not resident (a tall member's never are).
static size_t lockstep_bytes_per_lp(const lpipm_ctx* c, const BatchRequest& q, uint64_t i, uint64_t n_slack) {
    const uint64_t m = q.m[i], n = q.row_len(i);
    const Geometry g = geometry_of(Upload{.count = 32, .m = m, .n = n, .tall = q.tall, .keep_ok = false}, q.tall ? m : n_slack, c->first_cache, c->refine);
    Problem t;
    set_geometry(t, g);
    plan_builds(t, c);
    FactorPlan plans[SYS_COUNT];
    Arena measure;
    if (layout_problem(t, plans, c->refine, measure, false, nullptr) != LPIPM_OK) return (size_t)-1;
    return (size_t)round_up(measure.off, 4096);
}

// The upload of the members idx[k0 .. k0 + g) -- one shape, one verified hint ns -- with the arrays its request points into:
// a lockstep chunk, or (g == 1) a member solved alone.  Tall: a chunk is a batch whose members own their matrices, a member
// alone the tall LP of lpipm_upload_ub_tall itself (a batch of one would not be the same resident problem).
struct MemberUpload {
    std::vector<const double*> A, b, c;
    std::vector<double> c0;
    Upload u;
    MemberUpload() = default;
    MemberUpload(MemberUpload&&) = default;      // u points into the vectors' storage, which moves with them: moved, never copied
};
static MemberUpload member_upload(const BatchRequest& q, const std::vector<uint64_t>& idx, size_t k0, size_t g, uint64_t ns) {
    MemberUpload r;
    r.A.resize(g); r.b.resize(g); r.c.resize(g); r.c0.assign(g, 0.0);
    for (size_t k = 0; k < g; ++k) {
        const uint64_t j = idx[k0 + k];
        r.A[k] = q.A[j]; r.b[k] = q.b[j]; r.c[k] = q.c[j];
        if (q.c0) r.c0[k] = q.c0[j];
    }
    const uint64_t m = q.m[idx[k0]], n = q.n[idx[k0]];
    if (!q.tall) r.u = Upload{.count = g, .m = m, .n = n, .n_slack = ns, .A = r.A.data(), .lda = n, .b = r.b.data(), .c = r.c.data(),
                                .c0 = r.c0.data(), .hint_verified = true, .keep_ok = false};
    else if (g > 1) r.u = owned_tall_request(g, n, m, r.A.data(), n, r.b.data(), r.c.data(), r.c0.data());
    else            r.u = tall_request(n, m, r.A[0], n, r.b[0], r.c.data(), r.c0.data());
    return r;
}

// At least `count` worker contexts beside c: each with its own stream and buffers, kept until lpipm_destroy.
static int ensure_workers(lpipm_ctx* c, size_t count) {
    while (c->workers.size() < count) {
        lpipm_ctx* w = nullptr;
        LP_TRY(lpipm_create(c->device, &w));
        c->workers.push_back(w);
    }
    return LPIPM_OK;
}
// One group's chunks (split_chunks) as lockstep batches, through a pipeline over two contexts: while chunk k is being solved on
// one, a helper thread uploads chunk k+1 into the other (host staging + copy engine vs. compute: the PCIe time of a large batch
// hides behind the solves).  A chunk refused as a whole (Unconstrained, ...) gives every member that code; a runtime failure ends the call.
static int solve_chunks(lpipm_ctx* c, const BatchRequest& q, const std::vector<uint64_t>& grp, uint64_t ns, const std::vector<Span>& spans,
                        const lpipm_opts* o, const XOut& xo, const Results& res) {
    std::vector<MemberUpload> ups;
    ups.reserve(spans.size());
    for (const Span& s : spans) ups.push_back(member_upload(q, grp, s.k0, s.g, ns));
    if (spans.size() > 1) LP_TRY(ensure_workers(c, 1));
    lpipm_ctx* pipe[2] = {c, spans.size() > 1 ? c->workers[0] : nullptr};
    auto upload = [&](size_t k) -> int {
        lpipm_ctx* w = pipe[k & 1];
        (void)hipSetDevice(w->device);
        w->scaling = c->scaling;
        return upload_impl(w, ups[k].u);
    };
    int rc_up = spans.empty() ? LPIPM_OK : upload(0);
    for (size_t k = 0; k < spans.size(); ++k) {
        const Span& s = spans[k];
        int rc_next = LPIPM_OK;
        std::thread up;
        if (k + 1 < spans.size()) up = std::thread([&, k] { rc_next = upload(k + 1); });
        std::vector<double> gfun(s.g, NAN);
        std::vector<uint64_t> gits(s.g, 0);
        std::vector<int32_t> gst(s.g, 0);
        int rc = rc_up;
        if (rc == LPIPM_OK)      // (member i of the chunk is member grp[k0 + i] of the call: that row of x)
            rc = solve_lockstep(pipe[k & 1], o, SolveOut{.x = xo, .rows = grp.data() + s.k0, .res = Results{gfun.data(), gits.data(), gst.data()}});
        if (up.joinable()) up.join();
        if (rc >= 100) return rc;
        for (size_t i = 0; i < s.g; ++i)
            rc == LPIPM_OK ? res.set(grp[s.k0 + i], gst[i], gfun[i], gits[i]) : res.set(grp[s.k0 + i], rc);
        rc_up = rc_next;
    }
    return LPIPM_OK;
}

// The members left over, one by one.  They are latency-bound (the factorisation's diagonal chain keeps 1 of 256 CUs busy), so
// `batch_concurrency` contexts -- each with its own stream and buffers, each driven by its own host thread -- solve different
// members at the same time, handed out through an atomic counter.  -> the first runtime failure (which ends the handing out) or Ok.
static int solve_rest(lpipm_ctx* c, const BatchRequest& q, const std::vector<uint64_t>& ns, const std::vector<uint64_t>& rest,
                      const lpipm_opts* o, const XOut& xo, const Results& res) {
    if (rest.empty()) return LPIPM_OK;
    int nworkers = c->batch_concurrency;
    if (nworkers == 0) {   // auto: latency-bound sizes gain ~3x from 4-8 members in flight (1024x2048: 165 -> 513 LP/s); others do not
        uint64_t mmax = 0;
        for (uint64_t i : rest) mmax = q.m[i] > mmax ? q.m[i] : mmax;
        nworkers = mmax <= 2048 ? 8 : 2;
    }
    if ((size_t)nworkers > rest.size()) nworkers = (int)rest.size();
    LP_TRY(ensure_workers(c, (size_t)nworkers - 1));
    std::atomic<uint64_t> next{0};
    std::atomic<int> fatal{LPIPM_OK};
    auto run = [&](lpipm_ctx* w) {
        (void)hipSetDevice(w->device);
        w->scaling = c->scaling;
        lpipm_opts opts = *o;
        opts.disp = 0;   // interleaved tables from concurrent members would be unreadable
        for (;;) {
            const uint64_t k = next.fetch_add(1);
            if (k >= rest.size() || fatal.load() != LPIPM_OK) break;
            const uint64_t i = rest[k];
            const MemberUpload up = member_upload(q, rest, k, 1, ns[i]);
            int rc = upload_impl(w, up.u);
            double fun = NAN;
            uint64_t it = 0;
            if (rc == LPIPM_OK && !xo.dev && !xo.host[i]) rc = LPIPM_ERR_BAD_ARGUMENT;      // as lpipm_solve: a host row is not optional
            if (rc == LPIPM_OK)
                rc = solve_single(w, &opts, {.x_host = xo.dev ? nullptr : xo.host[i],
                                             .x_dev = xo.dev ? xo.dev + i * xo.stride_bytes : nullptr, .fun = &fun, .its = &it});
            res.set(i, rc, fun, it);
            if (rc >= 100) { int expected = LPIPM_OK; fatal.compare_exchange_strong(expected, rc); }
        }
    };
    std::vector<std::thread> threads;
    for (int t = 1; t < nworkers; ++t) threads.emplace_back(run, c->workers[t - 1]);
    run(c);
    for (std::thread& t : threads) t.join();
    return fatal.load();
}

//  1. Every member's hint is verified (verify_hints); a member whose hint is out of range is refused and takes no further part.
//  2. Members of one shape and one hint that holds (>= 2 of them, Cholesky arm) are solved as lockstep batches, in chunks that
//     fit the memory budget: one launch per kernel for the whole chunk (group_members, chunk_size, split_chunks, solve_chunks).
//  3. The rest (odd shapes, a chunk's odd member, QR arms) go one by one through the worker pool (solve_rest).
// Every member's result depends only on its own inputs.  The planning of 1 and 2 touches no device (batch_plan.hpp).
static int batch_members(lpipm_ctx* c, const BatchRequest& q, const lpipm_opts* o, const XArgs& xa, const Results& res) {
    XOut xo;
    if (q.x_always || q.count || xa.host_rows || xa.dev)
        LP_TRY(xout_of(xa, xo, q.has_lens() ? q.count : 0, [&](uint64_t i) { return q.row_len(i); }));
    if (!c || !o || (q.count && (!q.m || !q.n || !q.A || !q.b || !q.c || !res.status))) return LPIPM_ERR_BAD_ARGUMENT;
    std::vector<char> taken(q.count, 0);             // refused, or in a lockstep group
    const std::vector<uint64_t> ns = verify_hints(q.count, q.m, q.n, q.n_slack, q.A, taken);
    for (uint64_t i = 0; i < q.count; ++i)
        if (taken[i]) res.set(i, LPIPM_ERR_BAD_ARGUMENT);
    std::vector<uint64_t> rest;                      // members left to the one-by-one path
    if (c->lockstep_max != 0 && o->solver_type == LPIPM_SOLVER_CHOLESKY) {
        LP_HIP(hipSetDevice(c->device));
        for (const std::vector<uint64_t>& grp : group_members(q.count, q.m, q.n, ns, taken)) {
            const uint64_t first = grp[0];
            // what fits in ~60 % of the free memory: two chunks are resident, one being solved, the next one being uploaded
            size_t free_b = 0, total_b = 0;
            LP_HIP(hipMemGetInfo(&free_b, &total_b));
            free_b += c->p.arena_bytes;                // the current arena is released before the next one is made
            const size_t fit = (size_t)(0.3 * (double)free_b / (double)lockstep_bytes_per_lp(c, q, first, ns[first]));
            const std::vector<Span> spans = split_chunks(grp, chunk_size(grp.size(), c->lockstep_max, fit), rest);
            LP_TRY(solve_chunks(c, q, grp, ns[first], spans, o, xo, res));
        }
    }
    for (uint64_t i = 0; i < q.count; ++i)
        if (!taken[i]) rest.push_back(i);
    return solve_rest(c, q, ns, rest, o, xo, res);
}
// The chunks and the members solved one at a time are uploaded and solved on c itself (and on its workers), and each of those
// solves leaves its own duals behind: whichever member c happened to solve last.  None of that is the caller's resident
// problem, so on every way out of the batch the getter finds nothing (lpipm_get_duals: LPIPM_ERR_NO_PROBLEM).
static int batch_impl(lpipm_ctx* c, const BatchRequest& q, const lpipm_opts* o, const XArgs& xa, const Results& res) {
    if (c) invalidate_duals(c);
    const int rc = batch_members(c, q, o, xa, res);
    if (c) invalidate_duals(c);
    return rc;
}

extern "C" int lpipm_solve_batch(lpipm_ctx* c, uint64_t count, const uint64_t* m, const uint64_t* n,
                                 const double* const* A, const double* const* b, const double* const* cc,
                                 const double* c0, const lpipm_opts* o, double* const* x_slack_out,
                                 double* fun_out, uint64_t* iterations_out, int32_t* status_out) {
    return batch_impl(c, BatchRequest{.count = count, .m = m, .n = n, .A = A, .b = b, .c = cc, .c0 = c0}, o,
                      XArgs{.host_rows = x_slack_out}, Results{fun_out, iterations_out, status_out});
}
extern "C" int lpipm_solve_batch_device(lpipm_ctx* c, uint64_t count, const uint64_t* m, const uint64_t* n,
                                        const double* const* A, const double* const* b, const double* const* cc,
                                        const double* c0, const lpipm_opts* o, void* x_dev_out, uint64_t row_stride,
                                        double* fun_out, uint64_t* iterations_out, int32_t* status_out) {
    return batch_impl(c, BatchRequest{.count = count, .m = m, .n = n, .A = A, .b = b, .c = cc, .c0 = c0}, o,
                      XArgs{.dev = x_dev_out, .row_stride = row_stride}, Results{fun_out, iterations_out, status_out});
}
extern "C" int lpipm_solve_batch_slack(lpipm_ctx* c, uint64_t count, const uint64_t* m, const uint64_t* n, const uint64_t* n_slack,
                                       const double* const* A, const double* const* b, const double* const* cc,
                                       const double* c0, const lpipm_opts* o, double* const* x_slack_out, void* x_dev_out,
                                       uint64_t row_stride, double* fun_out, uint64_t* iterations_out, int32_t* status_out) {
    return batch_impl(c, BatchRequest{.count = count, .m = m, .n = n, .n_slack = n_slack, .A = A, .b = b, .c = cc, .c0 = c0, .x_always = true}, o,
                      XArgs{.host_rows = x_slack_out, .dev = x_dev_out, .row_stride = row_stride}, Results{fun_out, iterations_out, status_out});
}
extern "C" int lpipm_solve_batch_ub_tall(lpipm_ctx* c, uint64_t count, const uint64_t* m_ub, const uint64_t* n,
                                         const double* const* A_ub, const double* const* b_ub, const double* const* cc,
                                         const double* c0, const lpipm_opts* o, double* const* x_slack_out, void* x_dev_out,
                                         uint64_t row_stride, double* fun_out, uint64_t* iterations_out, int32_t* status_out) {
    return batch_impl(c, BatchRequest{.tall = true, .count = count, .m = m_ub, .n = n, .A = A_ub, .b = b_ub, .c = cc, .c0 = c0,
                                      .x_always = true}, o,
                      XArgs{.host_rows = x_slack_out, .dev = x_dev_out, .row_stride = row_stride}, Results{fun_out, iterations_out, status_out});
}

extern "C" int lpipm_set_batch_lockstep(lpipm_ctx* c, int max_group) {
    if (!c || max_group < -1 || max_group > 4096) return LPIPM_ERR_BAD_ARGUMENT;
    c->lockstep_max = max_group;
    return LPIPM_OK;
}

extern "C" int lpipm_set_batch_concurrency(lpipm_ctx* c, int nworkers) {
    if (!c || nworkers < 0 || nworkers > 64) return LPIPM_ERR_BAD_ARGUMENT;
    c->batch_concurrency = nworkers;
    return LPIPM_OK;
}

extern "C" int lpipm_set_collective(lpipm_ctx* c, int rank, int world, lpipm_allreduce_fn fn, void* user) {
    if (!c || world < 1 || rank < 0 || rank >= world || (world > 1 && !fn)) return LPIPM_ERR_BAD_ARGUMENT;
    c->rank = rank; c->world = world; c->coll = fn; c->coll_user = user;
    return LPIPM_OK;
}

extern "C" int lpipm_set_collective_on_stream(lpipm_ctx* c, int on) {
    if (!c) return LPIPM_ERR_BAD_ARGUMENT;
    c->coll_on_stream = on != 0;
    return LPIPM_OK;
}

extern "C" int lpipm_upload_nsplit(lpipm_ctx* c, uint64_t m, uint64_t n_total, uint64_t n_local, const double* A_local,
                                   uint64_t lda, const double* b, const double* c_local, double c0) {
    if (!c || n_local == 0 || n_local > n_total) return LPIPM_ERR_BAD_ARGUMENT;
    if (c->scaling > 0) return LPIPM_ERR_UNSUPPORTED;      // row maxima of a column split would need the collective
    const int rc = upload_impl(c, Upload{.m = m, .n = n_local, .A = &A_local, .lda = lda, .b = &b, .c = &c_local, .c0 = &c0,
                                         .keep_ok = false, .colsplit = true});
    if (rc != LPIPM_OK) return rc;
    if (c->world > 1) {
        const size_t need = (size_t)c->p.mp * ((size_t)c->p.mp + 128) / 2;
        if (need != c->mpack_count) {
            if (c->mpack) { LP_HIP(hipFree(c->mpack)); c->mpack = nullptr; c->mpack_count = 0; }
            LP_HIP(hipMalloc((void**)&c->mpack, need * sizeof(double)));
            c->mpack_count = need;
        }
    }
    if (c->world > 1 && !c->st_c) {
        if (hipStreamCreateWithFlags(&c->st_c, hipStreamNonBlocking) != hipSuccess ||
            hipEventCreateWithFlags(&c->ev_c0, hipEventDisableTiming) != hipSuccess ||
            hipEventCreateWithFlags(&c->ev_c1, hipEventDisableTiming) != hipSuccess) {
            (void)hipGetLastError();
            if (c->st_c) (void)hipStreamDestroy(c->st_c);
            c->st_c = nullptr;                   // M is then reduced in one block after the launch
        }
    }
    c->colsplit = true;
    c->p.va.n_total = (long long)n_total;
    c->p.va.gs = c->p.gs;
    return LPIPM_OK;
}

extern "C" int lpipm_set_first_factor_cache(lpipm_ctx* c, int on) {
    if (!c) return LPIPM_ERR_BAD_ARGUMENT;
    c->first_cache = on != 0;     // the buffers come and go with the next upload (upload_impl); off stops their use at once
    return LPIPM_OK;
}

extern "C" int lpipm_set_scaling(lpipm_ctx* c, int passes) {
    if (!c || passes < 0 || passes > 64) return LPIPM_ERR_BAD_ARGUMENT;
    c->scaling = passes;          // the exponents come and go with the next upload (upload_impl)
    return LPIPM_OK;
}
extern "C" int lpipm_get_scaling(const lpipm_ctx* c, uint64_t member, int32_t* row_exp_out, int32_t* col_exp_out) {
    if (!c || !row_exp_out || !col_exp_out) return LPIPM_ERR_BAD_ARGUMENT;
    if (!c->p.has_problem) return LPIPM_ERR_NO_PROBLEM;
    if (member >= (uint64_t)c->p.B) return LPIPM_ERR_BAD_ARGUMENT;
    if (c->p.scale_passes <= 0) {
        std::memset(row_exp_out, 0, c->p.m * sizeof(int32_t));
        std::memset(col_exp_out, 0, c->p.n * sizeof(int32_t));
        return LPIPM_OK;
    }
    LP_HIP(hipSetDevice(c->device));
    const long long off = (long long)member * c->p.sc.estride;   // (one set for a shared-matrix batch: estride 0)
    LP_HIP(hipMemcpyAsync(row_exp_out, c->p.sc.kr + off, c->p.m * sizeof(int32_t), hipMemcpyDeviceToHost, c->rs.st));
    LP_HIP(hipMemcpyAsync(col_exp_out, c->p.sc.kc + off, c->p.n * sizeof(int32_t), hipMemcpyDeviceToHost, c->rs.st));
    LP_HIP(hipStreamSynchronize(c->rs.st));
    return LPIPM_OK;
}

extern "C" int lpipm_update_vectors(lpipm_ctx* c, const double* b, const double* cc) {
    if (!c || !b || !cc) return LPIPM_ERR_BAD_ARGUMENT;
    if (!c->p.has_problem) return LPIPM_ERR_NO_PROBLEM;
    if (c->p.B != 1 || c->colsplit || c->p.from_parts) return LPIPM_ERR_UNSUPPORTED;
    LP_HIP(hipSetDevice(c->device));
    invalidate_duals(c);                      // b and c are new, the iterate is old
    // (the padding beyond m and n stays zero; A, and with it the kept first factor, is not touched)
    LP_HIP(hipMemcpyAsync((void*)c->p.va.b, b, c->p.m * sizeof(double), hipMemcpyHostToDevice, c->rs.st));
    LP_HIP(hipMemcpyAsync((void*)c->p.va.c, cc, c->p.n * sizeof(double), hipMemcpyHostToDevice, c->rs.st));
    if (c->p.scale_passes > 0)                // the kept exponents: A, and its kept factor, are the scaled ones
        LP_HIP(launch_scale_vectors(c->p.sc, (double*)c->p.va.b, (int)c->p.m, (double*)c->p.va.c, (int)c->p.n, c->rs.st, Batch{}));
    LP_HIP(hipStreamSynchronize(c->rs.st));   // the caller's arrays are free again from here
    return LPIPM_OK;
}

extern "C" int lpipm_update_vectors_device(lpipm_ctx* c, const void* b_dev, const void* c_dev) {
    if (!c || !b_dev || !c_dev) return LPIPM_ERR_BAD_ARGUMENT;
    if (!c->p.has_problem) return LPIPM_ERR_NO_PROBLEM;
    if (c->p.B != 1 || c->colsplit || c->p.from_parts) return LPIPM_ERR_UNSUPPORTED;
    LP_HIP(hipSetDevice(c->device));
    invalidate_duals(c);                      // b and c are new, the iterate is old
    const Dim db{c->p.m, 1}, dc{c->p.n, 1};
    LP_TRY(source_inside(c, b_dev, &db, 1, sizeof(double)));
    LP_TRY(source_inside(c, c_dev, &dc, 1, sizeof(double)));
    LP_HIP(hipMemcpyAsync((void*)c->p.va.b, b_dev, c->p.m * sizeof(double), hipMemcpyDeviceToDevice, c->rs.st));
    LP_HIP(hipMemcpyAsync((void*)c->p.va.c, c_dev, c->p.n * sizeof(double), hipMemcpyDeviceToDevice, c->rs.st));
    if (c->p.scale_passes > 0)
        LP_HIP(launch_scale_vectors(c->p.sc, (double*)c->p.va.b, (int)c->p.m, (double*)c->p.va.c, (int)c->p.n, c->rs.st, Batch{}));
    LP_HIP(hipStreamSynchronize(c->rs.st));   // the caller's blocks are free again from here
    return LPIPM_OK;
}

// At least `count` doubles in the context's pinned staging block and in its device image.
static int stage_grow(lpipm_ctx* c, size_t count) {
    if (count <= c->stage_cap) return LPIPM_OK;
    LP_HIP(hipStreamSynchronize(c->rs.st));
    if (c->stage_host) { (void)hipHostFree(c->stage_host); c->stage_host = nullptr; }
    if (c->stage_dev) { (void)hipFree(c->stage_dev); c->stage_dev = nullptr; }
    c->stage_cap = 0;
    LP_HIP(hipHostMalloc((void**)&c->stage_host, count * sizeof(double)));
    LP_HIP(hipMalloc((void**)&c->stage_dev, count * sizeof(double)));
    c->stage_cap = count;
    return LPIPM_OK;
}
// New b / c / c0 for every member of the resident batch.  host: per-member arrays, staged (with c0) in the pinned block,
// sent with one copy and distributed from its device image; otherwise b_dev / c_dev are the caller's packed device blocks and
// only c0 is staged.  One scatter launch either way.  A, the layout, the views and whatever factor is kept stay as they are.
static int update_lockstep_impl(lpipm_ctx* c, uint64_t count, const double* const* b, const double* const* cc, bool host,
                                const double* b_dev, uint64_t ldb, const double* c_dev, uint64_t ldc, const double* c0) {
    if (!c) return LPIPM_ERR_BAD_ARGUMENT;
    if (!c->p.has_problem) return LPIPM_ERR_NO_PROBLEM;
    if (c->colsplit || (c->p.from_parts && !c->p.shared_a && !c->p.owned_tall)) return LPIPM_ERR_UNSUPPORTED;
    const bool has_b = host ? b != nullptr : b_dev != nullptr, has_c = host ? cc != nullptr : c_dev != nullptr;
    if ((!has_b && !has_c) || count != (uint64_t)c->p.B) return LPIPM_ERR_BAD_ARGUMENT;
    const size_t B = (size_t)c->p.B, m = (size_t)c->p.m;
    const size_t nc = c->p.from_parts ? (size_t)c->p.nx : (size_t)c->p.n;      // parts: c = [c; 0], the slack costs stay 0
    if (host) {
        for (size_t i = 0; i < B; ++i)
            if ((has_b && !b[i]) || (has_c && !cc[i])) return LPIPM_ERR_BAD_ARGUMENT;
    } else if ((has_b && ldb < m) || (has_c && ldc < nc)) return LPIPM_ERR_BAD_ARGUMENT;
    LP_HIP(hipSetDevice(c->device));
    invalidate_duals(c);                      // b and c are new, the iterate is old
    hipStream_t st = c->rs.st;
    // the staged block: [b rows | c rows | c0], each part only if it is sent from the host
    const size_t nb_st = host && has_b ? B * m : 0, nc_st = host && has_c ? B * nc : 0, n0_st = c0 ? B : 0;
    const size_t total = nb_st + nc_st + n0_st;
    if (total) {
        LP_TRY(stage_grow(c, total));
        double* h = c->stage_host;
        for (size_t i = 0; i < B && nb_st; ++i) std::memcpy(h + i * m, b[i], m * sizeof(double));
        for (size_t i = 0; i < B && nc_st; ++i) std::memcpy(h + nb_st + i * nc, cc[i], nc * sizeof(double));
        if (n0_st) std::memcpy(h + nb_st + nc_st, c0, B * sizeof(double));
        LP_HIP(hipMemcpyAsync(c->stage_dev, h, total * sizeof(double), hipMemcpyHostToDevice, st));
    }
    ScatterRows<double> w;
    if (has_b) { w.seg[0].dst = (double*)c->p.va.b; w.seg[0].src = host ? c->stage_dev : b_dev; w.seg[0].ld = (long long)(host ? m : ldb); w.seg[0].len = (int)m; }
    if (has_c) { w.seg[1].dst = (double*)c->p.va.c; w.seg[1].src = host ? c->stage_dev + nb_st : c_dev; w.seg[1].ld = (long long)(host ? nc : ldc); w.seg[1].len = (int)nc; }
    if (c0)    { w.seg[2].dst = c->p.va.S + S_C0; w.seg[2].src = c->stage_dev + nb_st + nc_st; w.seg[2].ld = 1; w.seg[2].len = 1; }
    vec_scatter_rows(w, st, Batch{c->p.B, (long long)c->p.bstride, nullptr, 0});
    LP_HIP(hipGetLastError());
    if (c->p.scale_passes > 0)                // only what was just replaced, with the kept exponents
        LP_HIP(launch_scale_vectors(c->p.sc, has_b ? (double*)c->p.va.b : nullptr, (int)m, has_c ? (double*)c->p.va.c : nullptr, (int)nc,
                                    st, Batch{c->p.B, (long long)c->p.bstride, nullptr, 0}));
    LP_HIP(hipStreamSynchronize(st));   // the staging block (and with it the caller's arrays) is free again from here
    return LPIPM_OK;
}
extern "C" int lpipm_update_lockstep_vectors(lpipm_ctx* c, uint64_t count, const double* const* b, const double* const* cc,
                                             const double* c0) {
    return update_lockstep_impl(c, count, b, cc, true, nullptr, 0, nullptr, 0, c0);
}
extern "C" int lpipm_update_lockstep_vectors_device(lpipm_ctx* c, uint64_t count, const void* b_dev, uint64_t ldb,
                                                    const void* c_dev, uint64_t ldc, const double* c0) {
    return update_lockstep_impl(c, count, nullptr, nullptr, false, (const double*)b_dev, ldb, (const double*)c_dev, ldc, c0);
}

// ---- duals of the last solve (lpipm_get_duals, lpipm_get_duals_device) ---------------------------------------------------
// What both entries check first, in this order: the context, a resident problem, no column split, a completed solve whose
// iterate still means something (lpipm_ctx::duals_valid).
static int duals_ready(const lpipm_ctx* c) {
    if (!c) return LPIPM_ERR_BAD_ARGUMENT;
    if (!c->p.has_problem) return LPIPM_ERR_NO_PROBLEM;
    if (c->colsplit) return LPIPM_ERR_UNSUPPORTED;
    if (!c->duals_valid || c->last_ret.size() != (size_t)c->p.B) return LPIPM_ERR_NO_PROBLEM;
    return LPIPM_OK;
}
// One launch of k_final_duals + its scalar kernel over the whole resident batch, delivering the members [row0, row0 + rows)
// whose last status has a solution.  Device destinations (y_dev, z_dev; member k's rows at k - row0) are written directly;
// host ones (want_y / want_z with null device pointers) go through the context's staging block, which also carries the mask
// in and the {dual_fun, tau, kappa} triples out.  On return *ys / *zs / *infos point at the staged rows (m, n and 3 doubles each).
struct DualsRun { const double *ys = nullptr, *zs = nullptr, *infos = nullptr; };
static int run_duals(lpipm_ctx* c, size_t row0, size_t rows, bool want_y, bool want_z, double* y_dev, uint64_t ldy, double* z_dev,
                     uint64_t ldz, DualsRun& out) {
    const Problem& p = c->p;
    const size_t B = (size_t)p.B, m = (size_t)p.m, n = (size_t)p.n;
    const bool stage_y = want_y && !y_dev, stage_z = want_z && !z_dev;
    const size_t nmask = (B + 1) / 2, ninfo = 3 * rows, ny = stage_y ? rows * m : 0, nz = stage_z ? rows * n : 0;
    LP_TRY(stage_grow(c, nmask + ninfo + ny + nz));
    hipStream_t st = c->rs.st;
    int32_t* mask = (int32_t*)c->stage_host;
    bool any = false;
    for (size_t k = 0; k < B; ++k) {
        mask[k] = k >= row0 && k < row0 + rows && has_x(c->last_ret[k]) ? 1 : 0;
        any = any || mask[k] != 0;
    }
    out.infos = c->stage_host + nmask; out.ys = out.infos + ninfo; out.zs = out.ys + ny;
    if (!any) return LPIPM_OK;
    LP_HIP(hipMemcpyAsync(c->stage_dev, c->stage_host, nmask * sizeof(double), hipMemcpyHostToDevice, st));
    double* dev = c->stage_dev + nmask;
    DualsOut d{};
    d.info = dev; d.row0 = (long long)row0; d.mask = (const int32_t*)c->stage_dev;
    d.y = stage_y ? dev + ninfo : y_dev; d.ldy = (long long)(stage_y ? m : ldy);
    d.z = stage_z ? dev + ninfo + ny : z_dev; d.ldz = (long long)(stage_z ? n : ldz);
    if (p.scale_passes > 0) { d.kr = p.sc.kr; d.kc = p.sc.kc; d.estride = p.sc.estride; }
    vec_final_duals(p.va, d, st);
    if (p.box && p.bx.gen && d.z) box_caller_units(p.va, p.bx, d.z, BOX_OUT_Z, st);     // z_j = sigma_j z'_j (one LP: row 0)
    LP_HIP(hipGetLastError());
    LP_HIP(hipMemcpyAsync(c->stage_host + nmask, dev, (ninfo + ny + nz) * sizeof(double), hipMemcpyDeviceToHost, st));
    LP_HIP(hipStreamSynchronize(st));
    return LPIPM_OK;
}
static lpipm_dual_info dual_info_of(const double* triple, int32_t status) {
    return triple ? lpipm_dual_info{triple[0], triple[1], triple[2], status, 0} : lpipm_dual_info{NAN, NAN, NAN, status, 0};
}
extern "C" int lpipm_get_duals(lpipm_ctx* c, uint64_t member, double* y_out, double* z_out, lpipm_dual_info* info_out) {
    LP_TRY(duals_ready(c));
    if (member >= (uint64_t)c->p.B) return LPIPM_ERR_BAD_ARGUMENT;
    const int32_t code = c->last_ret[(size_t)member];
    if (!has_x(code)) return code;                   // the member's own outcome; nothing is written
    LP_HIP(hipSetDevice(c->device));
    DualsRun r;
    LP_TRY(run_duals(c, (size_t)member, 1, y_out != nullptr, z_out != nullptr, nullptr, 0, nullptr, 0, r));
    if (y_out) std::memcpy(y_out, r.ys, c->p.m * sizeof(double));
    if (z_out) std::memcpy(z_out, r.zs, c->p.n * sizeof(double));
    if (info_out) *info_out = dual_info_of(r.infos, code);
    return LPIPM_OK;
}
extern "C" int lpipm_get_duals_device(lpipm_ctx* c, void* y_dev, uint64_t ldy, void* z_dev, uint64_t ldz, lpipm_dual_info* info_out) {
    LP_TRY(duals_ready(c));
    const uint64_t B = (uint64_t)c->p.B;
    if ((y_dev && ldy < c->p.m) || (z_dev && ldz < c->p.n)) return LPIPM_ERR_BAD_ARGUMENT;
    LP_HIP(hipSetDevice(c->device));
    // nothing is launched before both destinations are known to be device memory that holds every member's row
    const Dim dy[2] = {{B, (int64_t)ldy}, {c->p.m, 1}}, dz[2] = {{B, (int64_t)ldz}, {c->p.n, 1}};
    if (y_dev) LP_TRY(source_inside(c, y_dev, dy, 2, sizeof(double)));
    if (z_dev) LP_TRY(source_inside(c, z_dev, dz, 2, sizeof(double)));
    DualsRun r;
    LP_TRY(run_duals(c, 0, (size_t)B, false, false, (double*)y_dev, ldy, (double*)z_dev, ldz, r));
    for (uint64_t k = 0; k < B && info_out; ++k) {
        const int32_t code = c->last_ret[(size_t)k];
        info_out[k] = dual_info_of(has_x(code) ? r.infos + 3 * k : nullptr, code);
    }
    return LPIPM_OK;
}

// ---- certificates of the last solve (lpipm_get_certificate, lpipm_get_certificate_device) -------------------------------
// The launches of vec_cert_rays, one pass over the resident image and vec_cert_residual over the whole resident batch,
// delivering the members [row0, row0 + rows).  Destinations as in run_duals: device rows written directly, host ones through
// the staging block, which carries the mask in and the info records out.  The pass is the residual pair's (ctx_gemv_dual:
// A^T.y^ and A.x^ in one read of the image, the structural slack block, shared images, the tall forms' X and the `eq` rows),
// with a Batch that has no done word: every member is done by now.
struct CertRun { const double *ys = nullptr, *cols = nullptr, *infos = nullptr; };
static int run_certificates(lpipm_ctx* c, size_t row0, size_t rows, bool want_y, bool want_col, double* y_dev, uint64_t ldy,
                            double* col_dev, uint64_t ldc, CertRun& out) {
    Problem& p = c->p;
    const size_t B = (size_t)p.B, m = (size_t)p.m, n = (size_t)p.n;
    const bool stage_y = want_y && !y_dev, stage_c = want_col && !col_dev;
    const size_t nmask = (B + 1) / 2, ninfo = (size_t)CERT_INFO_DOUBLES * rows, ny = stage_y ? rows * m : 0, nc = stage_c ? rows * n : 0;
    LP_TRY(stage_grow(c, nmask + ninfo + ny + nc));
    hipStream_t st = c->rs.st;
    int32_t* mask = (int32_t*)c->stage_host;
    bool any = false;
    for (size_t k = 0; k < B; ++k) {
        const int32_t code = c->last_ret[k];
        mask[k] = k < row0 || k >= row0 + rows ? CERT_ASK_NOT
                : code == LPIPM_INFEASIBLE ? CERT_ASK_INFEASIBLE : code == LPIPM_UNBOUNDED ? CERT_ASK_UNBOUNDED : CERT_ASK_PLAIN;
        any = any || mask[k] >= CERT_ASK_INFEASIBLE;
    }
    out.infos = c->stage_host + nmask; out.ys = out.infos + ninfo; out.cols = out.ys + ny;
    LP_HIP(hipMemcpyAsync(c->stage_dev, c->stage_host, nmask * sizeof(double), hipMemcpyHostToDevice, st));
    double* dev = c->stage_dev + nmask;
    CertOut d{};
    d.info = dev; d.row0 = (long long)row0; d.mask = (const int32_t*)c->stage_dev;
    d.y = stage_y ? dev + ninfo : y_dev; d.ldy = (long long)(stage_y ? m : ldy);
    d.col = stage_c ? dev + ninfo + ny : col_dev; d.ldc = (long long)(stage_c ? n : ldc);
    if (p.scale_passes > 0) { d.kr = p.sc.kr; d.kc = p.sc.kc; d.estride = p.sc.estride; }
    d.nxs = p.tall ? p.tv.nx : (int)n; d.slab = p.tall ? p.npa : p.np;
    VecArgs v = p.va;                      // (a copy: the solves' own block keeps its ax_chunks)
    if (any) {
        vec_cert_rays(v, d, st);
        LP_HIP(hipGetLastError());
        v.ax_chunks = gemv_dual_chunks(p.npa);
        const uint64_t passes = c->gemv_passes;
        const double* x_in = v.W;
        if (p.box && p.bx.nf > 0) {        // free columns: the pass reads the net ray
            box_net(v, p.bx, v.W, 0, p.bx.Xn, 0, 1, false, st);
            x_in = p.bx.Xn;
        }
        LP_HIP(ctx_gemv_dual(c, x_in, v.dy, v.Ax, Batch{p.bt.count, p.bt.stride, nullptr, p.bt.first}));
        c->gemv_passes = passes;           // (lpipm_phase_times counts a solve's passes)
        if (p.box) {     // the bound block: A_ext^T.y^ into u, A_ext.x^ into q, both whole, which the residual then reads as one slab each
            box_products(v, p.bx, BoxProducts{v.W, v.Ax, v.ax_chunks, v.q, v.dy, p.ATpart, (long long)p.np, v.u}, st);
            LP_HIP(hipGetLastError());
            v.ATpart = v.u; v.nsplit = 1; d.nxs = (int)n; d.slab = v.np;
            v.Ax = v.q; v.ax_chunks = 1;
        }
    }
    vec_cert_residual(v, d, st);           // (without a certificate to form: its scalar launch alone has work)
    // general bounds: z^ or the improving ray in the caller's orientation (sigma applied, the free halves netted; one LP: row 0)
    if (any && p.box && p.bx.gen && d.col) box_caller_units(v, p.bx, d.col, BOX_OUT_CERT, st);
    LP_HIP(hipGetLastError());
    LP_HIP(hipMemcpyAsync(c->stage_host + nmask, dev, (ninfo + ny + nc) * sizeof(double), hipMemcpyDeviceToHost, st));
    LP_HIP(hipStreamSynchronize(st));
    return LPIPM_OK;
}
static lpipm_cert_info cert_info_of(const double* rec, int32_t status) {
    return lpipm_cert_info{rec[0], rec[1], rec[2], rec[3], (int32_t)rec[4], status};
}
extern "C" int lpipm_get_certificate(lpipm_ctx* c, uint64_t member, double* y_out, double* col_out, lpipm_cert_info* info_out) {
    LP_TRY(duals_ready(c));
    if (member >= (uint64_t)c->p.B || !info_out) return LPIPM_ERR_BAD_ARGUMENT;
    LP_HIP(hipSetDevice(c->device));
    CertRun r;
    LP_TRY(run_certificates(c, (size_t)member, 1, y_out != nullptr, col_out != nullptr, nullptr, 0, nullptr, 0, r));
    const lpipm_cert_info info = cert_info_of(r.infos, c->last_ret[(size_t)member]);
    if (y_out && info.kind == LPIPM_CERT_FARKAS) std::memcpy(y_out, r.ys, c->p.m * sizeof(double));
    if (col_out && info.kind != LPIPM_CERT_NONE) std::memcpy(col_out, r.cols, c->p.n * sizeof(double));
    *info_out = info;
    return LPIPM_OK;
}
extern "C" int lpipm_get_certificate_device(lpipm_ctx* c, void* y_dev, uint64_t ldy, void* col_dev, uint64_t ldc,
                                            lpipm_cert_info* info_out) {
    LP_TRY(duals_ready(c));
    const uint64_t B = (uint64_t)c->p.B;
    if (!info_out || (y_dev && ldy < c->p.m) || (col_dev && ldc < c->p.n)) return LPIPM_ERR_BAD_ARGUMENT;
    LP_HIP(hipSetDevice(c->device));
    // nothing is launched before both destinations are known to be device memory that holds every member's row
    const Dim dy[2] = {{B, (int64_t)ldy}, {c->p.m, 1}}, dc[2] = {{B, (int64_t)ldc}, {c->p.n, 1}};
    if (y_dev) LP_TRY(source_inside(c, y_dev, dy, 2, sizeof(double)));
    if (col_dev) LP_TRY(source_inside(c, col_dev, dc, 2, sizeof(double)));
    CertRun r;
    LP_TRY(run_certificates(c, 0, (size_t)B, false, false, (double*)y_dev, ldy, (double*)col_dev, ldc, r));
    for (uint64_t k = 0; k < B; ++k) info_out[k] = cert_info_of(r.infos + CERT_INFO_DOUBLES * k, c->last_ret[(size_t)k]);
    return LPIPM_OK;
}

extern "C" int lpipm_set_profiling(lpipm_ctx* c, int on) {
    if (!c) return LPIPM_ERR_BAD_ARGUMENT;
    c->profiling = on < 0 ? 0 : (on > 2 ? 1 : on);
    return LPIPM_OK;
}
extern "C" int lpipm_get_phase_times(const lpipm_ctx* c, lpipm_phase_times* out) {
    if (!c || !out) return LPIPM_ERR_BAD_ARGUMENT;
    *out = c->times;
    return LPIPM_OK;
}

// ------------------------------------------------------------------------------------------------
// kernel-granularity entry points (parity tests / micro-benchmarks)
// The two timers.  Every ms_out of the entries comes from one of them; nothing else records ev_begin / ev_end.
// 1. A bracket per repeat: `prepare` (untimed: what a repeat needs put back first), ev_begin, `body`, ev_end, a drain of the
//    stream; *ms_out is the mean over the repeats.  lpipm_k_adat, lpipm_k_gemv_*, lpipm_k_mfma_f64_probe (no prepare),
//    lpipm_k_potrf (prepare restores the matrix the factorisation overwrote), lpipm_k_chol_solve (prepare reloads the
//    right-hand sides the solve overwrote) and lpipm_k_qr_solve (one repeat): each launch sequence alone on an idle device.
static int no_prepare() { return LPIPM_OK; }
template <typename F, typename P = int (*)()>
static int timed_repeats(lpipm_ctx* c, int repeats, double* ms_out, F&& body, P prepare = no_prepare) {
    if (repeats < 1) repeats = 1;
    float total = 0.f;
    for (int r = 0; r < repeats; ++r) {
        LP_TRY(prepare());
        LP_HIP(hipEventRecord(c->rs.ev_begin, c->rs.st));
        LP_TRY(body());
        LP_HIP(hipEventRecord(c->rs.ev_end, c->rs.st));
        LP_HIP(hipStreamSynchronize(c->rs.st));
        float ms = 0.f;
        LP_HIP(hipEventElapsedTime(&ms, c->rs.ev_begin, c->rs.ev_end));
        total += ms;
    }
    if (ms_out) *ms_out = total / repeats;
    return LPIPM_OK;
}
// 2. One bracket around `repeats` launches back to back; *ms_out is the bracket over the repeats.  lpipm_k_pack_matrix, for its
//    launch and for the runtime's copy beside it: a copy's rate is that of a queue kept full (profiles/device_upload.md).
template <typename F>
static int timed_back_to_back(lpipm_ctx* c, int repeats, double* ms_out, F&& launch) {
    if (repeats < 1) repeats = 1;
    LP_HIP(hipEventRecord(c->rs.ev_begin, c->rs.st));
    for (int r = 0; r < repeats; ++r) LP_HIP(launch());
    LP_HIP(hipEventRecord(c->rs.ev_end, c->rs.st));
    LP_HIP(hipStreamSynchronize(c->rs.st));
    float ms = 0.f;
    LP_HIP(hipEventElapsedTime(&ms, c->rs.ev_begin, c->rs.ev_end));
    if (ms_out) *ms_out = (double)ms / repeats;
    return LPIPM_OK;
}

// `rows` rows of `width` doubles from a block of row length ld_src to one of row length ld_dst: every size in doubles.  Every
// strided copy of the entries is one of these.
static hipError_t copy_rows(double* dst, size_t ld_dst, const double* src, size_t ld_src, size_t width, size_t rows, hipMemcpyKind kind,
                            hipStream_t st) {
    const size_t D = sizeof(double);
    return hipMemcpy2DAsync(dst, ld_dst * D, src, ld_src * D, width * D, rows, kind, st);
}
static hipError_t rows_to_device(double* dst, size_t ld_dev, const double* src, size_t ld_host, size_t width, size_t rows, hipStream_t st) {
    return copy_rows(dst, ld_dev, src, ld_host, width, rows, hipMemcpyHostToDevice, st);
}
static hipError_t rows_to_host(double* dst, size_t ld_host, const double* src, size_t ld_dev, size_t width, size_t rows, hipStream_t st) {
    return copy_rows(dst, ld_host, src, ld_dev, width, rows, hipMemcpyDeviceToHost, st);
}

// Device memory for the length of one entry.  Whichever way the entry is left, the destructor drains the stream the memory was
// used on and only then frees it: nothing enqueued may outlive what it reads or writes.
struct DeviceTemp {
    hipStream_t st;
    std::vector<void*> taken;
    explicit DeviceTemp(hipStream_t s) : st(s) {}
    DeviceTemp(const DeviceTemp&) = delete;
    ~DeviceTemp() { (void)hipStreamSynchronize(st); free_list(taken); }
    template <typename T>
    int take(T** out, size_t count, bool zero) {
        void* p = nullptr;
        LP_HIP(hipMalloc(&p, count * sizeof(T)));
        taken.push_back(p);
        if (zero) LP_HIP(hipMemsetAsync(p, 0, count * sizeof(T), st));
        *out = (T*)p;
        return LPIPM_OK;
    }
};

extern "C" int lpipm_k_resident_matrix(lpipm_ctx* c, uint64_t member, uint64_t rows, uint64_t cols, double* out, uint64_t ld,
                                       uint64_t* mp_out, uint64_t* npa_out) {
    if (!c || (rows && cols && !out)) return LPIPM_ERR_BAD_ARGUMENT;
    if (!c->p.has_problem) return LPIPM_ERR_NO_PROBLEM;
    const Problem& p = c->p;
    if (member >= (uint64_t)(p.shared_a ? 1 : p.B) || rows > (uint64_t)p.mp || cols > (uint64_t)p.npa || ld < cols) return LPIPM_ERR_BAD_ARGUMENT;
    if (mp_out) *mp_out = (uint64_t)p.mp;
    if (npa_out) *npa_out = (uint64_t)p.npa;
    if (rows == 0 || cols == 0) return LPIPM_OK;
    LP_HIP(hipSetDevice(c->device));
    const char* img = (const char*)p.A + (p.shared_a ? 0 : (size_t)member * p.bstride);
    LP_HIP(rows_to_host(out, ld, (const double*)img, (size_t)p.npa, cols, rows, c->rs.st));
    LP_HIP(hipStreamSynchronize(c->rs.st));
    return LPIPM_OK;
}

extern "C" int lpipm_k_pack_matrix(lpipm_ctx* c, const lpipm_device_problem* d, int repeats, double* pack_ms_out, double* copy_ms_out) {
    if (!c) return LPIPM_ERR_BAD_ARGUMENT;
    DeviceRequest q;
    LP_TRY(device_request(d, q));
    LP_TRY(check_upload(c, q.u));
    Problem& p = c->p;
    if (!p.has_problem) return LPIPM_ERR_NO_PROBLEM;
    if (c->world > 1 || p.scale_passes > 0) return LPIPM_ERR_UNSUPPORTED;      // (the launch would put the unscaled matrix back)
    LP_HIP(hipSetDevice(c->device));
    LP_TRY(sources_inside(c, q.u));
    // the resident problem must be this descriptor's: the launch writes its m x nx block into the resident image
    if (q.u.m != p.m || q.u.n != p.n || q.u.count != (uint64_t)p.B || q.u.shared != p.shared_a || q.u.tall != p.tall ||
        q.u.parts.has_value() != p.from_parts || (q.u.parts && q.u.n_slack != (uint64_t)p.ns))     // (parts: the same `ub` rows, so the same columns)
        return LPIPM_ERR_BAD_ARGUMENT;
    hipStream_t st = c->rs.st;
    const PackMatrix pm = pack_matrix_of(p, *d);
    const bool f32 = d->src_type == LPIPM_SRC_F32;
    const int members = member_strided(d) ? p.B : 1;
    LP_TRY(timed_back_to_back(c, repeats, pack_ms_out, [&] { return launch_pack_matrix(pm, f32, members, st); }));
    // the runtime's copy of as many bytes: the launch reads elements of the source type and writes doubles
    const size_t elems = (size_t)members * (size_t)p.m * (size_t)p.nx;
    const size_t bytes = elems * (src_elem_bytes(d->src_type) + sizeof(double)) / 2;
    DeviceTemp tmp{st};
    char *from = nullptr, *to = nullptr;
    LP_TRY(tmp.take(&from, bytes, true));
    LP_TRY(tmp.take(&to, bytes, false));
    return timed_back_to_back(c, repeats, copy_ms_out, [&] { return hipMemcpyDtoDAsync((hipDeviceptr_t)to, (hipDeviceptr_t)from, bytes, st); });
}

extern "C" int lpipm_k_adat(lpipm_ctx* c, const double* dinv, double* M_out, int repeats, double* ms_out) {
    if (!c || !dinv || !M_out) return LPIPM_ERR_BAD_ARGUMENT;
    if (!c->p.has_problem) return LPIPM_ERR_NO_PROBLEM;
    if (c->p.tall) return LPIPM_ERR_UNSUPPORTED;           // a tall upload has no M (lpipm_k_tall_normal returns K)
    if (c->p.box) return LPIPM_ERR_UNSUPPORTED;            // a bounded upload builds M~ from D~ (lpipm_k_bounded_normal returns it)
    LP_HIP(hipSetDevice(c->device));
    LP_HIP(hipMemcpyAsync(c->p.va.dinv, dinv, c->p.n * sizeof(double), hipMemcpyHostToDevice, c->rs.st));
    LP_TRY(timed_repeats(c, repeats, ms_out, [&]() -> int { LP_HIP(build_system(c, c->p.sys[SYS_WORK], Batch{}, BuildOpts{.M2 = c->p.M0})); return LPIPM_OK; }));
    LP_HIP(rows_to_host(M_out, c->p.m, c->p.sys[SYS_WORK].M, (size_t)c->p.mp, c->p.m, c->p.m, c->rs.st));
    LP_HIP(hipStreamSynchronize(c->rs.st));
    return LPIPM_OK;
}

// What the tall kernel entries start from: the iterate x = dinv, z = 1 (so that W_s = 1 / dinv_s and E_x = 1 / dinv_x), W_s, E_x
// and t of the nrhs given right-hand sides, K built and, `factor`, factored.  Ahead of a reduced solve (nrhs > 0): tall_eq_reset.
static int tall_entry_system(lpipm_ctx* c, const double* dinv, bool factor, int nrhs = 0, const double* r1 = nullptr,
                             const double* r2 = nullptr, const double* r1b = nullptr, const double* r2b = nullptr) {
    hipStream_t st = c->rs.st;
    NormalSystem& K = c->p.sys[SYS_WORK];
    const std::vector<double> ones((size_t)c->p.n, 1.0);
    invalidate_duals(c);
    vec_blind_start(c->p.va, st);                  // clears done / flags; the iterate is overwritten next
    if (nrhs > 0) LP_TRY(tall_eq_reset(c));
    LP_HIP(hipMemcpyAsync(c->p.va.x, dinv, c->p.n * sizeof(double), hipMemcpyHostToDevice, st));
    LP_HIP(hipMemcpyAsync(c->p.va.z, ones.data(), c->p.n * sizeof(double), hipMemcpyHostToDevice, st));
    LP_HIP(hipStreamSynchronize(st));              // `ones` goes out of scope
    tall_setup(c->p.va, c->p.tv, true, nrhs, r1, r2, r1b, r2b, st);
    LP_HIP(build_system(c, K, Batch{}));
    if (factor) LP_HIP(launch_potrf(*K.factor, K.info, st, Batch{}, nullptr, true, nullptr));
    return LPIPM_OK;
}
extern "C" int lpipm_k_tall_normal(lpipm_ctx* c, const double* dinv, double* K_out) {
    if (!c || !dinv || !K_out) return LPIPM_ERR_BAD_ARGUMENT;
    if (!c->p.has_problem) return LPIPM_ERR_NO_PROBLEM;
    if (!c->p.tall || c->p.shared_a || c->p.owned_tall) return LPIPM_ERR_UNSUPPORTED;     // (a single tall upload, not a batch)
    LP_HIP(hipSetDevice(c->device));
    LP_TRY(tall_entry_system(c, dinv, false));
    const size_t nx = (size_t)c->p.nx;
    LP_HIP(rows_to_host(K_out, nx, c->p.sys[SYS_WORK].M, (size_t)c->p.tv.nxp, nx, nx, c->rs.st));
    LP_HIP(hipStreamSynchronize(c->rs.st));
    return LPIPM_OK;
}
extern "C" int lpipm_k_tall_schur(lpipm_ctx* c, const double* dinv, double* S_out) {
    if (!c || !dinv || !S_out) return LPIPM_ERR_BAD_ARGUMENT;
    if (!c->p.has_problem) return LPIPM_ERR_NO_PROBLEM;
    if (!c->p.tall_eq || c->p.shared_a) return LPIPM_ERR_UNSUPPORTED;   // (the upload of lpipm_upload_ub_eq_tall with m_eq > 0, nothing else)
    LP_HIP(hipSetDevice(c->device));
    hipStream_t st = c->rs.st;
    const TallArgs& t = c->p.tv;
    LP_TRY(tall_entry_system(c, dinv, true));
    LP_TRY(tall_eq_schur(c, false));
    const size_t me = (size_t)t.me;
    LP_HIP(rows_to_host(S_out, me, c->p.sys[SYS_SCHUR].M, (size_t)t.mep, me, me, st));
    LP_HIP(hipMemsetAsync(c->p.va.potrf_info, 0, sizeof(int32_t), st));      // the solver expects a clean word
    LP_HIP(hipStreamSynchronize(st));
    return LPIPM_OK;
}
extern "C" int lpipm_k_tall_sym_solve(lpipm_ctx* c, const double* dinv, int nrhs, const double* R1, const double* R2,
                                      double* U_out, double* V_out, int32_t* info_out) {
    if (!c || !dinv || !R1 || !R2 || !U_out || !V_out || (nrhs != 1 && nrhs != 2)) return LPIPM_ERR_BAD_ARGUMENT;
    if (!c->p.has_problem) return LPIPM_ERR_NO_PROBLEM;
    if (!c->p.tall || c->p.shared_a || c->p.owned_tall) return LPIPM_ERR_UNSUPPORTED;     // (a single tall upload, not a batch)
    LP_HIP(hipSetDevice(c->device));
    hipStream_t st = c->rs.st;
    VecArgs& v = c->p.va;
    const TallArgs& t = c->p.tv;
    const size_t n = (size_t)c->p.n, m = (size_t)c->p.m, np = (size_t)c->p.np, mp = (size_t)c->p.mp;
    // the right-hand sides on the device, rows padded as the solver's own vectors are: R1 as [nrhs][np], R2 as [nrhs][mp]
    DeviceTemp tmp{st};
    double* rhs = nullptr;
    LP_TRY(tmp.take(&rhs, 2 * (np + mp), true));
    double* r1 = rhs;
    double* r2 = rhs + 2 * np;
    int32_t info = 0;
    lpipm_opts o;
    lpipm_default_opts(&o);
    LP_HIP(rows_to_device(r1, np, R1, n, n, (size_t)nrhs, st));
    LP_HIP(rows_to_device(r2, mp, R2, m, m, (size_t)nrhs, st));
    const double* r1b = nrhs == 2 ? r1 + np : nullptr;
    const double* r2b = nrhs == 2 ? r2 + mp : nullptr;
    LP_TRY(tall_entry_system(c, dinv, true, nrhs, r1, r2, r1b, r2b));
    if (c->p.tall_eq) LP_TRY(tall_eq_schur(c));
    LP_TRY(sym_solve(c, Iter{}, &o, SymRhs{nrhs, r1, r2, r1b, r2b}));
    if (nrhs == 2) tall_pq_uv(v, t, r1, r1b, st);
    else           tall_uv_corr(v, t, r1, st);
    LP_HIP(hipGetLastError());
    // nrhs == 2: (p, q) and (u, v) as the predictor leaves them; nrhs == 1: (u, v) as the corrector does
    if (nrhs == 2) LP_HIP(hipMemcpyAsync(U_out, v.p, n * sizeof(double), hipMemcpyDeviceToHost, st));
    LP_HIP(hipMemcpyAsync(U_out + (nrhs == 2 ? n : 0), v.u, n * sizeof(double), hipMemcpyDeviceToHost, st));
    LP_HIP(rows_to_host(V_out, m, v.R, mp, m, (size_t)nrhs, st));
    LP_HIP(hipMemcpyAsync(&info, v.potrf_info, sizeof(int32_t), hipMemcpyDeviceToHost, st));
    LP_HIP(hipMemsetAsync(v.potrf_info, 0, sizeof(int32_t), st));     // the solver expects a clean word
    LP_HIP(hipStreamSynchronize(st));
    if (info_out) *info_out = info;
    return LPIPM_OK;
}

// What the bounded kernel entries start from: the iterate x = dinv_ext, z = 1 over all n + nb columns (so that x / z, which the
// set-up takes from the vector k_pred_setup leaves it in, is dinv_ext), D~ and the ratios, W of the nrhs given right-hand
// sides, M~ built and, `factor`, factored.
static int box_entry_system(lpipm_ctx* c, const double* dinv, bool factor, int nrhs = 0, const double* r1 = nullptr,
                            const double* r2 = nullptr, const double* r1b = nullptr, const double* r2b = nullptr) {
    hipStream_t st = c->rs.st;
    NormalSystem& M = c->p.sys[SYS_WORK];
    const std::vector<double> ones((size_t)c->p.n, 1.0);
    invalidate_duals(c);
    vec_blind_start(c->p.va, st);                  // clears done / flags; the iterate is overwritten next
    LP_TRY(box_reset(c));
    LP_HIP(hipMemcpyAsync(c->p.va.x, dinv, c->p.n * sizeof(double), hipMemcpyHostToDevice, st));
    LP_HIP(hipMemcpyAsync(c->p.va.dinv, dinv, c->p.n * sizeof(double), hipMemcpyHostToDevice, st));
    LP_HIP(hipMemcpyAsync(c->p.va.z, ones.data(), c->p.n * sizeof(double), hipMemcpyHostToDevice, st));
    LP_HIP(hipStreamSynchronize(st));              // `ones` goes out of scope
    box_setup(c->p.va, c->p.bx, true, nrhs, r1, r2, r1b, r2b, st);
    LP_HIP(build_system(c, M, Batch{}));
    if (factor) LP_HIP(launch_potrf(*M.factor, M.info, st, Batch{}, nullptr, true, nullptr));
    return LPIPM_OK;
}
extern "C" int lpipm_k_bounded_normal(lpipm_ctx* c, const double* dinv_ext, double* M_out) {
    if (!c || !dinv_ext || !M_out) return LPIPM_ERR_BAD_ARGUMENT;
    if (!c->p.has_problem) return LPIPM_ERR_NO_PROBLEM;
    if (!c->p.box) return LPIPM_ERR_UNSUPPORTED;
    LP_HIP(hipSetDevice(c->device));
    LP_TRY(box_entry_system(c, dinv_ext, false));
    const size_t ma = (size_t)c->p.ma;
    LP_HIP(rows_to_host(M_out, ma, c->p.sys[SYS_WORK].M, (size_t)c->p.mp, ma, ma, c->rs.st));
    LP_HIP(hipStreamSynchronize(c->rs.st));
    return LPIPM_OK;
}
extern "C" int lpipm_k_bounded_sym_solve(lpipm_ctx* c, const double* dinv_ext, int nrhs, const double* R1, const double* R2,
                                         double* U_out, double* V_out, int32_t* info_out) {
    if (!c || !dinv_ext || !R1 || !R2 || !U_out || !V_out || (nrhs != 1 && nrhs != 2)) return LPIPM_ERR_BAD_ARGUMENT;
    if (!c->p.has_problem) return LPIPM_ERR_NO_PROBLEM;
    if (!c->p.box) return LPIPM_ERR_UNSUPPORTED;
    LP_HIP(hipSetDevice(c->device));
    hipStream_t st = c->rs.st;
    VecArgs& v = c->p.va;
    const size_t n = (size_t)c->p.n, m = (size_t)c->p.m, np = (size_t)v.np, mp = (size_t)v.mp;
    // the right-hand sides on the device, rows padded as the solver's own vectors are: R1 as [nrhs][np], R2 as [nrhs][mp]
    DeviceTemp tmp{st};
    double* rhs = nullptr;
    LP_TRY(tmp.take(&rhs, 2 * (np + mp), true));
    double* r1 = rhs;
    double* r2 = rhs + 2 * np;
    int32_t info = 0;
    lpipm_opts o;
    lpipm_default_opts(&o);
    LP_HIP(rows_to_device(r1, np, R1, n, n, (size_t)nrhs, st));
    LP_HIP(rows_to_device(r2, mp, R2, m, m, (size_t)nrhs, st));
    const double* r1b = nrhs == 2 ? r1 + np : nullptr;
    const double* r2b = nrhs == 2 ? r2 + mp : nullptr;
    LP_TRY(box_entry_system(c, dinv_ext, true, nrhs, r1, r2, r1b, r2b));
    LP_TRY(sym_solve(c, Iter{}, &o, SymRhs{nrhs, r1, r2, r1b, r2b}));
    if (nrhs == 2) box_pq_uv(v, c->p.bx, r1, r2, r1b, r2b, st);
    else           box_uv_corr(v, c->p.bx, r1, r2, st);
    LP_HIP(hipGetLastError());
    // nrhs == 2: (p, q) and (u, v) as the predictor leaves them; nrhs == 1: (u, v) as the corrector does
    if (nrhs == 2) LP_HIP(hipMemcpyAsync(U_out, v.p, n * sizeof(double), hipMemcpyDeviceToHost, st));
    LP_HIP(hipMemcpyAsync(U_out + (nrhs == 2 ? n : 0), v.u, n * sizeof(double), hipMemcpyDeviceToHost, st));
    LP_HIP(rows_to_host(V_out, m, v.R, mp, m, (size_t)nrhs, st));
    LP_HIP(hipMemcpyAsync(&info, v.potrf_info, sizeof(int32_t), hipMemcpyDeviceToHost, st));
    LP_HIP(hipMemsetAsync(v.potrf_info, 0, sizeof(int32_t), st));     // the solver expects a clean word
    LP_HIP(hipStreamSynchronize(st));
    if (info_out) *info_out = info;
    return LPIPM_OK;
}
// lpipm_k_gemv_n, lpipm_k_gemv_t and lpipm_k_gemv_dual on a bounded upload: they see A_ext at its extended lengths.  The pass
// runs over A from the first na (ma) entries of its input, which go into the solve's own buffers (rows nps and mps apart); the
// whole input sits in va.W / va.R, and box_products adds the bound block.  w: nrhs rows of n entries (null: no product A_ext.w),
// v: nrhs rows of m entries (null: no A_ext^T.v); dual: both in one read of A (one right-hand side).
static int box_k_passes(lpipm_ctx* c, int nrhs, const double* w, const double* v, bool dual, double* Aw_out, double* ATv_out,
                        int repeats, double* ms_out) {
    Problem& p = c->p;
    VecArgs& va = p.va;
    const BoxArgs& bx = p.bx;
    hipStream_t st = c->rs.st;
    const size_t n = (size_t)p.n, m = (size_t)p.m, na = (size_t)p.na, ma = (size_t)p.ma;
    if (w) {
        LP_HIP(rows_to_device(va.W, (size_t)va.np, w, n, n, (size_t)nrhs, st));
        if (bx.nf > 0) box_net(va, bx, va.W, va.np, bx.Wb, bx.nps, nrhs, false, st);      // free columns: the pass reads the net rows
        else LP_HIP(rows_to_device(bx.Wb, (size_t)bx.nps, w, n, na, (size_t)nrhs, st));
    }
    if (v) {
        LP_HIP(hipMemsetAsync(bx.Rs, 0, 2 * (size_t)bx.mps * sizeof(double), st));
        LP_HIP(rows_to_device(va.R, (size_t)va.mp, v, m, m, (size_t)nrhs, st));
        LP_HIP(rows_to_device(bx.Rs, (size_t)bx.mps, v, m, ma, (size_t)nrhs, st));
    }
    const int nch = gemv_dual_chunks(p.npa);
    LP_TRY(timed_repeats(c, repeats, ms_out, [&]() -> int {
        if (dual) {
            LP_HIP(ctx_gemv_dual(c, bx.Wb, bx.Rs, va.Ax, Batch{}));
            box_products(va, bx, BoxProducts{va.W, va.Ax, nch, va.q, va.R, p.ATpart, (long long)bx.nps, va.u}, st);
        } else if (w) {        // A.w_x into the rows of dy-sized scratch: Y, nrhs rows mps apart, then whole into rP / rP2
            LP_HIP(ctx_gemv_n(c, nrhs, bx.Wb, nullptr, nullptr, p.Y, Batch{}));
            for (int r = 0; r < nrhs; ++r)
                box_products(va, bx, BoxProducts{va.W + (size_t)r * va.np, p.Y + (size_t)r * bx.mps, 1, r ? va.rP2 : va.rP}, st);
        } else {
            LP_HIP(ctx_gemv_t(c, nrhs, bx.Rs, Batch{}));
            for (int r = 0; r < nrhs; ++r)
                box_products(va, bx, BoxProducts{nullptr, nullptr, 1, nullptr, va.R + (size_t)r * va.mp, p.ATpart + (size_t)r * bx.nps,
                                                 (long long)nrhs * bx.nps, r ? va.p : va.u}, st);
        }
        LP_HIP(hipGetLastError());
        return LPIPM_OK;
    }));
    if (dual) {
        LP_HIP(hipMemcpyAsync(Aw_out, va.q, m * sizeof(double), hipMemcpyDeviceToHost, st));
        LP_HIP(hipMemcpyAsync(ATv_out, va.u, n * sizeof(double), hipMemcpyDeviceToHost, st));
    } else if (w) {
        for (int r = 0; r < nrhs; ++r) LP_HIP(hipMemcpyAsync(Aw_out + (size_t)r * m, r ? va.rP2 : va.rP, m * sizeof(double), hipMemcpyDeviceToHost, st));
    } else {
        for (int r = 0; r < nrhs; ++r) LP_HIP(hipMemcpyAsync(ATv_out + (size_t)r * n, r ? va.p : va.u, n * sizeof(double), hipMemcpyDeviceToHost, st));
    }
    LP_HIP(hipStreamSynchronize(st));
    return LPIPM_OK;
}

// dst (mp x mp, zeroed) <- [[M, 0], [0, I]] from the host's m x m M (mp - m < NB; the ones outlive every copy)
static hipError_t copy_padded(double* dst, int mp, const double* M, size_t m, hipStream_t st) {
    static const std::vector<double> ones((size_t)NB, 1.0);
    const hipError_t e = rows_to_device(dst, (size_t)mp, M, m, m, m, st);
    if (e != hipSuccess || (size_t)mp == m) return e;
    return rows_to_device(dst + m * mp + m, (size_t)mp + 1, ones.data(), 1, 1, mp - m, st);      // (the diagonal: one double per "row")
}
static int kbuf_ensure(lpipm_ctx* c, int mp) {
    lpipm_ctx::KernelScratch& k = c->k;
    if (k.mp == mp) return LPIPM_OK;
    hipStream_t st = c->rs.st;
    LP_HIP(hipStreamSynchronize(st));
    free_list(k.allocs);
    factor_plan_destroy(k.plan);
    k.mp = 0; k.chol_valid = false;
    double* M = nullptr;
    LP_TRY(dalloc(k.allocs, nullptr, &M, (size_t)mp * mp, st));
    LP_TRY(dalloc(k.allocs, nullptr, &k.M0, (size_t)mp * mp, st));
    LP_TRY(dalloc(k.allocs, nullptr, &k.R, (size_t)2 * mp, st));
    LP_TRY(dalloc(k.allocs, nullptr, &k.Y, (size_t)2 * mp, st));
    LP_TRY(dalloc(k.allocs, nullptr, &k.info, 1, st));
    LP_TRY(dalloc(k.allocs, nullptr, &k.tau, (size_t)mp, st));
    Arena measure;
    LP_HIP(factor_plan_create(k.plan, M, mp, mp, measure, false, st, super_for(mp), merge_edge_for(1), nullptr, coupled_for(mp, true), couple_edge_for()));
    char* kar = nullptr;
    LP_TRY(dalloc(k.allocs, nullptr, &kar, measure.off + 256, st));   // zeroed
    Arena real{kar};
    LP_HIP(factor_plan_create(k.plan, M, mp, mp, real, true, st, super_for(mp), merge_edge_for(1), nullptr, coupled_for(mp, true), couple_edge_for()));
    k.mp = mp;
    return LPIPM_OK;
}

// Debug aid (LPIPM_DIAG_STAMPS): one more factorisation of the pristine copy with the cycle stamps of its first diagonal-block
// kernel collected, printed to stderr.  Best effort: a failure prints nothing.
static void dump_diag_stamps(lpipm_ctx* c, int mp) {
    DeviceTemp tmp{c->rs.st};
    long long* d = nullptr; long long h[64] = {0};
    if (tmp.take(&d, 64, true) != LPIPM_OK) return;
    g_diag_stamps = d;
    (void)hipMemcpyAsync(c->k.plan.L, c->k.M0, (size_t)mp * mp * sizeof(double), hipMemcpyDeviceToDevice, c->rs.st);
    (void)launch_potrf(c->k.plan, c->k.info, c->rs.st);
    (void)hipStreamSynchronize(c->rs.st);
    g_diag_stamps = nullptr;
    (void)hipMemcpy(h, d, sizeof(h), hipMemcpyDeviceToHost);
    fprintf(stderr, "diag stamps (cycles): E(0) %lld, P tile + wait for all eight on wave 0 %lld, barrier to barrier (k = 1) %lld, "
            "all block columns %lld, last stores %lld\n  k = 1, cycles after the barrier, per wave: P tile done",
            h[1]-h[0], h[2]-h[1], h[3]-h[1], h[6]-h[0], h[7]-h[6]);
    for (int w = 0; w < 16; ++w) fprintf(stderr, " %lld", h[32 + w] - h[1]);
    fprintf(stderr, "\n  at the next barrier");
    for (int w = 0; w < 16; ++w) fprintf(stderr, " %lld", h[16 + w] - h[1]);
    fprintf(stderr, "\n");
}

extern "C" int lpipm_k_potrf(lpipm_ctx* c, uint64_t m, double* M_inout, int32_t* info_out, int repeats,
                             double* ms_out) {
    if (!c || !M_inout || m == 0 || m > (1u << 20)) return LPIPM_ERR_BAD_ARGUMENT;
    LP_HIP(hipSetDevice(c->device));
    const int mp = (int)round_up(m, NB);
    LP_TRY(kbuf_ensure(c, mp));
    // padded pristine copy: [[M, 0], [0, I]]
    LP_HIP(hipMemsetAsync(c->k.M0, 0, (size_t)mp * mp * sizeof(double), c->rs.st));
    LP_HIP(copy_padded(c->k.M0, mp, M_inout, m, c->rs.st));
    LP_HIP(hipStreamSynchronize(c->rs.st));
    auto restore = [&]() -> int {      // the factorisation is in place: every repeat starts from the pristine copy
        LP_HIP(hipMemcpyAsync(c->k.plan.L, c->k.M0, (size_t)mp * mp * sizeof(double), hipMemcpyDeviceToDevice, c->rs.st));
        return LPIPM_OK;
    };
    LP_TRY(timed_repeats(c, repeats, ms_out, [&]() -> int { LP_HIP(launch_potrf(c->k.plan, c->k.info, c->rs.st, Batch{}, lookahead(c))); return LPIPM_OK; }, restore));
    if (lp_knob("LPIPM_DIAG_STAMPS")) dump_diag_stamps(c, mp);
    int32_t info = 0;
    LP_HIP(hipMemcpyAsync(&info, c->k.info, sizeof(int32_t), hipMemcpyDeviceToHost, c->rs.st));
    LP_HIP(rows_to_host(M_inout, m, c->k.plan.L, (size_t)mp, m, m, c->rs.st));
    LP_HIP(hipStreamSynchronize(c->rs.st));
    if (info_out) *info_out = info;
    c->k.chol_valid = true;
    return LPIPM_OK;
}

extern "C" int lpipm_k_factor_inverses(lpipm_ctx* c, uint64_t m, double* inv_out, double* invT_out, int32_t* super_w_out) {
    if (!c || !inv_out || !invT_out) return LPIPM_ERR_BAD_ARGUMENT;
    const int mp = (int)round_up(m, NB);
    if (c->k.mp != mp || !c->k.chol_valid) return LPIPM_ERR_NO_PROBLEM;  // needs a preceding lpipm_k_potrf of this size
    LP_HIP(hipSetDevice(c->device));
    std::fill(inv_out, inv_out + (size_t)mp * mp, 0.0);
    std::fill(invT_out, invT_out + (size_t)mp * mp, 0.0);
    for (const SuperBlock& s : c->k.plan.sbs) {
        const size_t w = (size_t)s.size, at = (size_t)s.row0 * mp + s.row0;
        LP_HIP(rows_to_host(inv_out + at, (size_t)mp, s.inv, w, w, w, c->rs.st));
        LP_HIP(rows_to_host(invT_out + at, (size_t)mp, s.invT, w, w, w, c->rs.st));
    }
    LP_HIP(hipStreamSynchronize(c->rs.st));
    if (super_w_out) *super_w_out = c->k.plan.super_w;
    return LPIPM_OK;
}

// The members of a lockstep factorisation, each in an arena of its own with identical layouts `stride` bytes apart: the padded
// matrix, the info word, whatever `extra` takes, the inverse storage of the plan.  factor() measures one arena, takes `count`
// of them zeroed, lays the plan out over member 0's, loads the padded matrices [[M, 0], [0, I]] from the host's `count` m x m
// ones and enqueues ONE launch_potrf over the members.  The order of the takes, the stride, super_for and merge_edge_for are
// those of a lockstep solve: the bits of the factors depend on them.
struct LockstepFactor {
    hipStream_t st;
    FactorPlan plan;
    double* M = nullptr; int32_t* info = nullptr;       // member 0's; member() gives member q's
    int mp = 0, count = 0;
    size_t stride = 0;
    DeviceTemp tmp;
    explicit LockstepFactor(hipStream_t s) : st(s), tmp(s) {}
    ~LockstepFactor() {                                 // the plan goes as the memory does: after a drain (tmp frees after this)
        (void)hipStreamSynchronize(st);
        factor_plan_destroy(plan);
    }
    template <typename T>
    T* member(T* of_first, int q) const { return (T*)((char*)of_first + (size_t)q * stride); }
    Batch batch(const int* done = nullptr) const { return Batch{count, (long long)stride, done, 0}; }
    template <typename Extra>
    int factor(int mp_, int count_, const double* Ms, size_t m, Extra&& extra) {
        mp = mp_; count = count_;
        auto layout = [&](Arena& ar, bool build) -> hipError_t {
            M = ar.take<double>((size_t)mp * mp);
            info = ar.take<int32_t>(1);
            extra(ar);
            return factor_plan_create(plan, M, mp, mp, ar, build, st, super_for(mp), merge_edge_for(count));
        };
        Arena measure;
        LP_HIP(layout(measure, false));
        stride = round_up(measure.off + 256, 4096);
        char* base = nullptr;
        LP_TRY(tmp.take(&base, stride * (size_t)count, true));
        Arena real{base};
        LP_HIP(layout(real, true));
        for (int q = 0; q < count; ++q) LP_HIP(copy_padded(member(M, q), mp, Ms + (size_t)q * m * m, m, st));
        LP_HIP(launch_potrf(plan, info, st, batch()));
        return LPIPM_OK;
    }
};

extern "C" int lpipm_k_potrf_lockstep(lpipm_ctx* c, uint64_t m, int count, double* Ms_inout, int32_t* infos_out) {
    if (!c || !Ms_inout || !infos_out || m == 0 || m > 16384 || count < 1 || count > 64) return LPIPM_ERR_BAD_ARGUMENT;
    LP_HIP(hipSetDevice(c->device));
    hipStream_t st = c->rs.st;
    LockstepFactor f{st};
    LP_TRY(f.factor((int)round_up(m, NB), count, Ms_inout, m, [](Arena&) {}));
    for (int q = 0; q < count; ++q) {
        LP_HIP(rows_to_host(Ms_inout + (size_t)q * m * m, m, f.member(f.M, q), (size_t)f.mp, m, m, st));
        LP_HIP(hipMemcpyAsync(infos_out + q, f.member(f.info, q), sizeof(int32_t), hipMemcpyDeviceToHost, st));
    }
    LP_HIP(hipStreamSynchronize(st));
    return LPIPM_OK;
}

// Z = B . L^-T for every member of a lockstep batch: `count` n x n SPD matrices factored as lpipm_k_potrf_lockstep factors
// them, then ONE launch_trsm_lt over the members.  B: one rows x cols block (ld ldb) when shared_b, else `count` of them, rows * ldb
// doubles apart.  Z_inout: count blocks of round_up(rows, 16) x round_up(n, 128) doubles; what they hold on entry is what the
// members' Z hold before the launch, so a member the launch skips hands it back.  done_mask (nullable): one int per member,
// non-zero = finished.  With count == 1 and no mask the launch has no member dimension: it is the single kernel's.
extern "C" int lpipm_k_trsm_lt_lockstep(lpipm_ctx* c, uint64_t n, int count, int rows, int cols, int shared_b, const double* Ms,
                                        const double* B, uint64_t ldb, double* Z_inout, int32_t* infos_out, const int32_t* done_mask) {
    if (!c || !Ms || !B || !Z_inout || !infos_out || n == 0 || n > 16384 || count < 1 || count > 64 || rows < 1 || rows > 4096 ||
        cols < 1 || (uint64_t)cols > n || ldb < (uint64_t)cols)
        return LPIPM_ERR_BAD_ARGUMENT;
    LP_HIP(hipSetDevice(c->device));
    const int mp = (int)round_up(n, NB), rp = (int)round_up((uint64_t)rows, 16);
    hipStream_t st = c->rs.st;
    const size_t zsize = (size_t)rp * mp;
    std::vector<int> done((size_t)count, 0);                      // (declared ahead of `f`: alive until its drain)
    for (int q = 0; q < count && done_mask; ++q) done[(size_t)q] = done_mask[q] != 0;
    // a member's arena also holds its done word, its block of B and its Z
    LockstepFactor f{st};
    int* done0 = nullptr; double *B0 = nullptr, *Z0 = nullptr;
    LP_TRY(f.factor(mp, count, Ms, n, [&](Arena& ar) {
        done0 = ar.take<int>(1);
        B0 = ar.take<double>((size_t)rows * cols);
        Z0 = ar.take<double>(zsize);
    }));
    for (int q = 0; q < count; ++q) {
        if (q == 0 || !shared_b) LP_HIP(rows_to_device(f.member(B0, q), (size_t)cols, B + (size_t)q * rows * ldb, ldb, (size_t)cols, (size_t)rows, st));
        LP_HIP(hipMemcpyAsync(f.member(Z0, q), Z_inout + (size_t)q * zsize, zsize * sizeof(double), hipMemcpyHostToDevice, st));
        LP_HIP(hipMemcpyAsync(f.member(done0, q), &done[(size_t)q], sizeof(int), hipMemcpyHostToDevice, st));
    }
    LP_HIP(launch_trsm_lt(B0, cols, rows, cols, f.plan, Z0, mp, st, f.batch(done_mask ? done0 : nullptr), shared_b != 0));
    for (int q = 0; q < count; ++q) {
        LP_HIP(hipMemcpyAsync(Z_inout + (size_t)q * zsize, f.member(Z0, q), zsize * sizeof(double), hipMemcpyDeviceToHost, st));
        LP_HIP(hipMemcpyAsync(infos_out + q, f.member(f.info, q), sizeof(int32_t), hipMemcpyDeviceToHost, st));
    }
    LP_HIP(hipStreamSynchronize(st));
    return LPIPM_OK;
}

// split >= 0: the forward steps [0, split) in a call of their own, the rest of the sweep in a second one (SolveSteps)
static int k_chol_solve_impl(lpipm_ctx* c, uint64_t m, int nrhs, const double* R, double* V, int repeats, double* ms_out, int split) {
    if (!c || !R || !V || (nrhs != 1 && nrhs != 2)) return LPIPM_ERR_BAD_ARGUMENT;
    const int mp = (int)round_up(m, NB);
    if (c->k.mp != mp || !c->k.chol_valid) return LPIPM_ERR_NO_PROBLEM;  // needs a preceding lpipm_k_potrf of this size
    LP_HIP(hipSetDevice(c->device));
    auto reload = [&]() -> int {       // the solve is in place: every repeat starts from the given right-hand sides
        LP_HIP(hipMemsetAsync(c->k.R, 0, (size_t)2 * mp * sizeof(double), c->rs.st));
        LP_HIP(rows_to_device(c->k.R, (size_t)mp, R, m, m, (size_t)nrhs, c->rs.st));
        return LPIPM_OK;
    };
    LP_TRY(timed_repeats(c, repeats, ms_out, [&]() -> int {
        if (split < 0) LP_HIP(launch_chol_solve(c->k.plan, nrhs, c->k.R, c->k.Y, c->rs.st));
        else {
            const int k = split < (int)c->k.plan.sbs.size() ? split : (int)c->k.plan.sbs.size();
            LP_HIP(launch_chol_solve(c->k.plan, nrhs, c->k.R, c->k.Y, c->rs.st, Batch{}, SolveSteps{0, k, false}));
            LP_HIP(launch_chol_solve(c->k.plan, nrhs, c->k.R, c->k.Y, c->rs.st, Batch{}, SolveSteps{k, -1, true}));
        }
        return LPIPM_OK;
    }, reload));
    LP_HIP(rows_to_host(V, m, c->k.R, (size_t)mp, m, (size_t)nrhs, c->rs.st));
    LP_HIP(hipStreamSynchronize(c->rs.st));
    return LPIPM_OK;
}

extern "C" int lpipm_k_chol_solve(lpipm_ctx* c, uint64_t m, int nrhs, const double* R, double* V, int repeats,
                                  double* ms_out) {
    return k_chol_solve_impl(c, m, nrhs, R, V, repeats, ms_out, -1);
}
extern "C" int lpipm_k_chol_solve_split(lpipm_ctx* c, uint64_t m, int nrhs, const double* R, double* V, int split) {
    if (split < 0) return LPIPM_ERR_BAD_ARGUMENT;
    return k_chol_solve_impl(c, m, nrhs, R, V, 1, nullptr, split);
}

// The sweep plan of an mp x mp factor as numbers (no device): see include/lpipm.h.
extern "C" int lpipm_k_sweep_plan(uint64_t m, int super_w, int coupled, int32_t* out, int cap, int32_t* count_out,
                                  uint64_t* coupling_bytes_out) {
    if (m == 0 || m > (1u << 20) || super_w < NB || super_w % NB != 0 || !out || !count_out || cap < 3) return LPIPM_ERR_BAD_ARGUMENT;
    const int mp = (int)round_up(m, NB);
    FactorPlan plan;
    Arena measure;
    LP_HIP(factor_plan_create(plan, nullptr, mp, mp, measure, false, nullptr, super_w, 32, nullptr,
                              coupled == 1 ? COUPLE_H | COUPLE_G : coupled == 2 ? COUPLE_H : coupled == 3 ? COUPLE_G : 0));
    std::vector<int32_t> v;
    const int nsb = (int)plan.sbs.size();
    v.push_back(nsb); v.push_back(plan.coupled ? 1 : 0); v.push_back(0);
    auto put = [&](int kind, int k, const SweepLaunch& l) {
        ++v[2];
        v.insert(v.end(), {kind, k, l.count, l.blocks});
        for (int i = l.first; i < l.first + l.count; ++i) {
            const SweepPiece& q = plan.pieces[(size_t)i];
            v.insert(v.end(), {q.rows, q.np0, q.A1 ? q.np1 : 0, q.w0, q.w0_y, q.A1 ? q.w1 : -1, q.w1_y, q.add, q.add_y, q.out, q.out_y, q.blk0});
        }
    };
    if (plan.coupled) {
        for (int k = 0; k < nsb && !plan.fwd.empty(); ++k) for (const SweepLaunch& l : plan.fwd[(size_t)k]) put(0, k, l);
        for (int i = 0; i < (int)plan.bwd.size(); ++i) put(1, nsb - 1 - i, plan.bwd[(size_t)i]);
        for (int k = 0; k < nsb; ++k) {
            const CoupleStep& cs = plan.couple[(size_t)k];
            v.insert(v.end(), {cs.lt ? cs.lt_row0 : -1, cs.lt ? cs.lt_ld : 0, plan.H[(size_t)k] ? 1 : 0, plan.G[(size_t)k] ? 1 : 0});
        }
    }
    if (coupling_bytes_out) *coupling_bytes_out = factor_coupling_bytes(mp, super_w, plan.coupled);
    factor_plan_destroy(plan);
    if ((int)v.size() > cap) return LPIPM_ERR_BAD_ARGUMENT;
    std::copy(v.begin(), v.end(), out);
    *count_out = (int32_t)v.size();
    return LPIPM_OK;
}

extern "C" int lpipm_k_symv_residual(lpipm_ctx* c, uint64_t m, const double* M, int nrhs, const double* V, const double* R0,
                                     double* Rho) {
    if (!c || !M || !V || !R0 || !Rho || m == 0 || m > 16384 || (nrhs != 1 && nrhs != 2)) return LPIPM_ERR_BAD_ARGUMENT;
    LP_HIP(hipSetDevice(c->device));
    const int mp = (int)round_up(m, NB);
    LP_TRY(kbuf_ensure(c, mp));
    hipStream_t st = c->rs.st;
    DeviceTemp tmp{st};
    double *ws = nullptr, *vbuf = nullptr;             // vbuf: V, R0 and Rho, two padded rows each
    LP_TRY(tmp.take(&ws, symv_slab_doubles(mp), false));
    LP_TRY(tmp.take(&vbuf, (size_t)6 * mp, true));
    double *Vd = vbuf, *R0d = vbuf + 2 * mp, *Rhod = vbuf + 4 * mp;
    LP_HIP(hipMemsetAsync(c->k.M0, 0, (size_t)mp * mp * sizeof(double), st));
    LP_HIP(rows_to_device(c->k.M0, (size_t)mp, M, m, m, m, st));
    LP_HIP(rows_to_device(Vd, (size_t)mp, V, m, m, (size_t)nrhs, st));
    LP_HIP(rows_to_device(R0d, (size_t)mp, R0, m, m, (size_t)nrhs, st));
    LP_HIP(launch_symv_residual(c->k.M0, mp, mp, nrhs, Vd, mp, R0d, mp, Rhod, mp, ws, st));
    LP_HIP(rows_to_host(Rho, m, Rhod, (size_t)mp, m, (size_t)nrhs, st));
    LP_HIP(hipStreamSynchronize(st));
    return LPIPM_OK;
}

extern "C" int lpipm_k_qr_solve(lpipm_ctx* c, uint64_t m, const double* M, int nrhs, const double* R, double* V,
                                int32_t* info_out, double* ms_out) {
    if (!c || !M || !R || !V || m == 0 || m > 16384 || (nrhs != 1 && nrhs != 2)) return LPIPM_ERR_BAD_ARGUMENT;
    LP_HIP(hipSetDevice(c->device));
    const int mp = (int)round_up(m, NB);
    LP_TRY(kbuf_ensure(c, mp));
    LP_HIP(hipMemsetAsync(c->k.plan.L, 0, (size_t)mp * mp * sizeof(double), c->rs.st));
    LP_HIP(copy_padded(c->k.plan.L, mp, M, m, c->rs.st));
    LP_HIP(hipMemsetAsync(c->k.R, 0, (size_t)2 * mp * sizeof(double), c->rs.st));
    LP_HIP(rows_to_device(c->k.R, (size_t)mp, R, m, m, (size_t)nrhs, c->rs.st));
    LP_TRY(timed_repeats(c, 1, ms_out, [&]() -> int {           // both are in place: one repeat
        LP_HIP(launch_qr_factor(c->k.plan.L, mp, mp, c->k.tau, c->k.info, c->rs.st));
        LP_HIP(launch_qr_solve(c->k.plan.L, mp, mp, c->k.tau, nrhs, c->k.R, c->k.info, c->rs.st));
        return LPIPM_OK;
    }));
    int32_t info = 0;
    LP_HIP(hipMemcpyAsync(&info, c->k.info, sizeof(int32_t), hipMemcpyDeviceToHost, c->rs.st));
    LP_HIP(rows_to_host(V, m, c->k.R, (size_t)mp, m, (size_t)nrhs, c->rs.st));
    LP_HIP(hipStreamSynchronize(c->rs.st));
    if (info_out) *info_out = info;
    c->k.chol_valid = false;   // plan.L no longer holds a Cholesky factor: lpipm_k_chol_solve needs a new lpipm_k_potrf
    return LPIPM_OK;
}

extern "C" int lpipm_k_gemv_n(lpipm_ctx* c, int nrhs, const double* W, double* Y, int repeats, double* ms_out) {
    if (!c || !W || !Y || (nrhs != 1 && nrhs != 2)) return LPIPM_ERR_BAD_ARGUMENT;
    if (!c->p.has_problem) return LPIPM_ERR_NO_PROBLEM;
    LP_HIP(hipSetDevice(c->device));
    if (c->p.box) return box_k_passes(c, nrhs, W, nullptr, false, Y, nullptr, repeats, ms_out);
    LP_HIP(rows_to_device(c->p.va.W, (size_t)c->p.np, W, c->p.n, c->p.n, (size_t)nrhs, c->rs.st));
    LP_TRY(timed_repeats(c, repeats, ms_out, [&]() -> int {
        LP_HIP(ctx_gemv_n(c, nrhs, c->p.va.W, nullptr, nullptr, c->p.va.R, Batch{}));
        return LPIPM_OK;
    }));
    LP_HIP(rows_to_host(Y, c->p.m, c->p.va.R, (size_t)c->p.mp, c->p.m, (size_t)nrhs, c->rs.st));
    LP_HIP(hipStreamSynchronize(c->rs.st));
    return LPIPM_OK;
}

extern "C" int lpipm_k_gemv_t(lpipm_ctx* c, int nrhs, const double* V, double* U, int repeats, double* ms_out) {
    if (!c || !V || !U || (nrhs != 1 && nrhs != 2)) return LPIPM_ERR_BAD_ARGUMENT;
    if (!c->p.has_problem) return LPIPM_ERR_NO_PROBLEM;
    LP_HIP(hipSetDevice(c->device));
    if (c->p.box) return box_k_passes(c, nrhs, nullptr, V, false, nullptr, U, repeats, ms_out);
    LP_HIP(hipMemsetAsync(c->p.va.R, 0, (size_t)2 * c->p.mp * sizeof(double), c->rs.st));
    LP_HIP(rows_to_device(c->p.va.R, (size_t)c->p.mp, V, c->p.m, c->p.m, (size_t)nrhs, c->rs.st));
    LP_TRY(timed_repeats(c, repeats, ms_out, [&]() -> int {
        LP_HIP(ctx_gemv_t(c, nrhs, c->p.va.R, Batch{}));
        if (c->p.tall) {   // slabs npa wide; the slack columns' A^T.v is v
            LP_HIP(launch_gemv_t_reduce(c->p.ATpart, c->p.nsplit, nrhs, c->p.npa, c->p.va.W, c->p.np, c->rs.st));
            LP_HIP(copy_rows(c->p.va.W + c->p.nx, (size_t)c->p.np, c->p.va.R, (size_t)c->p.mp, c->p.m, (size_t)nrhs, hipMemcpyDeviceToDevice, c->rs.st));
            return LPIPM_OK;
        }
        LP_HIP(launch_gemv_t_reduce(c->p.ATpart, c->p.nsplit, nrhs, c->p.np, c->p.va.W, c->p.np, c->rs.st));
        return LPIPM_OK;
    }));
    LP_HIP(rows_to_host(U, c->p.n, c->p.va.W, (size_t)c->p.np, c->p.n, (size_t)nrhs, c->rs.st));
    LP_HIP(hipStreamSynchronize(c->rs.st));
    return LPIPM_OK;
}

// One loop body of solve_normal_form (mod.rs:215-222) on the uploaded problem from a GIVEN iterate: what the loop does
// between two status read-backs -- residuals at the point (feasible_point.rs:122-125), normal equations, factor,
// predictor, corrector, step length, step.  For the differential tests of the vector stage (rhat.rs, delta.rs,
// feasible_point.rs:53-106) on arbitrary iterates, including ip = 1.
extern "C" int lpipm_k_iteration(lpipm_ctx* c, const lpipm_opts* o, int ip, double* x, double* y, double* z, double* tau,
                                 double* kappa, double* d_x, double* d_y, double* d_z, double* d_tk, double* alpha_out,
                                 int32_t* info_out) {
    if (!c || !o || !x || !y || !z || !tau || !kappa || !d_x || !d_y || !d_z || !d_tk || !alpha_out) return LPIPM_ERR_BAD_ARGUMENT;
    if (!c->p.has_problem) return LPIPM_ERR_NO_PROBLEM;
    if (c->p.B != 1 || (c->p.tall && (c->p.shared_a || c->p.owned_tall))) return LPIPM_ERR_UNSUPPORTED;      // one LP, not a batch (of any count)
    // (a column-split context: x, z, d_x, d_z are this rank's slices, everything else is replicated, and every rank must
    //  call together -- enqueue_residuals / enqueue_iteration contain the cross-rank reductions)
    LP_HIP(hipSetDevice(c->device));
    VecArgs& v = c->p.va;
    hipStream_t st = c->rs.st;
    const Iter it{.refine_now = c->refine == 2};
    invalidate_duals(c);
    vec_blind_start(v, st);                                   // clears done / flags; the iterate is overwritten next
    LP_TRY(tall_eq_reset(c));
    LP_TRY(box_reset(c));
    LP_HIP(hipMemcpyAsync(v.x, x, c->p.n * sizeof(double), hipMemcpyHostToDevice, st));
    LP_HIP(hipMemcpyAsync(v.y, y, c->p.m * sizeof(double), hipMemcpyHostToDevice, st));
    LP_HIP(hipMemcpyAsync(v.z, z, c->p.n * sizeof(double), hipMemcpyHostToDevice, st));
    const double tk[2] = {*tau, *kappa};
    LP_HIP(hipMemcpyAsync(v.S + S_TAU, &tk[0], sizeof(double), hipMemcpyHostToDevice, st));
    LP_HIP(hipMemcpyAsync(v.S + S_KAPPA, &tk[1], sizeof(double), hipMemcpyHostToDevice, st));
    LP_TRY(enqueue_residuals(c, 1, ip ? 1 : 0, o->tol));      // r_P, r_D, r_G, mu at the point
    LP_TRY(enqueue_iteration(c, it, ip ? 1 : 0, o));
    double sc[S_COUNT];
    LP_HIP(hipMemcpyAsync(sc, v.S, sizeof(sc), hipMemcpyDeviceToHost, st));
    LP_HIP(hipMemcpyAsync(x, v.x, c->p.n * sizeof(double), hipMemcpyDeviceToHost, st));
    LP_HIP(hipMemcpyAsync(y, v.y, c->p.m * sizeof(double), hipMemcpyDeviceToHost, st));
    LP_HIP(hipMemcpyAsync(z, v.z, c->p.n * sizeof(double), hipMemcpyDeviceToHost, st));
    LP_HIP(hipMemcpyAsync(d_x, v.dx, c->p.n * sizeof(double), hipMemcpyDeviceToHost, st));
    LP_HIP(hipMemcpyAsync(d_y, v.dy, c->p.m * sizeof(double), hipMemcpyDeviceToHost, st));
    LP_HIP(hipMemcpyAsync(d_z, v.dz, c->p.n * sizeof(double), hipMemcpyDeviceToHost, st));
    LP_HIP(hipStreamSynchronize(st));
    if (c->colsplit && c->p.sys[SYS_WORK].res.ngroups() > 0 && *c->rs.timeout_host != 0) {   // as solve_members: a group wait that gave up is an error
        g_err_detail = "a column group of A.D.A^T did not complete within the wait kernel's bound";
        return LPIPM_ERR_HIP;
    }
    *tau = sc[S_TAU]; *kappa = sc[S_KAPPA]; d_tk[0] = sc[S_DTAU]; d_tk[1] = sc[S_DKAPPA]; *alpha_out = sc[S_ALPHA];
    if (info_out) *info_out = c->rs.status_host->potrf_info;
    return LPIPM_OK;
}

extern "C" int lpipm_k_gemv_dual(lpipm_ctx* c, const double* w, const double* v, double* Aw_out, double* ATv_out, int repeats,
                                 double* ms_out) {
    if (!c || !w || !v || !Aw_out || !ATv_out) return LPIPM_ERR_BAD_ARGUMENT;
    if (!c->p.has_problem) return LPIPM_ERR_NO_PROBLEM;
    LP_HIP(hipSetDevice(c->device));
    if (c->p.box) return box_k_passes(c, 1, w, v, true, Aw_out, ATv_out, repeats, ms_out);
    VecArgs& va = c->p.va;
    LP_HIP(hipMemsetAsync(va.W, 0, (size_t)c->p.np * sizeof(double), c->rs.st));
    LP_HIP(hipMemsetAsync(va.R, 0, (size_t)c->p.mp * sizeof(double), c->rs.st));
    LP_HIP(hipMemcpyAsync(va.W, w, c->p.n * sizeof(double), hipMemcpyHostToDevice, c->rs.st));
    LP_HIP(hipMemcpyAsync(va.R, v, c->p.m * sizeof(double), hipMemcpyHostToDevice, c->rs.st));
    const int nch = gemv_dual_chunks(c->p.npa);
    LP_TRY(timed_repeats(c, repeats, ms_out, [&]() -> int {
        LP_HIP(ctx_gemv_dual(c, va.W, va.R, va.Ax, Batch{}));
        return LPIPM_OK;
    }));
    // the consumers' folds, on the host: chunk slabs of A.w, row-block slabs of A^T.v, in index order
    const size_t slab = c->p.tall ? (size_t)c->p.npa : (size_t)c->p.np;      // tall: slabs npa wide, A^T.v of a slack column is v
    std::vector<double> ax((size_t)nch * c->p.mp), at((size_t)c->p.nsplit * slab);
    LP_HIP(hipMemcpyAsync(ax.data(), va.Ax, ax.size() * sizeof(double), hipMemcpyDeviceToHost, c->rs.st));
    LP_HIP(hipMemcpyAsync(at.data(), c->p.ATpart, at.size() * sizeof(double), hipMemcpyDeviceToHost, c->rs.st));
    LP_HIP(hipStreamSynchronize(c->rs.st));
    for (uint64_t i = 0; i < c->p.m; ++i) { double s = 0.0; for (int ch = 0; ch < nch; ++ch) s += ax[(size_t)ch * c->p.mp + i]; Aw_out[i] = s; }
    for (uint64_t j = 0; j < c->p.n; ++j) {
        if (c->p.tall && j >= (uint64_t)c->p.nx) { ATv_out[j] = v[j - (uint64_t)c->p.nx]; continue; }
        double s = 0.0;
        for (int sp = 0; sp < c->p.nsplit; ++sp) s += at[(size_t)sp * slab + j];
        ATv_out[j] = s;
    }
    return LPIPM_OK;
}

extern "C" int lpipm_k_mfma_f64_probe(lpipm_ctx* c, int iters, double* tflops_out, double* ms_out) {
    if (!c || iters < 1) return LPIPM_ERR_BAD_ARGUMENT;
    LP_HIP(hipSetDevice(c->device));
    const int blocks = c->num_cu * 2;
    DeviceTemp tmp{c->rs.st};
    double* sink = nullptr;
    LP_TRY(tmp.take(&sink, (size_t)blocks * 256, false));
    double ms = 0.0;
    LP_TRY(timed_repeats(c, 3, &ms, [&]() -> int { LP_HIP(launch_mfma_probe(iters, sink, blocks, c->rs.st)); return LPIPM_OK; }));
    // per wave and loop trip: 16 independent accumulators x one 16x16x4 MFMA = 16 * 2048 flop
    const double flop = (double)blocks * 4.0 * (double)iters * 16.0 * 2048.0;
    if (ms_out) *ms_out = ms;
    if (tflops_out) *tflops_out = flop / (ms * 1e-3) / 1e12;
    return LPIPM_OK;
}
