// kernels_trsv.hip -- v = L^-T (L^-1 r) with the blocked factor of kernels_potrf.hip
// (replaces `factor.solvec_into(b2)`, newton_equations.rs:151-169; called from sym_solve :221).
//
// A substitution sweep over mp/128 blocks is mp/128 dependent steps, each a tiny launch: latency,
// not bytes.  Instead the factor is consumed through the explicit inverses of its diagonal
// SUPER-blocks (SUPER = 1024 wide; built once per factorisation from the 128-block inverses by
// log2(8) = 3 doubling levels of Inv21 = -Inv22.L21.Inv11 on the MFMA grouped GEMM):
//   forward  (k = 0..nsb-1):  y_k = Inv_k . r_k ;      r_below -= L[below, k] . y_k
//   backward (k = nsb-1..0):  y_k -= L[below, k]^T . v_below ;  v_k = Inv_k^T . y_k
// Every step is a row-split mat-vec over >= 128 workgroups (no serial inner dependency), so a solve
// is ~4*nsb launches that stream the lower triangle of L plus the inverses once each (HBM-bound).
// 1 or 2 right-hand sides per sweep (the predictor's two sym_solve calls share one).
// Reductions are fixed-order: results are bitwise reproducible.
// A coupled plan (FactorPlan::coupled; one large LP that owns its factor) runs the sweeps as launches of row-split pieces
// instead (sweep_kernel), the backward one through H_k = Inv_k^T . L[k+1,k]^T and transposed block columns of L that are
// formed once per factorisation: one launch per backward step (SweepPiece in lpipm_internal.hpp).
#include "lpipm_internal.hpp"

namespace lpipm {

// ------------------------------------------------------------------------------------------------
// plan: storage + static descriptors of the merge GEMMs
double* FactorPlan::blk_inv(int k) const {
    const int r = k * NB;
    for (const SuperBlock& s : sbs)
        if (r >= s.row0 && r < s.row0 + s.size) return s.inv + (size_t)(r - s.row0) * s.size + (r - s.row0);
    return nullptr;
}
double* FactorPlan::blk_invT(int k) const {
    const int r = k * NB;
    for (const SuperBlock& s : sbs)
        if (r >= s.row0 && r < s.row0 + s.size) return s.invT + (size_t)(r - s.row0) * s.size + (r - s.row0);
    return nullptr;
}
int FactorPlan::blk_ld(int k) const {
    const int r = k * NB;
    for (const SuperBlock& s : sbs)
        if (r >= s.row0 && r < s.row0 + s.size) return s.size;
    return 0;
}

namespace {
struct Merge { int sb, lo, mid, hi, level; size_t toff; };   // block indices local to the super-block

// inverse of blocks [lo, hi) from the inverses of [lo, mid) and [mid, hi); returns its level
int plan_merges(int sb, int lo, int hi, std::vector<Merge>& out, size_t& tcursor) {
    if (hi - lo <= 1) return 0;
    int p = 1;
    while (p * 2 < hi - lo) p *= 2;   // left part: largest power of two below the width
    const int mid = lo + p;
    const int l1 = plan_merges(sb, lo, mid, out, tcursor);
    const int l2 = plan_merges(sb, mid, hi, out, tcursor);
    const int lvl = (l1 > l2 ? l1 : l2) + 1;
    out.push_back(Merge{sb, lo, mid, hi, lvl, tcursor});
    tcursor += (size_t)(mid - lo) * NB * (size_t)(hi - mid) * NB;
    return lvl;
}

// first super-block whose block of block column k is kept transposed: the near one only where G of that super-block reads it
int lt_first_sb(int k, int nsb, bool use_g) { return use_g && k + 1 <= nsb - 2 ? k + 1 : k + 2; }
// one past the last such super-block: without H only G's near block is read
int lt_end_sb(int k, int nsb, bool use_h) { return use_h ? nsb : (k + 2 < nsb ? k + 2 : nsb); }

SweepPiece piece1(const double* A, int64_t lda, int rows, int np, int w, bool w_y, double a, int add, bool add_y, int out, bool out_y) {
    SweepPiece p{};
    p.A0 = A; p.lda0 = (int)lda; p.np0 = np; p.rows = rows;
    p.w0 = w; p.w0_y = w_y; p.a0 = a;
    p.add = add; p.add_y = add_y; p.out = out; p.out_y = out_y;
    return p;
}
SweepPiece piece2(SweepPiece p, const double* A1, int lda1, int np1, int w1, bool w1_y, double a1) {
    p.A1 = A1; p.lda1 = lda1; p.np1 = np1; p.w1 = w1; p.w1_y = w1_y; p.a1 = a1;
    return p;
}
SweepPiece tri(SweepPiece p, int t) { p.tri0 = (unsigned char)t; return p; }
SweepLaunch close_launch(std::vector<SweepPiece>& pieces, int first) {
    int blocks = 0;
    for (size_t i = (size_t)first; i < pieces.size(); ++i) { pieces[i].blk0 = blocks; blocks += (pieces[i].rows + 3) / 4; }
    return SweepLaunch{first, (int)pieces.size() - first, blocks};
}

// The launches of the coupled sweep (SweepPiece in lpipm_internal.hpp): R holds r, t and at the end v; Y holds y and s.
void plan_sweep(FactorPlan& plan, const double* L, int64_t ld) {
    const int nsb = (int)plan.sbs.size(), mp = plan.mp;
    std::vector<SweepPiece>& pc = plan.pieces;
    plan.fwd.assign((size_t)nsb, {});
    for (int k = 0; k < nsb && (plan.coupled & COUPLE_G); ++k) {
        const SuperBlock& s = plan.sbs[k];
        const int first = (int)pc.size();
        if (k == 0) {
            pc.push_back(tri(piece1(s.inv, s.size, s.size, s.size, s.row0, false, 1.0, -1, false, s.row0, true), 1));
            plan.fwd[k].push_back(close_launch(pc, first));
            continue;
        }
        const SuperBlock& q = plan.sbs[k - 1];
        if (k == nsb - 1) {   // t_k -= L[k,k-1].y_k-1, then y_k = Inv_k.t_k
            pc.push_back(piece1(L + (size_t)s.row0 * ld + q.row0, ld, s.size, q.size, q.row0, true, -1.0, s.row0, false, s.row0, false));
            plan.fwd[k].push_back(close_launch(pc, first));
            const int second = (int)pc.size();
            pc.push_back(tri(piece1(s.inv, s.size, s.size, s.size, s.row0, false, 1.0, -1, false, s.row0, true), 1));
            plan.fwd[k].push_back(close_launch(pc, second));
            continue;
        }
        pc.push_back(piece2(tri(piece1(s.inv, s.size, s.size, s.size, s.row0, false, 1.0, -1, false, s.row0, true), 1),
                            plan.G[k], q.size, q.size, q.row0, true, -1.0));
        const int below = s.row0 + s.size;    // t_j -= L[j,k-1].y_k-1, every j > k
        pc.push_back(piece1(L + (size_t)below * ld + q.row0, ld, mp - below, q.size, q.row0, true, -1.0, below, false, below, false));
        plan.fwd[k].push_back(close_launch(pc, first));
    }
    // the plain forward recurrence as pieces (two launches per step), where only the backward sweep is coupled
    for (int k = 0; k < nsb && !(plan.coupled & COUPLE_G); ++k) {
        const SuperBlock& s = plan.sbs[k];
        const int first = (int)pc.size(), below = s.row0 + s.size;
        pc.push_back(tri(piece1(s.inv, s.size, s.size, s.size, s.row0, false, 1.0, -1, false, s.row0, true), 1));
        plan.fwd[k].push_back(close_launch(pc, first));
        if (below >= mp) continue;
        const int second = (int)pc.size();    // t_below -= L[below,k].y_k
        pc.push_back(piece1(L + (size_t)below * ld + s.row0, ld, mp - below, s.size, s.row0, true, -1.0, below, false, below, false));
        plan.fwd[k].push_back(close_launch(pc, second));
    }
    plan.bwd.clear();
    for (int k = nsb - 1; k >= 0 && (plan.coupled & COUPLE_H); --k) {
        const SuperBlock& s = plan.sbs[k];
        const int first = (int)pc.size();
        SweepPiece main = tri(piece1(s.invT, s.size, s.size, s.size, s.row0, true, 1.0, -1, false, s.row0, false), 2);
        if (k == nsb - 1) { pc.push_back(main); plan.bwd.push_back(close_launch(pc, first)); continue; }
        const SuperBlock& n = plan.sbs[k + 1];
        pc.push_back(piece2(main, plan.H[k], n.size, n.size, n.row0, false, -1.0));
        for (int i = 0; i < k; ++i) {         // s_i -= L[k+1,i]^T.v_k+1
            const CoupleStep& c = plan.couple[i];
            pc.push_back(piece1(c.lt + (n.row0 - c.lt_row0), c.lt_ld, plan.sbs[i].size, n.size, n.row0, false, -1.0,
                                plan.sbs[i].row0, true, plan.sbs[i].row0, true));
        }
        plan.bwd.push_back(close_launch(pc, first));
    }
}
}  // namespace

size_t factor_coupling_bytes(int mp, int super_w, int coupled) {
    const int nsb = (mp + super_w - 1) / super_w;
    if (nsb < 2 || !coupled) return 0;
    const bool use_h = coupled & COUPLE_H, use_g = coupled & COUPLE_G;
    auto width = [&](int k) { return (size_t)(mp - k * super_w < super_w ? mp - k * super_w : super_w); };
    size_t doubles = 0;
    for (int k = 0; k < nsb; ++k) {
        if (use_h && k < nsb - 1) doubles += width(k) * width(k + 1);
        if (use_g && k >= 1 && k <= nsb - 2) doubles += width(k) * width(k - 1);
        const int j = lt_first_sb(k, nsb, use_g), j1 = lt_end_sb(k, nsb, use_h);
        if (j < j1) doubles += width(k) * (size_t)((j1 < nsb ? j1 * super_w : mp) - j * super_w);
    }
    return doubles * sizeof(double);
}

hipError_t factor_plan_create(FactorPlan& plan, double* L, int64_t ld, int mp, Arena& arena, bool build,
                              hipStream_t st, int super_w, int merge_edge, const FactorPlan* scratch_of, int coupled,
                              int couple_edge) {
    factor_plan_destroy(plan);
    plan.L = L; plan.ld = ld; plan.mp = mp;
    plan.super_w = super_w;
    plan.merge_edge = (merge_edge == 64 || merge_edge == 32) ? merge_edge : 128;
    const int E = plan.merge_edge, SUB = NB / E, EK = E / BK;   // sub-tiles per 128-block edge, k-tiles per sub-tile edge
    hipError_t e;
    for (int r0 = 0; r0 < mp; r0 += super_w) {
        SuperBlock s{};
        s.row0 = r0;
        s.size = mp - r0 < super_w ? mp - r0 : super_w;
        s.inv = arena.take<double>((size_t)s.size * s.size);
        s.invT = arena.take<double>((size_t)s.size * s.size);
        plan.sbs.push_back(s);
    }
    std::vector<Merge> merges;
    size_t tcursor = 0;
    int maxlvl = 0;
    for (size_t i = 0; i < plan.sbs.size(); ++i) {
        const int lvl = plan_merges((int)i, 0, plan.sbs[i].size / NB, merges, tcursor);
        if (lvl > maxlvl) maxlvl = lvl;
    }
    double* tws = scratch_of ? scratch_of->tws : arena.take<double>(tcursor);
    plan.tws = tws;
    // slabs of the backward sweep's transposed panel products: (rows below / 128) x 2 rhs x SUPER
    plan.tpart = scratch_of ? scratch_of->tpart : arena.take<double>((size_t)(mp / GEMVT_ROWS + 1) * 2 * super_w);
    // the coupled sweep: H_k, G_k and the transposed block columns, every one written whole by launch_couple_step
    const int nsb = (int)plan.sbs.size();
    plan.coupled = nsb >= 2 ? coupled & (COUPLE_H | COUPLE_G) : 0;
    plan.couple_edge = (couple_edge == 128 || couple_edge == 64) ? couple_edge : 32;
    if (plan.coupled) {
        const bool use_h = plan.coupled & COUPLE_H, use_g = plan.coupled & COUPLE_G;
        plan.H.assign((size_t)nsb, nullptr);
        plan.G.assign((size_t)nsb, nullptr);
        plan.couple.assign((size_t)nsb, CoupleStep{});
        for (int k = 0; k < nsb; ++k) {
            const SuperBlock& s = plan.sbs[k];
            if (use_h && k < nsb - 1) plan.H[k] = arena.take<double>((size_t)s.size * plan.sbs[k + 1].size);
            if (use_g && k >= 1 && k <= nsb - 2) plan.G[k] = arena.take<double>((size_t)s.size * plan.sbs[k - 1].size);
            const int j = lt_first_sb(k, nsb, use_g), j1 = lt_end_sb(k, nsb, use_h);
            if (j < j1) {
                CoupleStep& c = plan.couple[k];
                c.lt_row0 = plan.sbs[j].row0;
                c.lt_ld = (j1 < nsb ? plan.sbs[j1].row0 : mp) - c.lt_row0;
                c.lt = arena.take<double>((size_t)s.size * c.lt_ld);
            }
        }
        plan_sweep(plan, L, ld);
    }
    if (!build) return hipSuccess;

    std::vector<GemmTileDesc> descs;
    plan.stages.clear();
    plan.groups.clear();
    // a stage's descriptors stay in merge order -- super-block by super-block, left to right, so the chain step after which
    // a merge's inputs are final (block hi - 1 of its super-block) never decreases along a stage -- and the stage is cut
    // where the outer panel of that step changes
    auto count_in_group = [&](const Merge& m) {
        const int panel = (plan.sbs[m.sb].row0 / NB + m.hi - 1) / POTRF_OUTER, stage = (int)plan.stages.size();
        if (plan.groups.empty() || plan.groups.back().stage != stage || plan.groups.back().panel != panel)
            plan.groups.push_back(MergeGroup{(int)descs.size(), 0, stage, panel});
        return &plan.groups.back();
    };
    const int KPB = NB / BK;   // k-tiles per 128-block
    for (int lvl = 1; lvl <= maxlvl; ++lvl) {
        // stage A: T^T (s1 x s2) = Inv11^T . L21^T ; Inv11^T is upper triangular: k >= row tile
        const int a0 = (int)descs.size();
        for (const Merge& m : merges) {
            if (m.level != lvl) continue;
            const SuperBlock& s = plan.sbs[m.sb];
            const int n1 = m.mid - m.lo, n2 = m.hi - m.mid;
            MergeGroup* grp = count_in_group(m);
            grp->count += (n1 * SUB) * (n2 * SUB);
            for (int tj = 0; tj < n1 * SUB; ++tj)           // sub-tile indices: rows of T^T, columns of T^T
                for (int ti = 0; ti < n2 * SUB; ++ti) {
                    GemmTileDesc d{};
                    d.P = s.invT + (size_t)(m.lo * NB + tj * E) * s.size + m.lo * NB;
                    d.ldp = s.size;
                    d.Q = L + (size_t)(s.row0 + m.mid * NB + ti * E) * ld + s.row0 + m.lo * NB;
                    d.ldq = (int)ld;
                    d.C = tws + m.toff + (size_t)(tj * E) * (n2 * NB) + ti * E;
                    d.ldc = n2 * NB;
                    d.kt_begin = tj * EK;                   // Inv11^T is upper triangular: k >= row
                    d.kt_end = n1 * KPB;
                    d.alpha = 1.0;
                    descs.push_back(d);
                }
        }
        plan.stages.push_back({a0, (int)descs.size() - a0});
        // stage B: Inv21 (s2 x s1) = -Inv22 . T  and its transpose (s1 x s2) = -T^T . Inv22^T ;
        // Inv22 is lower triangular: k <= row tile of Inv22
        const int b0 = (int)descs.size();
        for (const Merge& m : merges) {
            if (m.level != lvl) continue;
            const SuperBlock& s = plan.sbs[m.sb];
            const int n1 = m.mid - m.lo, n2 = m.hi - m.mid;
            double* TT = tws + m.toff;
            MergeGroup* grp = count_in_group(m);
            grp->count += 2 * (n1 * SUB) * (n2 * SUB);
            for (int ti = 0; ti < n2 * SUB; ++ti)
                for (int tj = 0; tj < n1 * SUB; ++tj) {
                    GemmTileDesc d{};   // Inv21(ti,tj) = -sum_k Inv22[ti][k] T^T[tj][k]
                    d.P = s.inv + (size_t)(m.mid * NB + ti * E) * s.size + m.mid * NB;
                    d.ldp = s.size;
                    d.Q = TT + (size_t)(tj * E) * (n2 * NB);
                    d.ldq = n2 * NB;
                    d.C = s.inv + (size_t)(m.mid * NB + ti * E) * s.size + (m.lo * NB + tj * E);
                    d.ldc = s.size;
                    d.kt_begin = 0;
                    d.kt_end = (ti + 1) * EK;               // Inv22 is lower triangular: k <= row
                    d.alpha = -1.0;
                    descs.push_back(d);
                    GemmTileDesc t{};   // Inv21^T(tj,ti) = -sum_k T^T[tj][k] Inv22[ti][k]
                    t.P = TT + (size_t)(tj * E) * (n2 * NB);
                    t.ldp = n2 * NB;
                    t.Q = s.inv + (size_t)(m.mid * NB + ti * E) * s.size + m.mid * NB;
                    t.ldq = s.size;
                    t.C = s.invT + (size_t)(m.lo * NB + tj * E) * s.size + (m.mid * NB + ti * E);
                    t.ldc = s.size;
                    t.kt_begin = 0;
                    t.kt_end = (ti + 1) * EK;
                    t.alpha = -1.0;
                    descs.push_back(t);
                }
        }
        plan.stages.push_back({b0, (int)descs.size() - b0});
    }
    if (plan.coupled) {
        // behind the merges: per super-block one group, H_k = Inv_k^T . L[k+1,k]^T (stage A's form: Inv_k^T is upper
        // triangular, k >= row) and G_k = Inv_k . L[k,k-1] (Inv_k is lower triangular, k <= row; its second operand is the
        // transposed copy in block column k-1's buffer), on COUPLE_EDGE tiles
        const int E2 = plan.couple_edge, EK2 = E2 / BK;
        for (int k = 0; k < nsb; ++k) {
            const SuperBlock& s = plan.sbs[k];
            CoupleStep& c = plan.couple[k];
            c.first = (int)descs.size();
            if (plan.H[k]) {
                const SuperBlock& n = plan.sbs[k + 1];
                for (int ti = 0; ti < s.size / E2; ++ti)
                    for (int tj = 0; tj < n.size / E2; ++tj) {
                        GemmTileDesc d{};
                        d.P = s.invT + (size_t)(ti * E2) * s.size; d.ldp = s.size;
                        d.Q = L + (size_t)(n.row0 + tj * E2) * ld + s.row0; d.ldq = (int)ld;
                        d.C = plan.H[k] + (size_t)(ti * E2) * n.size + tj * E2; d.ldc = n.size;
                        d.kt_begin = ti * EK2; d.kt_end = s.size / BK; d.alpha = 1.0;
                        descs.push_back(d);
                    }
            }
            if (plan.G[k]) {
                const SuperBlock& q = plan.sbs[k - 1];
                const CoupleStep& cq = plan.couple[k - 1];
                for (int ti = s.size / E2 - 1; ti >= 0; --ti)     // (longest k-ranges first)
                    for (int tj = 0; tj < q.size / E2; ++tj) {
                        GemmTileDesc d{};
                        d.P = s.inv + (size_t)(ti * E2) * s.size; d.ldp = s.size;
                        d.Q = cq.lt + (size_t)(tj * E2) * cq.lt_ld + (s.row0 - cq.lt_row0); d.ldq = cq.lt_ld;
                        d.C = plan.G[k] + (size_t)(ti * E2) * q.size + tj * E2; d.ldc = q.size;
                        d.kt_begin = 0; d.kt_end = (ti + 1) * EK2; d.alpha = 1.0;
                        descs.push_back(d);
                    }
            }
            c.count = (int)descs.size() - c.first;
        }
        if ((e = hipMalloc((void**)&plan.pieces_dev, plan.pieces.size() * sizeof(SweepPiece))) != hipSuccess) return e;
        e = hipMemcpyAsync(plan.pieces_dev, plan.pieces.data(), plan.pieces.size() * sizeof(SweepPiece), hipMemcpyHostToDevice, st);
        if (e != hipSuccess) return e;
    }
    // (one allocation: the descriptors, then the hand-off words of the pipelined chain step -- 8 words x 4 B per 128-block)
    const size_t desc_bytes = round_up((descs.size() + 1) * sizeof(GemmTileDesc), 16), flag_bytes = (size_t)(mp / NB) * 8 * sizeof(unsigned int);
    if ((e = hipMalloc((void**)&plan.descs_dev, desc_bytes + flag_bytes)) != hipSuccess) return e;
    plan.pipe_flags = (unsigned int*)((char*)plan.descs_dev + desc_bytes);
    if ((e = hipMemsetAsync(plan.pipe_flags, 0, flag_bytes, st)) != hipSuccess) return e;
    if (!descs.empty()) {
        e = hipMemcpyAsync(plan.descs_dev, descs.data(), descs.size() * sizeof(GemmTileDesc), hipMemcpyHostToDevice, st);
        if (e != hipSuccess) return e;
    }
    return hipStreamSynchronize(st);   // `descs` must outlive the copy
}

void factor_plan_destroy(FactorPlan& plan) {
    if (plan.descs_dev) (void)hipFree(plan.descs_dev);   // the inverse storage belongs to the arena
    plan.sbs.clear();
    plan.stages.clear();
    plan.groups.clear();
    if (plan.pieces_dev) (void)hipFree(plan.pieces_dev);
    plan.coupled = 0;
    plan.H.clear(); plan.G.clear(); plan.couple.clear(); plan.pieces.clear(); plan.fwd.clear(); plan.bwd.clear();
    plan.pieces_dev = nullptr;
    plan.descs_dev = nullptr;
    plan.pipe_flags = nullptr;
    plan.tpart = nullptr;
    plan.tws = nullptr;
    plan.L = nullptr; plan.ld = 0; plan.mp = 0;
}

// ------------------------------------------------------------------------------------------------
// y[q][c] -= sum_s part[s][q][c]   (c < width): folds the row-split slabs of the transposed panel
// product into the right-hand side of the backward step, in slab order.
__global__ __launch_bounds__(256) void trsv_fold_kernel(double* __restrict__ y, long long ldy,
                                                        const double* __restrict__ part, int nsplit, int nrhs,
                                                        int width, BatchK bk) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= width || batch_done(bk)) return;
    y = batch_ptr(y, bk); part = batch_ptr(part, bk);
    for (int q = 0; q < nrhs; ++q) {
        // eight slab values are requested before any is added (one memory round trip per eight instead of per
        // value); the additions stay in slab order
        double s = 0.0;
        int sp = 0;
        for (; sp + 8 <= nsplit; sp += 8) {
            double v[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) v[u] = part[((long long)(sp + u) * nrhs + q) * width + c];
#pragma unroll
            for (int u = 0; u < 8; ++u) s += v[u];
        }
        for (; sp < nsplit; ++sp) s += part[((long long)sp * nrhs + q) * width + c];
        y[(long long)q * ldy + c] -= s;
    }
}

// ------------------------------------------------------------------------------------------------
// the coupled sweep
// T[c][r] = L[r][c] for r < 32 gridDim.x, c < 32 gridDim.y (both exact multiples of 32: blocks of 128)
__global__ __launch_bounds__(256) void transpose_block_kernel(const double* __restrict__ L, long long ld, double* __restrict__ T,
                                                              long long ldt) {
    __shared__ double tile[32][33];
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    const long long r0 = (long long)blockIdx.x * 32, c0 = (long long)blockIdx.y * 32;
#pragma unroll
    for (int i = 0; i < 4; ++i) tile[ty + 8 * i][tx] = L[(r0 + ty + 8 * i) * ld + c0 + tx];
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 4; ++i) T[(c0 + ty + 8 * i) * ldt + r0 + tx] = tile[tx][ty + 8 * i];
}

hipError_t launch_couple_step(const FactorPlan& plan, int k, hipStream_t st) {
    if (!plan.coupled) return hipSuccess;
    const double* L = plan.L; const int64_t ld = plan.ld;
    const CoupleStep& c = plan.couple[(size_t)k];
    const SuperBlock& s = plan.sbs[(size_t)k];
    if (c.lt) {
        hipLaunchKernelGGL(transpose_block_kernel, dim3(c.lt_ld / 32, s.size / 32), dim3(256), 0, st,
                           L + (size_t)c.lt_row0 * ld + s.row0, (long long)ld, c.lt, (long long)c.lt_ld);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return launch_gemm_grouped(plan.descs_dev + c.first, c.count, st, Batch{}, plan.couple_edge);
}

typedef double sweep_d2 __attribute__((ext_vector_type(2)));

// acc[q] += sum over this lane's columns k = k0 + 2 lane + 128 j < k1 of a[k] w[q][k], in ascending k.  The loads of U strides
// are issued before any of them is used (a wave's row is 4 to 16 strides: one memory round trip instead of one per stride);
// the additions keep their order.
template <int NRHS, int U>
__device__ __forceinline__ void sweep_dot_strides(const double* a, const double* w, long long ldv, int& k, int k1, double (&acc)[NRHS]) {
    for (; k + 128 * (U - 1) < k1; k += 128 * U) {
        sweep_d2 av[U], wv[U][NRHS];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            av[u] = *(const sweep_d2*)(a + k + 128 * u);
#pragma unroll
            for (int q = 0; q < NRHS; ++q) wv[u][q] = *(const sweep_d2*)(w + (long long)q * ldv + k + 128 * u);
        }
#pragma unroll
        for (int u = 0; u < U; ++u)
#pragma unroll
            for (int q = 0; q < NRHS; ++q) acc[q] += av[u][0] * wv[u][q][0] + av[u][1] * wv[u][q][1];
    }
}
template <int NRHS>
__device__ __forceinline__ void sweep_dot(const double* a, const double* w, long long ldv, int k0, int k1, int lane, double (&acc)[NRHS]) {
    int k = k0 + 2 * lane;
    sweep_dot_strides<NRHS, 8>(a, w, ldv, k, k1, acc);
    sweep_dot_strides<NRHS, 4>(a, w, ldv, k, k1, acc);
    sweep_dot_strides<NRHS, 1>(a, w, ldv, k, k1, acc);
}

// One launch of the coupled sweep: workgroup b belongs to the piece whose [blk0, next blk0) holds it; a wave owns one row of
// its piece and sums each term as gemv_n does (lanes stride the row by 128, then the butterfly).  tri0: the first term's
// matrix is a triangular inverse whose other half is exact zeros (1: lower, 2: upper): row i then reads the 128-blocks up to
// (from) its diagonal one only.
template <int NRHS>
__global__ __launch_bounds__(256) void sweep_kernel(const SweepPiece* __restrict__ pieces, int npieces, double* R, double* Y,
                                                    long long ldv, const int* done) {
    if (done && *done != 0) return;
    int p = 0;
    while (p + 1 < npieces && (int)blockIdx.x >= pieces[p + 1].blk0) ++p;
    const SweepPiece d = pieces[p];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int row = ((int)blockIdx.x - d.blk0) * 4 + wave;
    if (row >= d.rows) return;
    double acc0[NRHS], acc1[NRHS];
#pragma unroll
    for (int q = 0; q < NRHS; ++q) acc0[q] = acc1[q] = 0.0;
    const int k0 = d.tri0 == 2 ? (row & ~127) : 0, k1 = d.tri0 == 1 ? (row | 127) + 1 : d.np0;
    sweep_dot<NRHS>(d.A0 + (long long)row * d.lda0, (d.w0_y ? Y : R) + d.w0, ldv, k0, k1, lane, acc0);
    if (d.A1) sweep_dot<NRHS>(d.A1 + (long long)row * d.lda1, (d.w1_y ? Y : R) + d.w1, ldv, 0, d.np1, lane, acc1);
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1)
#pragma unroll
        for (int q = 0; q < NRHS; ++q) {
            acc0[q] += __shfl_xor(acc0[q], off, 64);
            acc1[q] += __shfl_xor(acc1[q], off, 64);
        }
    if (lane == 0) {
        const double* add = d.add >= 0 ? (d.add_y ? Y : R) + d.add : nullptr;
        double* out = (d.out_y ? Y : R) + d.out;
#pragma unroll
        for (int q = 0; q < NRHS; ++q) {
            double v = (add ? add[(long long)q * ldv + row] : 0.0) + d.a0 * acc0[q];
            if (d.A1) v += d.a1 * acc1[q];
            out[(long long)q * ldv + row] = v;
        }
    }
}

static hipError_t launch_sweep(const FactorPlan& plan, const SweepLaunch& l, int nrhs, double* R, double* Y, hipStream_t st,
                               const int* done) {
    if (nrhs == 1) hipLaunchKernelGGL(sweep_kernel<1>, dim3(l.blocks), dim3(256), 0, st, plan.pieces_dev + l.first, l.count, R, Y, (long long)plan.mp, done);
    else           hipLaunchKernelGGL(sweep_kernel<2>, dim3(l.blocks), dim3(256), 0, st, plan.pieces_dev + l.first, l.count, R, Y, (long long)plan.mp, done);
    return hipGetLastError();
}

hipError_t launch_chol_solve(const FactorPlan& plan, int nrhs, double* R, double* Y, hipStream_t st, const Batch& bt, const SolveSteps& steps, bool shared_factor) {
    // a coupled plan: one LP that owns its factor (the rule of the callers: a function of the shape alone).  Either sweep may
    // be the coupled one; both leave y in Y and take v to R, and the steps keep their meaning.
    if (plan.coupled && (bt.count != 1 || bt.first != 0 || shared_factor)) return hipErrorInvalidValue;
    // shared_factor: L, inv and invT are ONE factor for the whole batch and get no member offset; every mat-vec of the sweep
    // then runs as the shared-matrix group template (a block of the factor is read once per group of members).  R, Y and
    // the slabs stay per member, and a member's sums are those of the group of one.
    const double* L = plan.L; const int64_t ld = plan.ld;
    const int mp = plan.mp;
    hipError_t e;
    const int nsb = (int)plan.sbs.size();
    const int k1 = steps.fwd_end < 0 || steps.fwd_end > nsb ? nsb : steps.fwd_end;
    // forward: L y = r
    if (plan.coupled) {   // (without G: the plain recurrence, as pieces of the sweep kernel)
        for (int k = steps.fwd_begin; k < k1; ++k)
            for (const SweepLaunch& l : plan.fwd[(size_t)k])
                if ((e = launch_sweep(plan, l, nrhs, R, Y, st, bt.done)) != hipSuccess) return e;
    } else
    for (int k = steps.fwd_begin; k < k1; ++k) {
        const SuperBlock& s = plan.sbs[k];
        e = launch_gemv_n(s.inv, s.size, s.size, s.size, nrhs, R + s.row0, mp, nullptr, nullptr, Y + s.row0, mp, st, 1.0, bt, shared_factor);
        if (e != hipSuccess) return e;
        const int below = mp - (s.row0 + s.size);
        if (below > 0) {
            double* rb = R + s.row0 + s.size;
            e = launch_gemv_n(L + (size_t)(s.row0 + s.size) * ld + s.row0, ld, below, s.size, nrhs, Y + s.row0, mp, rb,
                              rb + mp, rb, mp, st, -1.0, bt, shared_factor);
            if (e != hipSuccess) return e;
        }
    }
    if (!steps.backward) return hipSuccess;
    if (plan.coupled & COUPLE_H) {
        for (const SweepLaunch& l : plan.bwd)
            if ((e = launch_sweep(plan, l, nrhs, R, Y, st, bt.done)) != hipSuccess) return e;
        return hipSuccess;
    }
    // backward: L^T v = y   (solution written over R)
    for (int k = nsb - 1; k >= 0; --k) {
        const SuperBlock& s = plan.sbs[k];
        const int below = mp - (s.row0 + s.size);
        if (below > 0) {
            e = launch_gemv_t(L + (size_t)(s.row0 + s.size) * ld + s.row0, ld, below, s.size, nrhs,
                              R + s.row0 + s.size, mp, plan.tpart, st, 0, bt, shared_factor);
            if (e != hipSuccess) return e;
            hipLaunchKernelGGL(trsv_fold_kernel, dim3((s.size + 255) / 256, 1, bt.count), dim3(256), 0, st, Y + s.row0,
                               (long long)mp, plan.tpart, below / GEMVT_ROWS, nrhs, s.size, batch_k(bt));
            if ((e = hipGetLastError()) != hipSuccess) return e;
        }
        e = launch_gemv_n(s.invT, s.size, s.size, s.size, nrhs, Y + s.row0, mp, nullptr, nullptr, R + s.row0, mp, st, 1.0, bt, shared_factor);
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

}  // namespace lpipm
