// Host-logic exerciser for an AddressSanitizer / UBSan build of liblpipm.so (scripts/diag/host_asan.sh): uploads of
// changing geometry, single solves, lockstep batches, a mixed-shape lpipm_solve_batch (grouping, chunk pipeline, worker
// threads), the ub/eq upload, error paths.  Exit code 0 = all answers as expected and no sanitizer report.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include <unistd.h>
#include "lpipm.h"

struct LP { uint64_t m, n; std::vector<double> A, b, c, xs; };
static LP make(uint64_t seed, uint64_t m, uint64_t n) {
    LP p{m, n, std::vector<double>(m * n), std::vector<double>(m), std::vector<double>(n), std::vector<double>(n)};
    if (lpipm_synth_planted_lp(seed, m, n, p.A.data(), p.b.data(), p.c.data(), p.xs.data()) != 0) { printf("synth failed\n"); exit(2); }
    return p;
}
static double maxerr(const std::vector<double>& x, const std::vector<double>& y) {
    double e = 0; for (size_t i = 0; i < x.size(); ++i) e = std::fmax(e, std::fabs(x[i] - y[i])); return e;
}
#define CHECK(cond) do { if (!(cond)) { printf("FAILED %s:%d: %s (%s)\n", __FILE__, __LINE__, #cond, lpipm_last_error_detail()); fflush(stdout); _exit(1); } } while (0)

int main() {
    lpipm_ctx* ctx = nullptr;
    CHECK(lpipm_create(0, &ctx) == 0);
    lpipm_opts o; lpipm_default_opts(&o);
    // single solves, geometry changing up and down
    for (auto mn : {std::pair<uint64_t, uint64_t>{64, 160}, {300, 700}, {1, 1}, {129, 130}, {64, 160}}) {
        LP p = make(mn.first + mn.second, mn.first, mn.second);
        CHECK(lpipm_upload(ctx, p.m, p.n, p.A.data(), p.n, p.b.data(), p.c.data(), 0.0) == 0);
        std::vector<double> x(p.n); double fun; uint64_t it;
        std::vector<lpipm_iter_row> log(o.max_iter);
        CHECK(lpipm_solve(ctx, &o, x.data(), &fun, &it, log.data()) == 0);
        CHECK(maxerr(x, p.xs) < 1e-5);
    }
    // lockstep batch + mixed-shape batch (groups of equal shape, an odd one, chunks of 3 -> pipeline over two contexts)
    std::vector<LP> lps;
    for (int s = 0; s < 7; ++s) lps.push_back(make(s, 96, 200));
    lps.push_back(make(77, 40, 100));
    for (int s = 0; s < 3; ++s) lps.push_back(make(20 + s, 130, 300));
    const size_t K = lps.size();
    std::vector<uint64_t> m(K), n(K), its(K);
    std::vector<const double*> A(K), b(K), c(K);
    std::vector<std::vector<double>> xs(K);
    std::vector<double*> xp(K);
    std::vector<double> fun(K);
    std::vector<int32_t> st(K);
    for (size_t i = 0; i < K; ++i) { m[i] = lps[i].m; n[i] = lps[i].n; A[i] = lps[i].A.data(); b[i] = lps[i].b.data(); c[i] = lps[i].c.data(); xs[i].resize(n[i]); xp[i] = xs[i].data(); }
    for (int mode : {-1, 3, 0}) {
        CHECK(lpipm_set_batch_lockstep(ctx, mode) == 0);
        CHECK(lpipm_solve_batch(ctx, K, m.data(), n.data(), A.data(), b.data(), c.data(), nullptr, &o, xp.data(), fun.data(), its.data(), st.data()) == 0);
        for (size_t i = 0; i < K; ++i) { CHECK(st[i] == 0); CHECK(maxerr(xs[i], lps[i].xs) < 1e-5); }
    }
    CHECK(lpipm_upload_lockstep(ctx, 7, 96, 200, A.data(), b.data(), c.data(), nullptr) == 0);
    CHECK(lpipm_solve_lockstep(ctx, &o, xp.data(), fun.data(), its.data(), st.data()) == 0);
    for (int i = 0; i < 7; ++i) CHECK(st[i] == 0);
    // a lockstep batch large enough for the two half-batch views (two host threads, shared arenas), then a smaller one again
    // (the views are torn down at the upload), then the large one twice in a row (views reused)
    {
        std::vector<LP> big;
        for (int s = 0; s < 18; ++s) big.push_back(make(100 + s, 96, 200));
        std::vector<const double*> A2(18), b2(18), c2v(18);
        std::vector<std::vector<double>> x2(18, std::vector<double>(200));
        std::vector<double*> xp2(18);
        std::vector<double> fun2(18); std::vector<uint64_t> its2(18); std::vector<int32_t> st2(18);
        for (int i = 0; i < 18; ++i) { A2[i] = big[i].A.data(); b2[i] = big[i].b.data(); c2v[i] = big[i].c.data(); xp2[i] = x2[i].data(); }
        for (int round = 0; round < 2; ++round) {
            CHECK(lpipm_upload_lockstep(ctx, 18, 96, 200, A2.data(), b2.data(), c2v.data(), nullptr) == 0);
            for (int rep = 0; rep < 2; ++rep) {
                CHECK(lpipm_solve_lockstep(ctx, &o, xp2.data(), fun2.data(), its2.data(), st2.data()) == 0);
                for (int i = 0; i < 18; ++i) { CHECK(st2[i] == 0); CHECK(maxerr(x2[i], big[i].xs) < 1e-5); }
            }
            CHECK(lpipm_upload_lockstep(ctx, 7, 96, 200, A.data(), b.data(), c.data(), nullptr) == 0);
            CHECK(lpipm_solve_lockstep(ctx, &o, xp.data(), fun.data(), its.data(), st.data()) == 0);
        }
    }
    // InteriorPoint<f32> (generic kernels; upload + solve + release inside the call) and its double twin
    {
        LP p = make(5, 70, 150);
        std::vector<float> Af(p.A.begin(), p.A.end()), bf(p.b.begin(), p.b.end()), cf(p.c.begin(), p.c.end()), xf(p.n);
        lpipm_opts of = o; of.tol = 1e-3;
        float funf; uint64_t itf;
        std::vector<lpipm_iter_row_f32> logf(of.max_iter);
        CHECK(lpipm_solve_f32(ctx, p.m, p.n, Af.data(), p.n, bf.data(), cf.data(), 0.0f, &of, xf.data(), &funf, &itf, logf.data()) == 0);
        double e = 0; for (size_t i = 0; i < p.n; ++i) e = std::fmax(e, std::fabs((double)xf[i] - p.xs[i]));
        CHECK(e < 5e-2);
        std::vector<double> xd(p.n); double fund; uint64_t itd;
        CHECK(lpipm_k_generic_solve_f64(ctx, p.m, p.n, p.A.data(), p.n, p.b.data(), p.c.data(), 0.0, &o, xd.data(), &fund, &itd, nullptr) == 0);
        CHECK(maxerr(xd, p.xs) < 1e-5);
        of.alpha0 = 2.0;
        CHECK(lpipm_solve_f32(ctx, p.m, p.n, Af.data(), p.n, bf.data(), cf.data(), 0.0f, &of, xf.data(), &funf, &itf, nullptr) == LPIPM_INVALID_PARAMETER);
    }
    // ub / eq upload (README LP: known answer [1, 0])
    const double c2[2] = {-1, 4}, Aub[4] = {-3, 1, 1, 2}, bub[2] = {6, 4}, Aeq[2] = {1, 1}, beq[1] = {1};
    CHECK(lpipm_upload_ub_eq(ctx, 2, 2, Aub, 2, bub, 1, Aeq, 2, beq, c2, 0.0) == 0);
    double x4[4], f4; uint64_t it4;
    CHECK(lpipm_solve(ctx, &o, x4, &f4, &it4, nullptr) == 0);
    CHECK(std::fabs(x4[0] - 1.0) < 1e-6 && std::fabs(x4[1]) < 1e-6);
    // error paths
    CHECK(lpipm_upload_ub_eq(ctx, 2, 0, nullptr, 0, nullptr, 0, nullptr, 0, nullptr, c2, 0.0) == LPIPM_UNCONSTRAINED);
    lpipm_opts bad = o; bad.alpha0 = 2.0;
    CHECK(lpipm_solve(ctx, &bad, x4, &f4, &it4, nullptr) == LPIPM_INVALID_PARAMETER);
    const double Ainf[4] = {1, 1, 1, 1}, binf[1] = {-1}, cinf[4] = {1, 1, 1, 1};
    CHECK(lpipm_upload(ctx, 1, 4, Ainf, 4, binf, cinf, 0.0) == 0);
    CHECK(lpipm_solve(ctx, &o, x4, &f4, &it4, nullptr) == LPIPM_INFEASIBLE);
    // round-2 entry points: one-iteration hook, one-read dual pass, symmetric residual
    {
        LP p = make(5, 100, 333);
        CHECK(lpipm_upload(ctx, p.m, p.n, p.A.data(), p.n, p.b.data(), p.c.data(), 0.0) == 0);
        std::vector<double> x(p.n, 1.5), y(p.m, 0.1), z(p.n, 0.7), dx(p.n), dy(p.m), dz(p.n), aw(p.m), atv(p.n);
        double tau = 1.2, kappa = 0.8, dtk[2], alpha; int32_t info = -1; double ms;
        CHECK(lpipm_k_iteration(ctx, &o, 0, x.data(), y.data(), z.data(), &tau, &kappa, dx.data(), dy.data(), dz.data(), dtk, &alpha, &info) == 0);
        CHECK(info == 0 && alpha > 0.0 && alpha <= 1.0);
        CHECK(lpipm_k_gemv_dual(ctx, x.data(), y.data(), aw.data(), atv.data(), 2, &ms) == 0);
        const uint64_t ms_ = 200;
        std::vector<double> S(ms_ * ms_), V(2 * ms_, 1.0), R0(2 * ms_, 0.5), Rho(2 * ms_);
        for (uint64_t i = 0; i < ms_; ++i) for (uint64_t j = 0; j <= i; ++j) S[i * ms_ + j] = 1.0 / (1.0 + i + j);
        CHECK(lpipm_k_symv_residual(ctx, ms_, S.data(), 2, V.data(), R0.data(), Rho.data()) == 0);
    }
    lpipm_destroy(ctx);
    // refined solves (LPIPM_REFINE=2): decided when a context is created
    setenv("LPIPM_EXPERIMENTAL", "1", 1);     // the library reads its measurement knobs only with the master switch on
    setenv("LPIPM_REFINE", "2", 1);
    {
        lpipm_ctx* c2 = nullptr;
        CHECK(lpipm_create(0, &c2) == 0);
        LP p = make(9, 300, 700);
        CHECK(lpipm_upload(c2, p.m, p.n, p.A.data(), p.n, p.b.data(), p.c.data(), 0.0) == 0);
        std::vector<double> x(p.n); double fun; uint64_t it;
        CHECK(lpipm_solve(c2, &o, x.data(), &fun, &it, nullptr) == 0);
        CHECK(maxerr(x, p.xs) < 1e-5);
        LP q = make(3, 2048, 2304);
        CHECK(lpipm_upload(c2, q.m, q.n, q.A.data(), q.n, q.b.data(), q.c.data(), 0.0) == 0);
        std::vector<double> xq(q.n);
        CHECK(lpipm_solve(c2, &o, xq.data(), &fun, &it, nullptr) == 0);
        CHECK(maxerr(xq, q.xs) < 1e-4);
        CHECK(lpipm_upload(c2, p.m, p.n, p.A.data(), p.n, p.b.data(), p.c.data(), 0.0) == 0);   // back to a small geometry
        CHECK(lpipm_solve(c2, &o, x.data(), &fun, &it, nullptr) == 0);
        lpipm_destroy(c2);
    }
    printf("host exerciser ok\n");
    fflush(stdout);
    _exit(0);   // skip the HSA runtime's exit-time teardown: under ASan it trips a CHECK of the sanitizer's own device
                // allocator ("dev_runtime_unloaded_"), which is not this library's code
}
