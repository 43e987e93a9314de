// test_ripped_tall_eq.cpp -- InteriorPoint::tall_eq_form() of include/ripped.hpp, through liblpipm.so on device 0: the
// README LP (two `ub` rows, one `eq` row; src/lib.rs:84-96) goes through lpipm_upload_ub_eq_tall and comes back with the known
// answer and the ordinary path's iteration count; tall_form() alone keeps taking the ordinary path for a problem with `eq` rows;
// a pure-`ub` problem under tall_eq_form() is the tall form itself.
#include <cmath>
#include <cstdio>
#include <vector>

#include "ripped.hpp"

using namespace ripped;

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond); ++failures; } } while (0)

static bool close(const std::vector<double>& a, const std::vector<double>& b, double eps) {
    if (a.size() != b.size()) return false;
    for (size_t i = 0; i < a.size(); ++i)
        if (!(std::fabs(a[i] - b[i]) <= eps)) return false;
    return true;
}

int main() {
    const Matrix A_ub{{-3, 1, 1, 2}, 2, 2}, A_eq{{1, 1}, 1, 2};
    const std::vector<double> b_ub{6, 4}, b_eq{1}, c{-1, 4};
    const Problem with_eq = Problem::target(c).ub(A_ub, b_ub).eq(A_eq, b_eq).build();
    const Problem ub_only = Problem::target(c).ub(A_ub, b_ub).build();
    try {
        const OptimizeResult plain = InteriorPoint::default_().solve(with_eq);
        const OptimizeResult tall_eq = InteriorPoint::default_().tall_eq_form().solve(with_eq);
        CHECK(close(tall_eq.x(), {1.0, 0.0}, 1e-6));
        CHECK(close(tall_eq.x(), plain.x(), 1e-6) && std::fabs(tall_eq.fun() - plain.fun()) <= 1e-6);
        const OptimizeResult tall = InteriorPoint::default_().tall_form().solve(with_eq);     // the ordinary path: the same bits
        CHECK(close(tall.x(), plain.x(), 0.0) && tall.fun() == plain.fun());
        const OptimizeResult a = InteriorPoint::default_().tall_form().solve(ub_only);
        const OptimizeResult b = InteriorPoint::default_().tall_eq_form().solve(ub_only);     // m_eq == 0: lpipm_upload_ub_tall itself
        CHECK(close(a.x(), b.x(), 0.0) && a.fun() == b.fun());
    } catch (const LinearProgramError& e) {
        std::printf("FAIL: %s\n", e.what());
        ++failures;
    }
    std::printf(failures ? "%d failure(s)\n" : "ok\n", failures);
    return failures ? 1 : 0;
}
