// test_ripped_bounds.cpp -- ProblemBuilder::lower of include/ripped.hpp, through liblpipm.so on device 0: one shifted, one
// reflected and one free column (min x1 - x2 + x3, x1 + x2 + x3 <= 10, x3 - x1 = 1, x1 >= -2, x2 <= 3, x3 free: x = (-2, 3, -1),
// fun = -6) through lpipm_upload_bounds; the same LP rewritten by hand in non-negative variables (x1 = -2 + a, x2 = 3 - b,
// x3 = p - q) gives the same answer and iteration count; the duals come in the caller's orientation; an LP unbounded along its
// free column throws with the improving ray; the builder refuses a lower bound of +inf.
#include <cmath>
#include <cstdio>
#include <limits>
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
    const double inf = std::numeric_limits<double>::infinity();
    const Matrix A_ub{{1, 1, 1}, 1, 3}, A_eq{{-1, 0, 1}, 1, 3};
    const std::vector<double> b_ub{10}, b_eq{1}, c{1, -1, 1}, lo{-2, -inf, -inf}, up{inf, 3, inf};
    const Problem general = Problem::target(c).ub(A_ub, b_ub).eq(A_eq, b_eq).lower(lo).upper(up).build();
    CHECK(general.general_bounds() && general.n_bounded() == 0 && general.n_free() == 1 && general.tail() == 2);
    CHECK(general.lower() == lo && general.upper() == up);
    // by hand: columns (a, b, p, q); a - b + p - q <= 9; -a + p - q = -1; cost a + b + p - q (- 5)
    const Matrix H_ub{{1, -1, 1, -1}, 1, 4}, H_eq{{-1, 0, 1, -1}, 1, 4};
    const std::vector<double> hb_ub{9}, hb_eq{-1}, hc{1, 1, 1, -1};
    const Problem by_hand = Problem::target(hc).ub(H_ub, hb_ub).eq(H_eq, hb_eq).build();
    CHECK(!by_hand.general_bounds() && by_hand.n_free() == 0);
    try {
        const OptimizeResult got = InteriorPoint::default_().solve(general);
        const OptimizeResult want = InteriorPoint::default_().solve(by_hand);
        CHECK(close(got.x(), {-2.0, 3.0, -1.0}, 1e-6) && std::fabs(got.fun() + 6.0) <= 1e-6);
        const std::vector<double>& h = want.x();
        CHECK(h.size() == 4 && close(got.x(), {-2.0 + h[0], 3.0 - h[1], h[2] - h[3]}, 1e-6) && got.iteration() == want.iteration());
        CHECK(std::fabs(got.fun() - (want.fun() - 5.0)) <= 1e-6);
        const InteriorPoint::DualResult d = InteriorPoint::default_().solve_with_duals(general);
        CHECK(d.y_ub.size() == 1 && d.y_eq.size() == 1 && d.reduced_costs.size() == 3);
        CHECK(close(d.result.x(), {-2.0, 3.0, -1.0}, 1e-6) && std::fabs(d.dual_fun - d.result.fun()) <= 1e-6);
        if (d.y_ub.size() == 1 && d.y_eq.size() == 1 && d.reduced_costs.size() == 3) {
            // A^T y + z = c in the caller's orientation: z <= 0 on the reflected column, ~ 0 on the free one
            for (int j = 0; j < 3; ++j)
                CHECK(std::fabs(A_ub.data[j] * d.y_ub[0] + A_eq.data[j] * d.y_eq[0] + d.reduced_costs[j] - c[j]) <= 1e-6);
            CHECK(d.reduced_costs[0] >= -1e-6 && d.reduced_costs[1] <= 1e-6 && std::fabs(d.reduced_costs[2]) <= 1e-6);
        }
    } catch (const LinearProgramError& e) {
        std::printf("FAIL: %s\n", e.what());
        ++failures;
    }
    // min -x3, x1 + x2 = 1, 0 <= x1 <= 1, x2 >= 0.5, x3 free: unbounded along the free column
    const Matrix U_eq{{1, 1, 0}, 1, 3};
    const std::vector<double> ub_{1}, uc{0, 0, -1}, ulo{0, 0.5, -inf}, uup{1, inf, inf};
    bool thrown = false;
    try {
        (void)InteriorPoint::default_().solve_with_certificate(Problem::target(uc).eq(U_eq, ub_).lower(ulo).upper(uup).build());
    } catch (const CertifiedError& e) {
        thrown = e.kind() == ErrorKind::Unbounded && e.certificate().kind == LPIPM_CERT_RAY && e.certificate().x.size() == 3 &&
                 e.certificate().x[2] > 0 && e.certificate().residual <= 1e-6;
    } catch (const LinearProgramError& e) {
        std::printf("FAIL: %s\n", e.what());
    }
    CHECK(thrown);
    bool refused = false;
    try {
        const std::vector<double> bad{0, inf, 0};
        (void)Problem::target(c).ub(A_ub, b_ub).lower(bad).build();
    } catch (const LinearProgramError&) {
        refused = true;
    }
    CHECK(refused);
    std::printf(failures ? "%d failure(s)\n" : "ok\n", failures);
    return failures ? 1 : 0;
}
