// CPU test of csrc/cycle_kick.hpp (the host arithmetic of the kick that ends armon_hip_mgpu_cycle), built with
// -fsanitize=address,undefined by tests/test_body_force_host.py: the range walks exactly the real cells of a ghosted block —
// marked in a buffer of the block's own size, so that an index outside it is the sanitizer's to report —, and the cycle's step
// is recovered from the plans of every splitting.
#include "../../armon.jl_amd/csrc/cycle_kick.hpp"

#include <cstdio>
#include <cstdlib>
#include <vector>

#define CHECK(cond)                                                          \
    do {                                                                     \
        if (!(cond)) {                                                       \
            printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);         \
            return 1;                                                        \
        }                                                                    \
    } while (0)

static armon_cycle_plan plan_of(int n, const int* axis, const double* factor, double dt)
{
    armon_cycle_plan p = {};
    p.n_sweeps = n;
    for (int s = 0; s < n; s++) {
        p.axis[s] = axis[s];
        p.dt[s] = dt * factor[s];
    }
    p.dt[3] = 1e300;                       // not a sweep of the cycle: never read
    return p;
}

int main()
{
    const int64_t shapes[][3] = {{5, 3, 2}, {64, 1, 5}, {1, 1, 1}, {130, 7, 4}, {3, 7000, 5}, {24, 20, 0}};
    for (const auto& s : shapes) {
        const int64_t nx = s[0], ny = s[1], g = s[2], row = nx + 2 * g, rows = ny + 2 * g;
        const armon_range r = armon::real_range(nx, ny, (int)g);
        CHECK(r.col_len == ny && r.row_len == nx && r.col_step == row && r.row_start == 0);
        std::vector<unsigned char> hit((size_t)(row * rows), 0);
        for (int64_t j = 0; j < r.col_len; j++)
            for (int64_t i = 0; i < r.row_len; i++) hit[(size_t)(r.col_start + j * r.col_step + r.row_start + i)]++;
        for (int64_t y = 0; y < rows; y++)
            for (int64_t x = 0; x < row; x++) {
                const bool real = x >= g && x < g + nx && y >= g && y < g + ny;
                CHECK(hit[(size_t)(y * row + x)] == (real ? 1 : 0));
            }
    }
    const double steps[] = {1e-3, 0.1, 1. / 3., 4.94e-324, 1.7e308, 0.0123f};
    const int X = ARMON_AXIS_X, Y = ARMON_AXIS_Y;
    const int seq[] = {X, Y}, rev[] = {Y, X}, strang_even[] = {X, Y, X}, strang_odd[] = {Y, X, Y}, x_only[] = {X}, y_only[] = {Y};
    const double one[] = {1., 1.}, halves[] = {0.5, 1., 0.5};
    for (double dt : steps) {
        CHECK(armon::cycle_step(plan_of(2, seq, one, dt)) == dt);
        CHECK(armon::cycle_step(plan_of(2, rev, one, dt)) == dt);
        CHECK(armon::cycle_step(plan_of(1, x_only, one, dt)) == dt);
        CHECK(armon::cycle_step(plan_of(1, y_only, one, dt)) == dt);
        if (dt > 1e-300) {                 // (half of the smallest subnormal is not a number of the format)
            CHECK(armon::cycle_step(plan_of(3, strang_even, halves, dt)) == dt);
            CHECK(armon::cycle_step(plan_of(3, strang_odd, halves, dt)) == dt);
        }
        // fp32 runs: the plan holds products formed in float
        const float f = (float)dt;
        if (f > 1e-30f && f < 1e30f) {
            armon_cycle_plan p = plan_of(3, strang_even, halves, 0.);
            p.dt[0] = p.dt[2] = (double)(f * 0.5f);
            p.dt[1] = (double)f;
            CHECK((float)armon::cycle_step(p) == f);
        }
    }
    armon_cycle_plan none = {};
    CHECK(armon::cycle_step(none) == 0.);
    printf("cycle_kick OK\n");
    return 0;
}
