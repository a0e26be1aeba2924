// cycle_kick.hpp — the host arithmetic of the body-force kick that ends armon_hip_mgpu_cycle (multi_gpu.hip):
// which cells a tile kicks and with which step. Plain C++ over the header's structs, no HIP: tests/native/cycle_kick_test.cpp
// runs it on the CPU under ASan / UBSan (tests/test_body_force_host.py).
#pragma once

#include <cstdint>

#include "../../include/armon_hip.h"

namespace armon {

// the real cells of a tile of nx x ny cells with `nghost` ghost layers (ref real_domain: domain_range((0, 0), (0, 0)))
inline armon_range real_range(int64_t nx, int64_t ny, int nghost)
{
    const int64_t row = nx + 2 * (int64_t)nghost;
    return armon_range{nghost * row + nghost, row, ny, 0, nx};
}

// The cycle's full step current_dt from a plan that only holds the steps of its sweeps (dt[s] = current_dt x the splitting's
// factor): the sum over the sweeps along the cycle's first axis — one sweep of factor 1 under every splitting of the
// reference but Strang, whose two halves add up exactly (a product by 0.5 is exact, and so is the sum of two equal halves).
inline double cycle_step(const armon_cycle_plan& plan)
{
    double dt = 0.;
    for (int s = 0; s < plan.n_sweeps && s < 4; s++)
        if (plan.axis[s] == plan.axis[0]) dt += plan.dt[s];
    return dt;
}

}  // namespace armon
