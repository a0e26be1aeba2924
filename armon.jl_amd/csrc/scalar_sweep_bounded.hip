// scalar_sweep_bounded.hip — fp64 instantiation of the bound-preserving passive-scalar sweep (armon_hip_sweep_scalars_bounded;
// DESIGN.md §4.17): scalar_sweep.hpp with the planes transported per unit mass.
#define ARMON_SWEEP_REAL double
#define ARMON_SWEEP_DESC armon_sweep_desc
#define ARMON_SCALARS_FN armon_hip_sweep_scalars_bounded
#define ARMON_SCALARS_TRANSPORT 1
#include "scalar_sweep.hpp"
