// scalar_sweep_bounded_f32.hip — fp32 instantiation of the bound-preserving passive-scalar sweep (armon_hip_sweep_scalars_bounded_f32;
// DESIGN.md §4.17): scalar_sweep.hpp with the planes transported per unit mass.
#define ARMON_SWEEP_REAL float
#define ARMON_SWEEP_DESC armon_sweep_desc_f32
#define ARMON_SCALARS_FN armon_hip_sweep_scalars_bounded_f32
#define ARMON_SCALARS_TRANSPORT 1
#include "scalar_sweep.hpp"
