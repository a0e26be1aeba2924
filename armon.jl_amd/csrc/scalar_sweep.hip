// scalar_sweep.hip — fp64 instantiation of the passive-scalar sweep (armon_hip_sweep_scalars).
#define ARMON_SWEEP_REAL double
#define ARMON_SWEEP_DESC armon_sweep_desc
#define ARMON_SCALARS_FN armon_hip_sweep_scalars
#include "scalar_sweep.hpp"
