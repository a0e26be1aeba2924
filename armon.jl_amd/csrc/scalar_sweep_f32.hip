// scalar_sweep_f32.hip — fp32 instantiation of the passive-scalar sweep (armon_hip_sweep_scalars_f32).
#define ARMON_SWEEP_REAL float
#define ARMON_SWEEP_DESC armon_sweep_desc_f32
#define ARMON_SCALARS_FN armon_hip_sweep_scalars_f32
#include "scalar_sweep.hpp"
