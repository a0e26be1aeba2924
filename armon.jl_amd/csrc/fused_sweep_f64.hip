// fused_sweep_f64.hip — fp64 instantiation of the fused sweep (armon_hip_sweep).
#define ARMON_SWEEP_REAL double
#define ARMON_SWEEP_FN armon_hip_sweep
#define ARMON_SWEEP_DESC armon_sweep_desc
#define ARMON_CYCLE_FN armon_hip_cycle_xy
#define ARMON_PAIR_FN armon_hip_sweep_pair
#define ARMON_PAIR_PITCH_FN armon_hip_sweep_pair_pitch
#include "fused_sweep.hpp"
