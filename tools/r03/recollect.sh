#!/bin/bash
# re-collections after the last kernel changes of round 3: the fp32 line under rocprofv3 and the tile measurements
root=${GRAFT_REPO_ROOT:-$PWD}
out=$root/gpurun_out/prof_r03
mkdir -p $out
cd /tmp && export TMPDIR=/tmp
tag=r03_fused_fast_sod16384_f32
rocprofv3 --kernel-trace --stats --output-format csv -d $out/$tag -- python3 $root/bench.py --full --f32 --no-cpu-baseline > $out/${tag}_bench_under_rocprof.json 2> $out/${tag}.err
cp "$(find $out/$tag -name '*kernel_stats.csv' | head -1)" $out/${tag}_kernel_stats.csv
python3 $root/tools/trace_timed_region.py "$(find $out/$tag -name '*kernel_trace.csv' | head -1)" $out/${tag}_timed_region.json 20 k_sweep > /dev/null
rm -rf $out/$tag
cd $root
bash tools/r03/tiles.sh > gpurun_out/r03_tiles_2.txt 2>&1
python tools/tile_overhead.py --grids 1x8,2x4 >> gpurun_out/r03_tiles_2.txt 2>&1
