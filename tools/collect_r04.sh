#!/bin/bash
# GPU box, ONE call: everything profiles/ quotes for round 4 (-> $out/r04_*).   bash tools/collect_r04.sh
cd $GRAFT_REPO_ROOT
export OUT_DIR=${OUT_DIR:-prof_out}; out=$OUT_DIR; mkdir -p $out   # output folder (git-ignored), shared with the scripts called below
bash tools/collect_profiles.sh r04 > $out/r04_collect.log 2>&1
bash tools/util_report.sh r04 >> $out/r04_collect.log 2>&1
python bench.py --full --config C1 --steps 48 --warmup 6 --no-cpu-baseline --no-fp32 --no-config2 --no-host-delivery --no-concurrent 2>&1 | tail -1 > $out/r04_bench_config2_1deg.json
python tools/stage_classes.py C3 bf16 > $out/r04_stage_classes_C3_bf16.txt 2>&1
cd /tmp && export TMPDIR=/tmp && cd $GRAFT_REPO_ROOT
rocprofv3 --kernel-trace --stats --output-format csv -d $out/r04_fx -o kt -- python tools/fuxi_time.py bf16 5 > $out/r04_fuxi_time.log 2>&1
python tools/prof_summary.py $out/r04_fx > $out/r04_fuxi_kernel_stats.txt
rm -rf $out/r04_fx
python tools/fuxi_time.py bf16 10 2>&1 | tail -1 > $out/r04_fuxi_forward.txt
BAND_CLASSES=1 python tools/band_time.py C3 bf16 8 > $out/r04_latband_virtual_ranks_C3_bf16.txt 2>&1
tools/_build/gemm_wreg_probe 1 > $out/r04_gemm_wreg_probe_raw.txt 2>&1
WX_LC_CFG=2 tools/_build/gemm_lc_probe 0 > $out/r04_gemm_lc_probe_raw.txt 2>&1
python tools/stress_report.py > $out/r04_stress_report.txt 2>&1
cut -c1-400 $out/r04_bench.json; head -14 $out/r04_kernel_stats.txt; cat $out/r04_fuxi_forward.txt; cut -c1-200 $out/r04_bench_config2_1deg.json
