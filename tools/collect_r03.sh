#!/bin/bash
# GPU box, ONE call: everything profiles/ quotes for round 3 (-> $out/r03_*).   bash tools/collect_r03.sh
cd $GRAFT_REPO_ROOT
export OUT_DIR=${OUT_DIR:-prof_out}; out=$OUT_DIR; mkdir -p $out   # output folder (git-ignored), shared with the scripts called below
bash tools/collect_profiles.sh r03 > $out/r03_collect.log 2>&1
bash tools/util_report.sh r03 >> $out/r03_collect.log 2>&1
python bench.py --full --config C1 --steps 48 --warmup 6 --no-cpu-baseline --no-fp32 --no-config2 2>&1 | tail -1 > $out/r03_bench_config2_1deg.json
python tools/stage_classes.py C3 bf16 > $out/r03_stage_classes_C3_bf16.txt 2>&1
WX_ATTN_BLOCK=1 python tools/stage_classes.py C3 bf16 > $out/r03_stage_classes_C3_bf16_attn_block.txt 2>&1
cd /tmp && export TMPDIR=/tmp && cd $GRAFT_REPO_ROOT
rocprofv3 --kernel-trace --stats --output-format csv -d $out/r03_fx -o kt -- python tools/fuxi_time.py bf16 5 > $out/r03_fuxi_time.log 2>&1
python tools/prof_summary.py $out/r03_fx > $out/r03_fuxi_kernel_stats.txt
rm -rf $out/r03_fx
python tools/fuxi_time.py bf16 10 2>&1 | tail -1 > $out/r03_fuxi_forward.txt
python tools/fuxi_time.py fp32 3 2>&1 | tail -1 >> $out/r03_fuxi_forward.txt
(for a in "400 800 128 10 0 2" "400 800 128 10 1 2" "200 400 256 10 0 2" "200 400 256 5 1 2"; do tools/_build/attn_block_probe $a; done) > $out/r03_attn_block_probe.txt 2>&1
(WX_ABL=1 tools/_build/gemm_pp_probe 0) > $out/r03_gemm_pp_probe.txt 2>&1
cut -c1-400 $out/r03_bench.json; head -14 $out/r03_kernel_stats.txt; cat $out/r03_fuxi_forward.txt; cut -c1-200 $out/r03_bench_config2_1deg.json
