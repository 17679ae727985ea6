# A round's profile set in one GPU session: bash tools/collect_profiles.sh [OUT] (OUT defaults to prof_out/; R=rNN names the
# files, default r04).  Counter passes carry --pmc only (no trace domains); the program goes directly after `--`.
cd "$(dirname "$0")/.." && export TMPDIR=/tmp && R=${R:-r04} && OUT=${1:-prof_out} && mkdir -p "$OUT" && \
rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/${R}k -o k -- python3 bench.py --full --steps 5 --warmup 2 --no-cpu-baseline --no-fresh > $OUT/${R}k.log 2>&1 && echo stats-done && \
rocprofv3 --pmc FETCH_SIZE --output-format csv -d $OUT/pmc_f -o p -- python3 bench.py --full --steps 1 --warmup 1 --no-cpu-baseline --no-fresh > $OUT/pmc_f.log 2>&1 && echo fetch-done && \
rocprofv3 --pmc WRITE_SIZE --output-format csv -d $OUT/pmc_w -o p -- python3 bench.py --full --steps 1 --warmup 1 --no-cpu-baseline --no-fresh > $OUT/pmc_w.log 2>&1 && echo write-done && \
rocprofv3 --pmc SQ_VALU_MFMA_BUSY_CYCLES SQ_BUSY_CU_CYCLES SQ_ACTIVE_INST_VALU SQ_WAVE_CYCLES SQ_WAIT_ANY SQ_WAIT_INST_ANY SQ_ACTIVE_INST_ANY SQ_VALU_MFMA_COEXEC_CYCLES --output-format csv -d $OUT/pmc_b -o p -- python3 bench.py --full --steps 1 --warmup 1 --no-cpu-baseline --no-fresh > $OUT/pmc_b.log 2>&1 && echo busy-done && \
rocprofv3 --pmc SQ_INSTS_LDS SQ_ACTIVE_INST_LDS SQ_LDS_BANK_CONFLICT SQ_WAIT_INST_LDS SQ_LDS_IDX_ACTIVE SQ_BUSY_CU_CYCLES SQ_WAVE_CYCLES --output-format csv -d $OUT/pmc_l -o p -- python3 bench.py --full --steps 1 --warmup 1 --no-cpu-baseline --no-fresh > $OUT/pmc_l.log 2>&1 && echo lds-done && \
python3 tools/pmc_traffic.py traffic $OUT/pmc_f/p_counter_collection.csv $OUT/pmc_w/p_counter_collection.csv 4194304 > $OUT/${R}_pmc_traffic.json && \
python3 tools/pmc_traffic.py busy $OUT/pmc_b/p_counter_collection.csv,$OUT/pmc_l/p_counter_collection.csv 4194304 > $OUT/${R}_pmc_mfma.json && echo json-done && rm -rf $OUT/pmc_f $OUT/pmc_w $OUT/pmc_b $OUT/pmc_l && \
python3 bench.py --full --steps 10 --warmup 3 > $OUT/${R}_bench.json 2> $OUT/${R}_bench.err && echo bench-done && \
python3 bench.py --full --config 3 --steps 10 --warmup 3 --no-cpu-baseline > $OUT/${R}_bench_cfg3.json 2> $OUT/${R}_bench_cfg3.err && \
python3 bench.py --full --config 5 --steps 10 --warmup 3 --no-cpu-baseline > $OUT/${R}_bench_cfg5.json 2> $OUT/${R}_bench_cfg5.err && echo cfg-done
