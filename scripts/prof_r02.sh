# Round-2 profiling recipe (run on the GPU box via gpurun).  Kernel-trace stats first, then PMC passes in their own runs (never
# combined with sys/runtime/hip tracing).  scripts/summarize_profiles_r02.py turns the raw outputs into profiles/r02_*.
cd /tmp && export TMPDIR=/tmp
cd $GRAFT_REPO_ROOT
OUT=gpurun_out/prof_r02
rm -rf $OUT && mkdir -p $OUT
B="python bench.py --no-cpu-baseline"
# (1) the strict configuration: one forward at a time (the engine's default schedule for a forward alone)
rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/single -o s -- $B --sequential --steps 8 --warmup 3 --no-phase-a > $OUT/single.log 2>&1
# (1b) the same without the chunk overlap: every scan is ONE whole-sequence launch (the durations the roofline figures use)
SFSN_OVERLAP_CHUNKS=0 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/single_whole -o s -- $B --sequential --steps 8 --warmup 3 --no-phase-a > $OUT/single_whole.log 2>&1
# (2) the default command (phases S, K and the timed region with 12 forwards in flight)
rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/default -o d -- $B --full > $OUT/default.log 2>&1
# (3) PMC passes, whole-sequence launches, one forward at a time
for c in "FETCH_SIZE" "WRITE_SIZE" "SQ_WAVES SQ_BUSY_CYCLES SQ_WAVE_CYCLES SQ_INSTS_VALU SQ_ACTIVE_INST_VALU SQ_WAIT_INST_ANY SQ_WAIT_ANY SQ_ACTIVE_INST_ANY" "SQ_INSTS_MFMA SQ_VALU_MFMA_BUSY_CYCLES SQ_INSTS_LDS SQ_ACTIVE_INST_LDS SQ_LDS_BANK_CONFLICT SQ_INSTS_VMEM_WR SQ_INSTS_VMEM_RD GRBM_GUI_ACTIVE"; do
  tag=$(echo $c | cut -d' ' -f1)
  SFSN_OVERLAP_CHUNKS=0 rocprofv3 --pmc $c --kernel-trace --output-format csv -d $OUT/pmc_$tag -o p -- $B --sequential --steps 2 --warmup 1 --no-phase-a > $OUT/pmc_$tag.log 2>&1
done
# (4) HBM traffic of one forward in the timed region's geometry (full-band stack at 8, sub-band scans at 16 rows per workgroup, fused input products)
for c in FETCH_SIZE WRITE_SIZE; do
  SFSN_OVERLAP_CHUNKS=0 rocprofv3 --pmc $c --kernel-trace --output-format csv -d $OUT/job_$c -o p -- $B --sequential --rpw 8,16 --steps 3 --warmup 1 --no-phase-a > $OUT/job_$c.log 2>&1
done
python bench.py --full > $OUT/bench_default.json 2> $OUT/bench_default.err
python bench.py --streaming --no-cpu-baseline > $OUT/bench_streaming.json 2>> $OUT/bench_default.err
python -c "from spiking_fullsubnet_amd import _lib; print(_lib.source_hash())" > $OUT/source_hash.txt
tail -c 600 $OUT/bench_default.json
