# round 3 measurement pass: everything profiles/r03_* is made of, on one box, with the library that ships
O=gpurun_out/r3f; mkdir -p $O
cd /tmp && export TMPDIR=/tmp && cd $GRAFT_REPO_ROOT
sha256sum globecom2020-resourceallocationgnn_amd/libv2xgnn.so > $O/lib_sha.txt
timeout 2400 python -m pytest tests -m gpu -q -s 2>&1 | grep -v amdgpu.ids | grep -e "every gradient" -e passed -e failed -e FAILED -e Error | tail -12 > $O/gputests.txt; cat $O/gputests.txt
# PMC passes first (hbm_traffic.json must exist before bench.py reports roofline.traffic)
B="python bench.py --no-graph --no-cpu-baseline --no-roofline --no-edge-gather --steps 40 --warmup 5 --min-seconds 0"
rocprofv3 --pmc FETCH_SIZE -d $O/fetch -o pmc -- $B > /dev/null 2> $O/fetch.err
rocprofv3 --pmc WRITE_SIZE -d $O/write -o pmc -- $B > /dev/null 2> $O/write.err
python tools/make_traffic_json.py $(ls $O/fetch/*/*.db $O/fetch/*.db 2>/dev/null | head -1) $(ls $O/write/*/*.db $O/write/*.db 2>/dev/null | head -1) > $O/hbm_traffic.json
cp $O/hbm_traffic.json profiles/hbm_traffic.json
rocprofv3 --pmc SQ_WAVE_CYCLES SQ_BUSY_CYCLES SQ_WAIT_ANY SQ_WAIT_INST_ANY SQ_WAIT_INST_LDS SQ_ACTIVE_INST_ANY SQ_ACTIVE_INST_VALU SQ_INSTS_VALU_MFMA_MOPS_F32 -d $O/st1 -o pmc -- $B > /dev/null 2> $O/st1.err
rocprofv3 --pmc SQ_WAVE_CYCLES SQ_ACTIVE_INST_LDS SQ_ACTIVE_INST_VMEM SQ_ACTIVE_INST_SCA SQ_ACTIVE_INST_MISC SQ_VALU_MFMA_BUSY_CYCLES SQ_INSTS_VMEM SQ_INSTS_LDS -d $O/st2 -o pmc -- $B > /dev/null 2> $O/st2.err
rocprofv3 --pmc SQ_WAVES SQ_INSTS_VALU SQ_INSTS_SALU SQ_INSTS_MFMA SQ_INST_CYCLES_VMEM SQ_WAIT_INST_VMEM SQ_BUSY_CYCLES -d $O/st3 -o pmc -- $B > /dev/null 2> $O/st3.err
python tools/stall_table.py $(ls $O/st1/*/*.db $O/st1/*.db | head -1) $(ls $O/st2/*/*.db $O/st2/*.db | head -1) $(ls $O/st3/*/*.db $O/st3/*.db | head -1) > $O/stalls.txt 2>&1
# headline + kernel stats of the same command
python bench.py --full > $O/bench.json 2> $O/bench.err; cut -c1-700 $O/bench.json
rocprofv3 --kernel-trace --stats -d $O/prof -o stats -- python bench.py --no-cpu-baseline --no-roofline --no-edge-gather --min-seconds 0.5 > $O/prof_bench.json 2> $O/prof.err
python tools/rocpd_summary.py $(ls $O/prof/*/*.db $O/prof/*.db 2>/dev/null | head -1) > $O/kernel_stats.txt 2>&1; head -9 $O/kernel_stats.txt
# shares of the fixed global batch, other workloads
Q="python bench.py --full --no-cpu-baseline"
for g in 2 4 8; do $Q --shard-of $g --no-edge-gather > $O/bench_b$((4096/g)).json 2>/dev/null; done
$Q --share-weights > $O/bench_shared.json 2>/dev/null
$Q --batch 65536 --steps 20 --warmup 3 --no-edge-gather > $O/bench_b65536.json 2>/dev/null
V2X_FUSED=0 V2X_MLP_WG=0 $Q > $O/bench_layerwise.json 2>/dev/null
V2X_MLP_WG=0 $Q > $O/bench_mlp_split.json 2>/dev/null
for wl in cfg4 cfg5; do
  $Q --workload $wl --shard-of 8 > $O/bench_$wl.json 2> /dev/null
  W="python bench.py --workload $wl --shard-of 8 --no-graph --no-cpu-baseline --no-roofline --steps 20 --warmup 3 --min-seconds 0"
  rocprofv3 --pmc FETCH_SIZE -d $O/fetch_$wl -o pmc -- $W > /dev/null 2> $O/fetch_$wl.err
  rocprofv3 --pmc WRITE_SIZE -d $O/write_$wl -o pmc -- $W > /dev/null 2> $O/write_$wl.err
  rocprofv3 --pmc SQ_VALU_MFMA_BUSY_CYCLES SQ_BUSY_CYCLES SQ_WAVE_CYCLES SQ_WAIT_ANY SQ_WAIT_INST_ANY SQ_ACTIVE_INST_ANY SQ_WAIT_INST_LDS SQ_ACTIVE_INST_LDS -d $O/mfma_$wl -o pmc -- $W > /dev/null 2> $O/mfma_$wl.err
  for d in fetch write mfma; do python tools/rocpd_summary.py $(ls $O/${d}_$wl/*/*.db $O/${d}_$wl/*.db 2>/dev/null | head -1) > $O/${d}_$wl.txt 2>&1; done
  python tools/roofline_table2.py $O/bench_$wl.json $O/fetch_$wl.txt $O/write_$wl.txt $O/mfma_$wl.txt > $O/roofline_$wl.md 2>&1
done
python bench.py --full --workload cfg0 --envs 10 > $O/bench_cfg0_episode_envs10.json 2>/dev/null
python bench.py --workload cfg2loop --envs 50 > $O/bench_cfg2loop_envs50.json 2>/dev/null
python tools/predict_latency.py 2>&1 | grep -v amdgpu.ids > $O/predict_latency.txt
python tools/roofline_table.py $O/bench.json $O/hbm_traffic.json > $O/roofline.md 2>&1
for f in $O/bench_*.json; do echo "$f: $(python -c "
import json
d=json.loads(open('$f').read().strip().splitlines()[-1])
print(d.get('ms_per_step'), d.get('value'), (d.get('roofline') or {}).get('kernel'), (d.get('roofline') or {}).get('frac'))")"; done
