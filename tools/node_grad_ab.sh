#!/bin/bash
# Same-box A/B of the node side of the block backward, run on the GPU box from the repo root after
#   python __graft_entry__.py && bash tools/build_variant.sh gen "-DMGN_CHAIN_NODE_GRAD=0" mgn_mlp.hip
# A = the generic node_grad_kernel everywhere (var/libmgn_gen.so), B = the shipped library (chain16_node_grad_kernel
# where node_grad_any picks it). Headline six times per side, interleaved; the last step's outputs compared array
# for array (Cfg B and Cfg E); Cfg E and the plate workload once per side; per-class times alone (--full); one
# kernel trace per side (no counters) for the launch inside the replayed step. Output under $MGN_LOGDIR/node_grad_ab
# (default logs/): ab_headline.txt is the record, profiles/node_grad_chain_ab.txt its copy with the trace lines.
L=graph-physics_amd/graphphysics/_lib
O=${MGN_LOGDIR:-logs}/node_grad_ab
mkdir -p $O
cp $L/libmgn.so /tmp/libmgn_B.so
cp $L/var/libmgn_gen.so /tmp/libmgn_A.so
use() { cp /tmp/libmgn_$1.so $L/libmgn.so; touch $L/libmgn.so; }
val() { tail -1 $1 | python3 -c "import json,sys; d=json.loads(sys.stdin.read()); print(d['value'], d['ms_per_step'])"; }
run() {  # side tag timeout args...
  local side=$1 tag=$2 to=$3; shift 3
  use $side
  timeout -k 10 $to python bench.py "$@" > $O/ab_${tag}_$side.log 2>&1
  local rc=$?
  if [ $rc -ne 0 ]; then echo "$tag $side failed rc=$rc"; tail -5 $O/ab_${tag}_$side.log; use B; exit 1; fi
}
: > $O/ab_headline.txt
for i in 1 2 3 4 5 6; do
  for s in A B; do
    run $s head$i 200
    echo "headline $i $s $(val $O/ab_head${i}_$s.log)" | tee -a $O/ab_headline.txt
  done
done
# results unchanged
for s in A B; do run $s dump 200 --steps 20 --dump-outputs /tmp/dump_$s; done
python3 tools/compare_dumps.py /tmp/dump_A /tmp/dump_B 2>&1 | tail -3 | tee $O/ab_dumps.txt
[ ${PIPESTATUS[0]} -eq 0 ] || { use B; exit 1; }
# other workloads, once per side
for w in aneurysm plate; do
  for s in A B; do
    run $s $w 300 --workload $w
    echo "$w $s $(val $O/ab_${w}_$s.log)" | tee -a $O/ab_headline.txt
  done
done
for s in A B; do run $s dumpE 300 --workload aneurysm --steps 20 --dump-outputs /tmp/dumpE_$s; done
python3 tools/compare_dumps.py /tmp/dumpE_A /tmp/dumpE_B 2>&1 | tail -1 | tee -a $O/ab_dumps.txt
[ ${PIPESTATUS[0]} -eq 0 ] || { use B; exit 1; }
# per class, one stream on the whole chip
for s in A B; do
  run $s full 400 --full --no-secondary --cpu-steps 0
  echo "full $s $(tail -1 $O/ab_full_$s.log | python3 -c "import json,sys; d=json.loads(sys.stdin.read()); k=d['kernels']; print(d['value'], ' '.join('%s=%s' % (n, k[n]['avg_us']) for n in sorted(k)))")" | tee -a $O/ab_headline.txt
done
# in the replay: kernel trace, no counters
ARGS="--steps 5 --warmup 3 --cpu-steps 0 --no-mse --no-profile --no-secondary --sustain 0"
for s in A B; do
  use $s
  rm -rf /tmp/trace_$s
  timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d /tmp/trace_$s -o run -- python3 bench.py $ARGS > $O/ab_trace_$s.log 2>&1 || { echo "trace $s failed"; tail -5 $O/ab_trace_$s.log; use B; exit 1; }
  python3 tools/gap_summary.py $(find /tmp/trace_$s -name '*kernel_trace.csv' | head -1) 5 > $O/ab_trace_summary_$s.txt
  head -1 $O/ab_trace_summary_$s.txt; grep node_grad $O/ab_trace_summary_$s.txt
done
use B
echo ab-done
