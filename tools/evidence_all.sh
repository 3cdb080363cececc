#!/bin/bash
# Whole round-end evidence in one GPU call: tools/evidence_profiles.sh <tag> (tests, smoke, 4 profiled
# workloads), the PMC records copied into profiles/ for bench.py, then the default bench line with
# every measurement (--full). Logs under $MGN_LOGDIR (default logs/).
TAG=${1:-r04}
LOGDIR=${MGN_LOGDIR:-logs}
bash tools/evidence_profiles.sh $TAG || exit 1
for s in "" f a p e; do cp $LOGDIR/prof_${TAG}$s/traffic.json profiles/${TAG}${s}_traffic.json; done
timeout -k 10 600 python3 bench.py --full > $LOGDIR/bench_$TAG.log 2>&1
rc=$?; echo bench=$rc; tail -1 $LOGDIR/bench_$TAG.log > $LOGDIR/bench_$TAG.json; exit $rc
