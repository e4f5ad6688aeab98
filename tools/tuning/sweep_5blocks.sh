run() { env "$@" timeout -k 10 200 python bench.py --full --no-cpu-baseline 2>/dev/null | python -c "
import json,sys;d=json.loads(sys.stdin.read());print(sys.argv[1:],d['value'],d['roofline']['kernel_avg_launch_ms'],flush=True)" "$@"; }
run A=0
run RTAMD_WF_SPLIT=8:7
run RTAMD_WF_SPLIT=7:8
run RTAMD_WF_SPLIT=6:5
run RTAMD_WF_SPLIT=5:6
run RTAMD_WF_DYNAMIC_256=96
run RTAMD_WF_DYNAMIC_256=40
run RTAMD_TRACE_REFILL=12 RTAMD_LIGHT_REFILL=12
run RTAMD_TRACE_REFILL=24 RTAMD_LIGHT_REFILL=24
run RTAMD_TRACE_LEAF_BATCH=14 RTAMD_LIGHT_LEAF_BATCH=14
run RTAMD_TRACE_LEAF_BATCH=28 RTAMD_LIGHT_LEAF_BATCH=28
