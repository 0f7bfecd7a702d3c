mkdir -p gpurun_out
timeout -k 10 600 python -m pytest tests/test_gpu_device_level.py tests/test_gpu_parity.py -x -q > gpurun_out/dl.log 2>&1; tail -2 gpurun_out/dl.log
GPRC_PANEL_TRACE=0 GPRC_SERVICE=0 timeout -k 10 120 python tools/panel_trace.py 8192 2>&1 | tail -1
timeout -k 10 120 python tools/factor_bench.py 8192 16384 > gpurun_out/fb_now.txt 2>&1; grep factor_all gpurun_out/fb_now.txt
timeout -k 10 120 python bench.py --full --workload c2 --steps 10 --warmup 3 --no-cpu-baseline | python -c "
import json, sys
d=json.loads([ln for ln in sys.stdin if ln.startswith('{')][0]); print(d['ms_per_step'], d['phases_ms']['fit_F1_F3'], d.get('parity_timed_config_normwise_err'))"
timeout -k 10 200 python tools/service_trace.py 8192 2>&1 | tail -1
