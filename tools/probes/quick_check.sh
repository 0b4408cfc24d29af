# parity + full-size tests, the bench line with its variant legs and roofline, and the render phase profile
# usage: bash tools/probes/quick_check.sh OUT_DIR      (on the GPU box)
O=${1:?usage: bash tools/probes/quick_check.sh OUT_DIR}; mkdir -p $O
timeout 600 python -m pytest -q -m gpu tests/test_hip_parity.py tests/test_hip_full_size.py -x > $O/pytest.log 2>&1; tail -2 $O/pytest.log
timeout 300 python bench.py --full --no-cpu-baseline --no-extras > $O/bench.json 2>$O/bench.err
python - $O/bench.json <<'PY'
import json, sys
j=json.loads(open(sys.argv[1]).read().strip().splitlines()[-1]); c=j["config"]
print('value %.1f pipelined %.1f exact %.1f allhit %.1f frac %.3f kernel %s' % (j["value"]/1e6, c["value_pipelined"]/1e6, c["value_mlp_exact_fp32"]/1e6, c["value_all_rays_hit"]/1e6, j["roofline"]["frac"], j["kernel_ms_stats"]))
PY
NFI_PHASES=1 timeout 200 python tools/quick_bench.py 2>&1 | grep -A8 "phase profile" | grep "total\|phase"
