set -uo pipefail
# PPO GPU tests, then the 65,536-env bench line in fp32 and with bf16 GEMMs (logs and lines under $OUT, default a temp dir)
O=${OUT:-$(mktemp -d)}
echo "outputs in $O"
timeout -k 10 600 python3 -u -m pytest tests/test_ppo_gpu.py -m gpu -x -q --timeout 240 --timeout-method thread > $O/pytest.log 2>&1; rc=$?; tail -12 $O/pytest.log; [ $rc -ne 0 ] && exit $rc
for mp in "" "--mixed-precision"; do
  timeout -k 10 300 python3 bench.py --full --envs 65536 --steps 10 --no-cpu-baseline --c2-steps 0 $mp > $O/b$mp.json 2> $O/b$mp.err || exit $?
  python3 -c "import json;d=json.load(open('$O/b$mp.json'));e=d['extra'];print('$mp', d['value']/1e6, d['ms_per_step'], e['rollout_ms'], e['update_ms'], e['update_us_per_minibatch'], d['roofline_ppo']['launch_ms'], d['wall_clock_to_reward'])"
done
