set -o pipefail
cd $GRAFT_REPO_ROOT
out="${VR_OUT:-out}/final"
mkdir -p "$out"
timeout -k 10 900 python -u -m pytest -x -q --timeout 300 --timeout-method thread -m gpu tests/ > "$out/gpu_tests.log" 2>&1 || { echo TESTFAIL; grep -E "^FAILED|^ERROR|Error" "$out/gpu_tests.log" | head; exit 1; }
tail -n 1 "$out/gpu_tests.log"
timeout -k 10 300 python -c "import __graft_entry__ as g; g.smoke(); print('smoke ok')" > "$out/smoke.log" 2>&1 || { echo SMOKEFAIL; tail "$out/smoke.log"; exit 1; }
tail -n 1 "$out/smoke.log"
timeout -k 10 600 python bench.py --full --gpus 1 --steps 20 --warmup 5 > "$out/bench.json" 2> "$out/bench.err" || { echo BENCHFAIL; tail "$out/bench.err"; exit 1; }
python -c "import json,sys;d=json.load(open(sys.argv[1]));print('bench', d['value'], d['ms_per_step'], d['roofline']['frac'], d['cpu_baseline']['value'])" "$out/bench.json"
