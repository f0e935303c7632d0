# in-step A/B of two builds of the library (interleaved, one box): ab_lib.sh "finetrainers_amd/libftmi355_prev.so finetrainers_amd/libftmi355.so" [rounds] [extra env] [benchmark command]
# The benchmark command (default: the flagship line of bench.py) prints its JSON result as its last line; a run that fails or hangs ends the A/B.
set -o pipefail
LIBS=$1; R=${2:-2}; CMD=${4:-python bench.py --full --steps 12 --warmup 3 --no-cpu-baseline}
for r in $(seq $R); do for l in $LIBS; do echo -n "$l  "; env FTMI_LIB_PATH=$l ${3:-} timeout -k 10 600 $CMD 2>/dev/null | python -c "
import json,sys
d=json.loads([x for x in sys.stdin.read().splitlines() if x.startswith('{')][-1]); print('ms/step %.2f'%d.get('ms_per_step',d.get('step_ms')), 'min/med/max', d.get('step_ms_min_median_max') or sorted(round(v,3) for v in d['steps_ms'][d['warmup']:]), ' '.join('%s %.2f'%(k,v['ms_per_step']) for k,v in d.get('kernels',{}).items()))" || exit 1; done; done
