# The ceilings of the domain table's answer kernel on the bench batch: the whole kernel (0), without its table and row loads
# (1: the mask is a constant), without its mask stores (2: one word per wave, so that the loads stay alive).  Timing experiments
# that compute WRONG masks: they need a library built with `make clean && make EXPERIMENTS=1`; the product library does not
# know TXQ_PROBE_EXPERIMENT.  Two rounds, so that the spread shows.
set -e
cd "$(dirname "$0")/.."
for round in 1 2; do
  for e in 0 1 2; do
    TXQ_PROBE_EXPERIMENT=$e timeout -k 10 200 python3 bench.py --no-cpu --no-queries --steps 50 2>/dev/null | python3 -c "
import json,sys; d=json.loads(sys.stdin.read()); print('round $round TXQ_PROBE_EXPERIMENT=$e ms_per_step', round(d['ms_per_step'],4), 'avg_kernel_ms(HIP events)', round(d['roofline']['avg_kernel_ms'],4))"
  done
done
