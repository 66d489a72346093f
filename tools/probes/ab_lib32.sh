#!/bin/bash
# Same-box A/B of other builds of the library against this one on the headline job (1024^2, Adam, fp32), the driver's own command in
# alternating fresh processes, three rounds: ab_lib32.sh <other libst2_hip.so> [<another> ...]
# (e.g. the parent commit's library next to the tree's: every run of the tree above every run of the parent, and the difference of
# the medians a multiple of the parent's own max - min, is what "faster" means on a box whose default line repeats within +-0.2 it/s)
set -o pipefail
for i in 1 2 3; do
  for lib in "$@" ""; do
    ST2_HIP_LIB=${lib:-$PWD/style_transfer2_amd/lib/libst2_hip.so} timeout -k 10 300 python3 bench.py --gpus 1 --steps 30 --warmup 5 2>/dev/null \
      | python3 -c "import json,sys; d=json.loads(sys.stdin.read().strip().splitlines()[-1]); print('%-60s round $i: %.3f it/s  %.4f ms/step' % ('${lib:-this build}', d['value'], d['ms_per_step']))" || exit 1
  done
done
