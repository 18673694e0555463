#!/bin/bash
# strict forward with deeper full-band rings (exp libs dg6 / dg9; their combination with the prep of all chunks ahead was measured
# with a switch that is gone: profiles/EXPERIMENTS.md)
run() { # name, env...
  n=$1; shift
  env "$@" python bench.py --full --steps 24 --no-cpu-baseline --no-training-leg --no-streaming-leg --no-w16-leg 2>/dev/null | python -c "
import json,sys; l=json.loads(sys.stdin.readline()); c=l['config']; print('$n', 'strict', c['single_stream']['ms_per_step'], 'lean strict', c['no_layer_outputs']['single_stream']['ms_per_step'], 'value', l['value'])"
}
for i in 1 2; do
  run base X=1
  run dg6 SFSN_LIB_PATH=$PWD/spiking_fullsubnet_amd/csrc_dg6/libsfsn_hip.so
  run dg9 SFSN_LIB_PATH=$PWD/spiking_fullsubnet_amd/csrc_dg9/libsfsn_hip.so
done
