#!/bin/bash
# A/B of two library builds on ONE box, interleaved rounds: each side is an MMVAE_LIB_PATH setting, e.g. the product library against a
# `make VARIANT=name` build:  tools/ab_bench.sh "-" "MMVAE_LIB_PATH=vae-los-angeles_amd/mmvae/libmmvae_name.so" [rounds]   ("-" = product library)
# prints ms/step of every run (bench.py --no-probe --cpu-steps 0 --steps 30 --warmup 10)
A="$1"; B="$2"; R=${3:-3}
for i in $(seq $R); do
  for v in "$A" "$B"; do
    if [ "$v" = "-" ]; then e=""; else e="$v"; fi
    ms=$(env $e python3 bench.py --steps 30 --warmup 10 --cpu-steps 0 --no-probe 2>/dev/null | python3 -c "import sys,json; print(round(json.loads(sys.stdin.read())['ms_per_step'],4))")
    echo "round $i [$v] $ms"
  done
done
