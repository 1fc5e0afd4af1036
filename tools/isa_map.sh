#!/bin/bash
# study build of the step kernel of ONE shipped map (plus the generic 64- and 80-VGPR kernels of its capacity) with the ISA kept:
#   tools/isa_map.sh <map> <capacity> [extra hipcc flags]   e.g. tools/isa_map.sh ingolstadt21 896
# -> tools/scratch/isa_<map>/resco_sim-hip-amdgcn-amd-amdhsa-gfx950.s (read it with tools/isa_sloads.py / tools/isa_loads.py; registers and scratch: tools/kernel_resources.sh).
# No GPU needed.
cd "$(dirname "$0")/.." || exit 1
map=$1; cap=$2; shift 2
root=$PWD
python -c "from resco_amd.build import generate_scn_header; generate_scn_header()" || exit 1
mkdir -p tools/scratch/isa_$map && cd tools/scratch/isa_$map && rm -f resco_sim-hip-*
${HIPCC:-/opt/rocm/bin/hipcc} --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -fno-honor-nans -mllvm -disable-machine-licm -fPIC -shared \
  -DRS_ONE_CAP=$cap -DRS_ONE_MAP=$map "$@" -I$root/include -I$root/resco_amd/csrc -I$root/resco_amd/csrc/_gen $root/resco_amd/csrc/resco_sim.hip -o one.so \
  -save-temps || exit 1
echo $PWD/resco_sim-hip-amdgcn-amd-amdhsa-gfx950.s
