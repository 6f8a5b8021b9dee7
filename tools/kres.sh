#!/bin/bash
# registers / scratch / occupancy of the kernels whose name matches $1: compiles the library of the tree this script lives in, once,
# into the directory $2 (default: a fresh temporary one), which keeps the compiler's remarks (kres.txt) and the device assembly
# (-save-temps), so that two trees -- a copy of another commit and the working tree -- can be compared side by side
set -e
tree=$(cd "$(dirname "$0")/.." && pwd)
out=${2:-$(mktemp -d)}
mkdir -p "$out" && cd "$out"
${HIPCC:-/opt/rocm/bin/hipcc} --offload-arch=gfx950 -O3 -std=c++17 -fPIC -shared -I"$tree/include" -I"$tree/ropebwt2_amd/csrc" -Wno-unused-value -save-temps -Rpass-analysis=kernel-resource-usage -o kres.so "$tree/ropebwt2_amd/csrc/rb2_engine.hip" -ldl -lpthread 2> kres.txt
grep -A12 "Function Name: .*$1" kres.txt | grep -E "Function Name|VGPRs:|ScratchSize|Occupancy|GPRs Spill|LDS Size" | sed -e 's/.*remark: *//' -e 's/ \[-Rpass.*//'
echo "(remarks and assembly in $out)"
