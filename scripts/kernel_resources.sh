#!/bin/bash
# Developer tool: registers, scratch and LDS of the kernels in an object file of ml-quant_amd/lib (from the code object's notes;
# the value is the last field of a line: the first key of a kernel's entry follows a list dash).
# usage: scripts/kernel_resources.sh ml-quant_amd/lib/lsq_act_fused.o [name filter]
obj=$1; filt=${2:-.}
B=/opt/rocm/lib/llvm/bin
tmp=$(mktemp -d)
$B/llvm-objcopy --dump-section .hip_fatbin=$tmp/fat.bin $obj 2>/dev/null
$B/clang-offload-bundler --type=o --targets=hipv4-amdgcn-amd-amdhsa--gfx950 --input=$tmp/fat.bin --output=$tmp/dev.o --unbundle
$B/llvm-readelf --notes $tmp/dev.o | awk '
/\.name:/ {name=$NF} /\.vgpr_count:/ {v=$NF} /\.agpr_count:/ {ag=$NF} /\.sgpr_count:/ {s=$NF} /\.private_segment_fixed_size:/ {p=$NF} /\.group_segment_fixed_size:/ {l=$NF}
/\.wavefront_size:/ {print name, "vgpr", v, "agpr", ag, "sgpr", s, "scratch", p, "lds", l}' | c++filt | grep -E "$filt" | cut -c1-160
rm -rf $tmp
