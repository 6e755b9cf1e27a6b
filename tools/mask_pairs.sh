#!/bin/bash
# Lane masks that travel through a VGPR in a kernel's disassembly: `v_cndmask_b32 vN, 0, 1, <mask>` (the mask spread out, a 0 / 1 per lane)
# and, further down, `v_cmp_ne_u32 <mask>, 0, vN` (the mask formed again) -- what the compiler does with an i1 that lives across a basic
# block boundary.  One line per pair: the two listing lines and the register; then the count.  With FIRST and LAST only the pairs whose
# first half lies in that range of listing lines (a sweep, the sort) are reported.
# usage: llvm-objdump -d unit.hsaco > unit.s; tools/mask_pairs.sh unit.s [FIRST LAST]
awk -v first="${2:-1}" -v last="${3:-1000000000}" '
    { gsub(/,/, " ") }
    $1 ~ /^v_cndmask_b32/ && $3 == "0" && $4 == "1" { spread[$2] = NR; next }
    $1 ~ /^v_cmp_ne_u32/ && $3 == "0" && ($4 in spread) {
        if (spread[$4] >= first && spread[$4] <= last) { printf "%6d %6d %s\n", spread[$4], NR, $4; n++ }
        delete spread[$4]; next
    }
    # any other write of the register ends the candidate (the destination is the first operand of a VALU instruction)
    $1 ~ /^v_/ && ($2 in spread) { delete spread[$2] }
    END { printf "%d pairs\n", n + 0 }' "$1"
