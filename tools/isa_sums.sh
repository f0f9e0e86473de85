#!/bin/bash
# sha256 of every unit's device assembly (csrc/Makefile `make isa O=<dir>` -> <dir>/isa/*.s) without
# the lines that name __hip_cuid_ (a hash of the source text): two trees whose sums agree unit by
# unit compile to the same machine code.
# usage: tools/isa_sums.sh <dir>/isa
for f in "$1"/*.s; do
  printf '%s  %s\n' "$(grep -v __hip_cuid_ "$f" | sha256sum | cut -d' ' -f1)" "$(basename "$f" .s)"
done
