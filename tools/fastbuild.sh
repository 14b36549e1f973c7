#!/bin/bash
# Development build of libjmhip.so by csrc/Makefile (one object per translation unit, rebuilt only when
# its source or a header is newer, compiled in parallel).  OUT=path overrides the library,
# DEFS="-D..." adds defines (A/B variants use their own object directory).
set -e
cd "$(dirname "$0")/../h264-jm-commentary_amd/csrc"
DEFS=${DEFS:-}
OUT=${OUT:-libjmhip.so}
rm -f "$OUT"   # always link: another variant's objects may have made it
tag=$(echo "$DEFS" | tr -c 'A-Za-z0-9_=\n' '_')
make -j16 OBJDIR=".obj${tag:+/$tag}" OUT="$OUT" DEFS="$DEFS"
echo "built $OUT"
