#!/bin/bash
# Build the committed HEAD's libjmhip.so as an A/B variant: csrc/ab/libjmhip_head.so
# (git archive of HEAD's csrc + include into a temp dir, built there by HEAD's own csrc/Makefile)
set -e
R=$(cd "$(dirname "$0")/.." && pwd)
T=$(mktemp -d)
git -C "$R" archive HEAD h264-jm-commentary_amd/csrc include | tar -x -C "$T"
make -C "$T/h264-jm-commentary_amd/csrc" -j16 OUT=libjmhip.so OBJDIR=.obj DEFS=
mkdir -p "$R/h264-jm-commentary_amd/csrc/ab"
cp "$T/h264-jm-commentary_amd/csrc/libjmhip.so" "$R/h264-jm-commentary_amd/csrc/ab/libjmhip_head.so"
rm -rf "$T"
echo "built ab/libjmhip_head.so from $(git -C "$R" rev-parse --short HEAD)"
