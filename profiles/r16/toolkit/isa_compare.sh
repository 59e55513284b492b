#!/bin/bash
# Rebuilds isa.md's table: the parent commit's sources (exported next to the
# tree) against this tree's, every kernel of the touched files.
#   profiles/r16/toolkit/isa_compare.sh [PARENT_COMMIT]   (default HEAD~1)
set -e
cd "$(dirname "$0")/../../.."
parent=$(mktemp -d)
trap 'rm -rf "$parent"' EXIT
git archive "${1:-HEAD~1}" gibson_amd/csrc include | tar -x -C "$parent"
python3 profiles/r16/toolkit/isa_compare.py "$parent/gibson_amd/csrc" gibson_amd/csrc \
    lzf_lane.hip:lzf_lane.hip+lzf_lane_diag.hip lzf_cand.hip lzf_stream.hip \
    lzf_compress.hip lzf_decompress.hip diag:lzf_wparse.hip
