#!/bin/bash
# Same-box A/B against an earlier revision of SOME kernel files: builds tools/ubench/_build/libgritlm_hip_prev.so from the current tree with
# every named file taken from git revision <rev> (default HEAD).  A header counts as a file: the earlier .hip files include the earlier
# common.h when it is named too (they sit in one directory), the current ones keep the current header.
#   usage: build_prev_lib.sh attention.hip [rev]
#          build_prev_lib.sh common.h elementwise.hip pool.hip moe.hip backward.hip [rev]
set -e
FILES=(); REV=HEAD
for a in "$@"; do case "$a" in *.hip|*.h) FILES+=("$a");; *) REV=$a;; esac; done
[ ${#FILES[@]} -gt 0 ] || { echo "usage: $0 file [file ...] [rev]   (files under gritlm_amd/csrc)"; exit 2; }
cd "$(dirname "$0")/../.."
B=tools/ubench/_build/prev_obj; mkdir -p $B; rm -f $B/*.hip $B/*.h
for F in "${FILES[@]}"; do git show $REV:gritlm_amd/csrc/$F > $B/$F; done
for f in gritlm_amd/csrc/*.hip; do
  n=$(basename $f); src=$f; [ -f $B/$n ] && src=$B/$n
  /opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -Igritlm_amd/csrc -Iinclude -c $src -o $B/${n%.hip}.o &
done
wait
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o tools/ubench/_build/libgritlm_hip_prev.so $B/*.o
echo built tools/ubench/_build/libgritlm_hip_prev.so "(${FILES[*]} @ $REV)"
