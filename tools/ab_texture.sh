#!/bin/bash
# k_texture's two store mappings, interleaved: one lane per 16-byte half record (libd2pc.so, the product) against one lane
# per record (libd2pc_texrec.so = make variant NAME=texrec DEFS="-DD2PC_TEXTURE_LANE_PER_RECORD=1").  The timed launch is
# d2pc_texture_device alone (tools/ab.py --texture) on the cloud the candidate's warm-up launch produced.
#   bash tools/ab_texture.sh | tee profiles/texture_ab.txt
set -o pipefail
run() {
  echo "== $*"
  timeout -k 10 240 python tools/ab.py --libs base,texrec --rounds 11 --dtype u8 "$@" 2>&1 | grep -v amdgpu.ids | sed 's/ bpc=128 novec=0//; s/ oalign=16 ooff=0 form=0//' || exit 1
}
compact="--modes compact --algos 0 --pxts 8 --holes 0.3 --idx 1"
parity="--modes parity --pxts 0 --idx 0"
for tex in u8 bgr8; do
  run --texture $tex --frames 1 --w 752 --h 480 $compact --iters 2000
  run --texture $tex --frames 16 --w 752 --h 480 $compact --iters 400
  run --texture $tex --frames 16 --w 3840 --h 2160 $compact --iters 20
  run --texture $tex --frames 16 --w 3840 --h 2160 $parity --iters 20
done
# sizes between a rig of camera frames and the 4K batch
run --texture u8 --frames 4 --w 1920 --h 1080 $compact --iters 100
run --texture u8 --frames 1 --w 3840 --h 2160 $parity --iters 100
run --texture u8 --frames 16 --w 1920 --h 1080 $compact --iters 50
run --texture u8 --frames 2 --w 3840 --h 2160 $parity --iters 50
run --texture u8 --frames 4 --w 3840 --h 2160 $parity --iters 50
