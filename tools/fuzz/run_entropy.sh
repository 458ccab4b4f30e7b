#!/bin/bash
# CPU-only: build the GPU entropy decoder's host emulation (hjd_entropy_emulate.cpp
# and what it links against: every unit of csrc/) with host-side AddressSanitizer +
# UBSan, and fuzz it on damaged sequential JPEGs, one scan or several
# (tools/fuzz/entropy_emulate_fuzz.cpp).
set -eu
R=$(cd "$(dirname "$0")/../.." && pwd)
O=$R/build/efuzz   # in the tree (git-ignored): a shared temp directory may belong to another user
mkdir -p $O
SAN="-Xarch_host -fsanitize=address -Xarch_host -fsanitize=undefined -Xarch_host -fno-sanitize-recover=undefined"
FLAGS="-std=c++17 -O1 -g -fno-omit-frame-pointer -I$R/include -I$R/ocljpegdecoder_amd/csrc"
C=$R/ocljpegdecoder_amd/csrc
pids=()
newest_hdr=$(ls -t $C/*.hpp $C/*.h $R/include/*.h | head -1)
# the library's units are whatever csrc/ holds (as tools/build_native.py lists them):
# *.hip with device code, *.cpp as plain C++; objects of units that are gone are dropped
for o in $O/*.o; do
  f=$(basename $o .o)
  [ -e $C/$f.hip ] || [ -e $C/$f.cpp ] || rm -f $o   # (main.o too: rebuilt below)
done
for s in $C/*.hip $C/*.cpp; do
  f=$(basename ${s%.*})
  [ $O/$f.o -nt $s ] && [ $O/$f.o -nt $newest_hdr ] && continue
  case $s in
    *.hip) /opt/rocm/bin/hipcc --offload-arch=gfx950 $FLAGS $SAN -c $s -o $O/$f.o & pids+=($!) ;;
    *.cpp) /opt/rocm/bin/hipcc -x c++ $FLAGS $SAN -c $s -o $O/$f.o & pids+=($!) ;;
  esac
done
for p in ${pids[@]+"${pids[@]}"}; do wait $p; done
/opt/rocm/bin/hipcc -x c++ $FLAGS $SAN -c $R/tools/fuzz/entropy_emulate_fuzz.cpp -o $O/main.o
/opt/rocm/bin/hipcc --offload-arch=gfx950 -fsanitize=address,undefined -fno-gpu-sanitize $O/*.o -o $O/efuzz -lpthread
PYTHONPATH=$R:$R/tests python3 $R/tools/fuzz/make_inputs.py $O >/dev/null
# larger seeds: many subsequences and several sync groups per frame at small S
python3 - $O <<'PY'
import io, sys
import numpy as np
from PIL import Image
rng = np.random.default_rng(11)
for name, (w, h, q, sub, kw) in {"big420": (512, 384, 90, 2, {}), "big444dri": (320, 240, 95, 0, {"restart_marker_blocks": 5}),
                                 "big422": (400, 200, 75, 1, {})}.items():
    x = np.linspace(0, 255, w)[None, :, None] + rng.normal(0, 20, (h, w, 3))
    b = io.BytesIO()
    Image.fromarray(np.clip(x, 0, 255).astype(np.uint8)).save(b, format="JPEG", quality=q, subsampling=sub, **kw)
    open(f"{sys.argv[1]}/{name}.jpg", "wb").write(b.getvalue())
PY
$O/efuzz ${1:-200} $O/*.jpg
