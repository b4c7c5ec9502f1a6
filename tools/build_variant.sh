#!/bin/bash
# build_variant.sh <name> <file.hip> [extra -D flags]: tools/tmpv/libdvq_<name>.so = libdvq.so with <file.hip> recompiled with the flags
# (A/B of compile-time choices on one GPU box; select with DVQ_LIBRARY=<path>).  The other objects are the product build's; the
# list of units is the Makefile's SRCS.
set -e
T=$(cd "$(dirname "$0")" && pwd)
C=$T/../dynamicvectorquantization_amd/csrc
n=$1; f=$2; shift 2
mkdir -p $T/tmpv   # (git-ignored: *.so)
srcs=$(make -s -C $C --eval 'print-srcs: ; @echo $(SRCS)' print-srcs)
case " $srcs " in *" $f "*) ;; *) echo "$f is not one of: $srcs" >&2; exit 1;; esac
objs=""
for s in $srcs; do
  o=${s%.hip}
  if [ "$s" = "$f" ]; then
    SRC=${VARIANT_SRC:-$C/$f}; /opt/rocm/bin/hipcc -O3 -std=c++17 -fPIC -fvisibility=hidden --offload-arch=gfx950 -ffp-contract=off -Wall -Wno-unused-function -I$C "$@" -c $SRC -o /tmp/var_${n}_$o.o
    objs="$objs /tmp/var_${n}_$o.o"
  else
    objs="$objs $C/$o.o"
  fi
done
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -Wl,--version-script=$C/libdvq.map -o $T/tmpv/libdvq_$n.so $objs
echo built $T/tmpv/libdvq_$n.so
