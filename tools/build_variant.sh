#!/bin/bash
# ALLFLAGS="-D..." build_variant.sh NAME [extra hipcc flags for step_kernel.hip...]  (ALLFLAGS reach every file, PMIFLAGS pmi_kernel.hip) -> build_variants/NAME.so (A/B timing with tools/sweep.py --lib)
# Every object but step_kernel.o is taken from the main build (csrc/build/*.o) unless ALLFLAGS or REBUILD_ALL is set (SKIP_STEP: step_kernel.o too).
# What is compiled here goes through csrc/Makefile with OBJDIR and OUT overridden: the per-file flags exist there alone.
set -e
ROOT=$(cd "$(dirname "$0")/.." && pwd)
NAME=$1; shift
SRC=$ROOT/marl-uavs-targets-tracking_amd/csrc
OUT=$ROOT/build_variants; OBJ=$OUT/obj_$NAME; mkdir -p $OBJ
mk() { make -C $SRC -j8 OBJDIR=$OBJ OUT=$OUT/$NAME.so EXTRA_CXXFLAGS="$ALLFLAGS $1" $2; }      # mk "flags" target
rm -f $OBJ/*.o $OBJ/*.d
if [ -z "$ALLFLAGS" ] && [ -z "$REBUILD_ALL" ]; then
  for o in $SRC/build/*.o; do [ $(basename $o) = step_kernel.o ] || cp $o $OBJ/; done
fi
if [ -n "$SKIP_STEP" ] && [ -f $SRC/build/step_kernel.o ]; then cp $SRC/build/step_kernel.o $OBJ/
elif [ -n "$*" ]; then mk "$*" $OBJ/step_kernel.o      # (without flags of its own it is built with the rest, below)
fi
if [ -n "$PMIFLAGS" ]; then rm -f $OBJ/pmi_kernel.o; mk "$PMIFLAGS" $OBJ/pmi_kernel.o; fi
mk "" all
echo built $OUT/$NAME.so
