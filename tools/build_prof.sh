#!/bin/bash
# Profile build of the library (-DMISO_K2_PROFILE: per-phase cycle counters of the two-isoform step, written into
# loglik[0..4] of every event's first chain; read them with tools/k2_phase_cycles.py).  Every unit that instantiates
# k2_body is recompiled with the define and linked with the in-tree objects of everything else (tools/build_variant.sh:
# build the library first), so the unit list is the Makefile's kernels_k2* objects and nothing else.
#   tools/build_prof.sh   -> tools/_build/libmiso_prof.so   (OUTNAME=x: libmiso_x.so; PROFDEF / EXTRA: other defines)
set -e
cd "$(dirname "$0")/.."
units=$(sed -n 's/^OBJS *= *//p' miso_amd/csrc/Makefile | tr ' ' '\n' | sed -n 's/^\(kernels_k2[a-z0-9_]*\)\.o$/\1/p')
[ -n "$units" ] || { echo "no kernels_k2* units in miso_amd/csrc/Makefile" >&2; exit 1; }
exec tools/build_variant.sh "${OUTNAME:-prof}" "${PROFDEF--DMISO_K2_PROFILE} $EXTRA" $units
