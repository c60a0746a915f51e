#!/bin/bash
# Build the gfx950 engine library in-tree (also done by __graft_entry__.build()): the translation units are compiled
# in parallel and linked into sbayes_amd/libsbe_engine.so.  Extra arguments are passed to every compile (experiments).
set -e
cd "$(dirname "$0")"
FLAGS="--offload-arch=gfx950 -O3 -ffp-contract=off -fPIC -std=c++17 -Wall -Wno-unused-function"
mkdir -p build/obj
units="sbe_engine_steps sbe_engine sbe_engine_resident sbe_engine_stateless sbe_mixture sbe_mixture_tuple sbe_mixture_rows sbe_mixture_mfma sbe_elpd sbe_em sbe_assoc sbe_geo sbe_wgibbs sbe_diag sbe_align sbe_summary sbe_consensus sbe_compare sbe_predict sbe_ppc sbe_partdist sbe_contrib sbe_pairppc sbe_loopred sbe_partsearch sbe_psens sbe_spatial sbe_simerr sbe_objpair sbe_objloo"
pids=""
objects=""
for unit in $units; do
  /opt/rocm/bin/hipcc $FLAGS "$@" -c sbayes_amd/csrc/$unit.hip -o build/obj/$unit.o &
  pids="$pids $!"
  objects="$objects build/obj/$unit.o"
done
for pid in $pids; do wait $pid; done
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC $objects -o sbayes_amd/libsbe_engine.so
# the host layer's CPython extension (plain C, no device code): sbayes_amd/_fast.py uses it when present
# (optional: without it sbayes_amd/_fast.py takes the ctypes route to the same helpers)
gcc -O3 -fPIC -shared -Wall $(python3 -c "import sysconfig; print('-I' + sysconfig.get_paths()['include'])") sbayes_amd/csrc/sbe_pyhost.c \
    -o sbayes_amd/_sbe_pyhost$(python3 -c "import sysconfig; print(sysconfig.get_config_var('EXT_SUFFIX'))") \
    || echo "[build.sh] warning: sbayes_amd._sbe_pyhost not built; the host layer takes the ctypes / Python route"
