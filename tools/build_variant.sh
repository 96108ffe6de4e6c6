# Developer tool (build container): build a variant of the library into ab/lib_<name>.so
#   bash tools/build_variant.sh <name> [N-list "256"] [K-list "4"] -- <extra hipcc flags>
# Only the listed (N, k) translation units of the frame kernel are compiled with the extra flags; the rest, and the
# auxiliary kernels' units (wofdm_aux_n*.o) and the coded link's (wofdm_code.o), come from csrc/*.o.  The units of the kernels with a built geometry
# (wofdm_kernel_n256_k<k>_geo.o) of a listed (N, k) get the flags as well.
set -e
name=$1; shift
NS=${1:-256}; shift || true
KS=${1:-4}; shift || true
[ "$1" = "--" ] && shift
cd "$(dirname "$0")/../w-ofdm-optimization_amd/csrc"
mkdir -p ../../ab/obj_$name
FLAGS="-O3 -std=c++17 -fPIC --offload-arch=gfx950 -fno-slp-vectorize -Wall -Wno-unused-function"
objs=""
for o in wofdm_kernel_n*_k*.o; do
  n=$(echo $o | sed 's/.*_n\([0-9]*\)_k.*/\1/'); k=$(echo $o | sed 's/.*_k\([0-9]*\)\(_geo\)\{0,1\}\.o/\1/')
  geo=""; case $o in *_geo.o) geo="-DWOFDM_TU_GEO";; esac
  if echo " $NS " | grep -q " $n " && echo " $KS " | grep -q " $k "; then
    sched=""; { [ "$n" = 64 ] || [ "$n" = 512 ] || [ "$n" = 1024 ]; } && sched="-mllvm -amdgpu-sched-strategy=max-ilp"      # (as the Makefile's SCHED_64 / SCHED_512 / SCHED_1024)
    /opt/rocm/bin/hipcc $FLAGS $sched "$@" $geo -DWOFDM_TU_N=$n -DWOFDM_TU_K=$k -c wofdm_kernel.hip -o ../../ab/obj_$name/$o &
    objs="$objs ../../ab/obj_$name/$o"
  else
    objs="$objs $o"
  fi
done
/opt/rocm/bin/hipcc $FLAGS "$@" -c wofdm_abi.hip -o ../../ab/obj_$name/wofdm_abi.o &
wait
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o ../../ab/lib_$name.so $objs wofdm_aux_n*.o wofdm_code.o ../../ab/obj_$name/wofdm_abi.o
echo built ab/lib_$name.so
