#!/bin/bash
# Build libdff_amd.so (HIP kernels + C ABI) for gfx950, in-tree.  The translation units of UNITS below, compiled in
# parallel: the <= 64-row kernel, the <= 16-row kernel once per sampler mode (score / Langevin / DDPM), the host half
# (model, dispatch, sampler ABI), weight preparation (folds, range guard, operand images: pure CPU work), the sample-analysis
# half in four family units (dff_an_structures: PWD / structure / TICA / state / ensemble-RMSD / superposition / clustering;
# dff_an_trajectories: kinetics / transition paths / autocorrelation / JS bootstrap; dff_an_markov: Markov state models,
# passage, spectrum, propagation; dff_an_hmm: hidden Markov models -- each with its kernels and their ABI) and the forward process with its loss (dff_loss: q_sample, p_losses).
# Each dff_an_* unit includes its kernel files (dff_an_markov.hip: dff_msm.hip, dff_msm_batch.hip, ...; dff_an_hmm.hip: dff_hmm.hip, dff_hmm_viterbi.hip, dff_hmm_mstep.hip; dff_an_trajectories.hip: dff_paths.hip, dff_jsboot.hip, ...): a new kernel file
# is compiled, tracked for staleness (the compiler's dependency list) and hashed (csrc/*) without a line of its own here.
# UNITS is the only list of units: a new unit is one word there (./build.sh --objects prints the objects the library is linked from, for tools_exp.sh).
#   DFF_EXTRA_FLAGS="-DDFF_FAST_BUILD"   development build: headline variants only (fast to compile)
set -e
cd "$(dirname "$(readlink -f "$0")")"
SRC=two-for-one-diffusion_amd/csrc
OUT=two-for-one-diffusion_amd/libdff_amd.so
OBJ=build/obj
UNITS="dff_kernels dff_small_m0 dff_small_m1 dff_small_m2 dff_host dff_prep dff_an_structures dff_an_trajectories dff_an_markov dff_an_hmm dff_loss"
OBJECTS=$(for tu in $UNITS; do printf '%s ' $OBJ/$tu.o; done)
[ "$1" = --objects ] && { echo $OBJECTS; exit 0; }
mkdir -p $OBJ
FLAGS="--offload-arch=gfx950 -O3 -std=c++17 -fPIC -Iinclude -Wno-unused-result ${DFF_EXTRA_FLAGS}"
# what the device code was built from: sha256 over csrc/* (sorted) + include/dff.h (+ non-default flags), first 16 hex digits.  dff_version() carries
# it, tools_profile_report.py writes it into every traffic.json, bench.py drops profile counters whose hash is not the library's
# (two-for-one-diffusion_amd/srcsha.py computes the same hash from the tree).
# Non-default compile flags (DFF_EXTRA_FLAGS, a scheduler override) are part of what the device code is built from: they are hashed
# in (empty for the product build, whose hash stays the tree's) and dff_version() names them (flags=[...]).
BUILD_FLAGS="${DFF_EXTRA_FLAGS}${DFF_SMALL_SCHED+ sched:${DFF_SMALL_SCHED}}${DFF_KERNELS_SCHED+ ksched:${DFF_KERNELS_SCHED}}"
SRC_SHA=$( (cat $(ls $SRC/* | LC_ALL=C sort) include/dff.h; printf '%s' "$BUILD_FLAGS") | sha256sum | cut -c1-16)
printf '#define DFF_BUILD_FLAGS "%s"\n' "$(printf '%s' "$BUILD_FLAGS" | sed 's/[\\"]/\\&/g')" > $OBJ/dff_build_info.h.tmp
cmp -s $OBJ/dff_build_info.h.tmp $OBJ/dff_build_info.h || mv $OBJ/dff_build_info.h.tmp $OBJ/dff_build_info.h
# a unit is stale when a file it was compiled from (the compiler's own list, $OBJ/<unit>.d; system headers left out) is newer
# than its object or gone, or when the list is missing
stale() {
    [ -f "$OBJ/$1.o" ] && [ -f "$OBJ/$1.d" ] || return 0
    for f in $(sed -e 's/^[^:]*://' -e 's/\\$//' "$OBJ/$1.d"); do
        case $f in /*) continue;; esac
        [ -e "$f" ] && [ ! "$f" -nt "$OBJ/$1.o" ] || return 0
    done
    return 1
}
pids=()
for tu in $UNITS; do
    # rebuild a unit only when one of its own sources is newer than its object (or the flags changed)
    stamp="$OBJ/$tu.flags"
    src=$tu; extra=""
    # the <= 16-row kernels are scheduled for ILP with the AMDGPU register-pressure trackers (measured on the headline kernel:
    # 54.2 -> 53.1 us / step; the same switches LOSE 1 - 2 % on the <= 64-row kernels, which keep the default strategy)
    case $tu in dff_host) extra="-DDFF_SRC_SHA=$SRC_SHA -include $OBJ/dff_build_info.h";; esac
    # the <= 64-row kernels without machine-level loop-invariant code motion (round 6): hoisted scalars are what its 104 SGPRs
    # spill to VGPR lanes -- v_readlane in the head loops 147 -> 71, scratch 68 -> 36 B on villin's variant; villin -0.7 %,
    # trp-cage -0.65 %, BBA / protein G +-0.2 % (profiles/r06/qkv_all_heads/compiler_flags.txt); it LOSES 1.6 % on the <= 16-row kernel
    case $tu in dff_kernels) extra="${DFF_KERNELS_SCHED--mllvm -disable-machine-licm}";; esac
    case $tu in dff_small_m*) src=dff_small; extra="-DDFF_SMALL_MODE=${tu#dff_small_m} ${DFF_SMALL_SCHED--mllvm -amdgpu-sched-strategy=max-ilp -mllvm -amdgpu-use-amdgpu-trackers}";; esac
    if [ "$(cat $stamp 2>/dev/null)" != "$FLAGS $extra" ] || stale $tu; then
        ( hipcc $FLAGS $extra -MD -MF $OBJ/$tu.d -c $SRC/$src.hip -o $OBJ/$tu.o.tmp && mv $OBJ/$tu.o.tmp $OBJ/$tu.o && echo "$FLAGS $extra" > $stamp ) &
        pids+=($!)
    fi
done
rc=0
for p in "${pids[@]}"; do wait $p || rc=1; done
[ $rc = 0 ] || { echo "compile failed"; exit 1; }
hipcc --offload-arch=gfx950 -shared -fPIC $OBJECTS -o $OUT
echo "built $OUT"
