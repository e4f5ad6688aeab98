#!/usr/bin/env bash
# Same surfaces as the reference's run.sh scripts:
#   hw8/run.sh:2-9   ./run.sh <scene.gltf> <width> <height> <samples> <out.ppm> [<envmap.png>]
#   hw1/run.sh:2     ./run.sh <scene.txt> <out.ppm>
# RTAMD_SNAPSHOT=hw1|hw3|hw6|hw8 picks which snapshot's integrator replays the scene (default hw8 / hw3).
# RTAMD_SLICE=n / RTAMD_CHECKPOINT=path render the glTF surface in slices with a checkpoint, on every visible GPU;
# RTAMD_TARGET_NOISE=x ends such a run at the first slice whose estimated noise is at most x (RTAMD_NOISE_MIN_BATCHES slices at least,
# default 4; RTAMD_NOISE_MAP=path writes the per-pixel standard error as a PFM);
# RTAMD_GUIDES=prefix writes the first-hit guide images prefix_albedo.pfm, prefix_normal.pfm and prefix_depth.pfm before the frame;
# RTAMD_DEVICE_LIST=0,1,3 names the HIP devices to use (the environment goes through to build/main as it is).
if [ $# -eq 2 ]
then
    ./build/main "$1" "$2"
elif [ $# -eq 6 ]
then
    echo "Launching version with environment map"
    ./build/main "$1" "$2" "$3" "$4" "$5" "$6"
else
    echo "Launching version without environment map"
    ./build/main "$1" "$2" "$3" "$4" "$5"
fi;
