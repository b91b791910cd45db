#!/bin/bash
# build_variant.sh NAME [-DFLAG=..]...  ->  variants/libinrfit_NAME.so   (A/B and stamps builds, loaded through INRFIT_LIB)
set -e
cd "$(dirname "$0")/.." && mkdir -p variants && python -m awesome_amd.build --force --out "variants/libinrfit_$1.so" "${@:2}"
