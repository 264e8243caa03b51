#!/bin/bash
# Build the standalone native scorer for gfx950 (cross-compiles without a GPU).
set -e
cd "$(dirname "$0")/../.."
# IFA_NO_HEAP_ROUTE: the CLI scores on the level-order v4 route and leaves
# the heap-record instantiations out (binary size cap, tools/lint_offline.py);
# IFA_NO_LARGE_BUILD: it never builds trees, so the large-bag build kernels
# stay out for the same reason
/opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off \
  -DIFA_NO_HEAP_ROUTE -DIFA_NO_LARGE_BUILD \
  tools/native/ifa_score.cpp \
  isolation_forest_amd/ops/hip/forest_kernels.hip \
  -Iisolation_forest_amd/ops/hip -lz -o tools/native/ifa_score
echo "built tools/native/ifa_score"
