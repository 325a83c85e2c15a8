// TEST INFRASTRUCTURE: the device counterpart of tests/emu/emu_main.cpp.  The product's headers, unchanged and compiled
// by hipcc for gfx950 with the library's own flags (contour-context_amd/__init__.py: HIPCC_FLAGS), plus the probe kernels
// and probe_* launchers of probes.inc.  Built by tests/dev_probe.py into tests/devprobe/libcc_devprobe.so and loaded only
// by tests/test_gpu_primitives.py; nothing under contour-context_amd/ includes or links it.
#include <hip/hip_runtime.h>

#include "../../contour-context_amd/csrc/cc_group.h"
#include "../../contour-context_amd/csrc/cc_fmath.h"
#include "../../contour-context_amd/csrc/cc_sort.h"
#include "../../contour-context_amd/csrc/cc_stats.h"
#include "../../contour-context_amd/csrc/k_knn.h"
#include "../../contour-context_amd/csrc/k_gmm.h"

#include "probes.inc"
