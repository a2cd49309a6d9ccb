// Test-only C wrapper around the oracle's deterministic exp2 (oracle/detmath.h: dm_exp2f, the float program csrc/rtow_detmath.hip.h restates as det_exp2), so that
// tests/tonemap_reference.py takes RtowExposureState.exposure from the same fmaf chain as the device and does not emulate it in floating point.
// Built by tests/tonemap_reference.py (and ahead of time by build()) with g++ and the oracle's strict flags.
#include "../../oracle/detmath.h"

extern "C" float shim_det_exp2(float t) { return dm_exp2f(t); }
