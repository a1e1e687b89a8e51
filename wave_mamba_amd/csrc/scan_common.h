// scan_common.h - the carry launch that the forward unit (scan_fwd.hip) defines and the backward unit (scan_bwd.hip) also uses.
// The carry kernels (selscan.hip.h) are instantiated in scan_fwd.hip alone.
#pragma once
#include "host_common.h"
#include "selscan.hip.h"

namespace wm {

static inline long long carry_nsegs(long long nchunks) { return (nchunks + kCarrySegLen - 1) / kCarrySegLen; }

// phase 2 over [nchunks][nchains] summaries of `ndirs` independent scans with the same chain count and the same
// hierarchy depth (all <= 1024 chunks, or all above); d[i].segP / segH = scratch for carry_nsegs(nchunks) * nchains
// floats each
WM_HIDDEN void launch_carry_batch(CarryBatch cb, int ndirs, long long nchains, hipStream_t st);

}  // namespace wm
