// What the HIP executor calls of the host-only sharding planner (halo_plan.cpp): csrc/hip/executor.hip asks GuideReachRows when it plans the guide rows of a range and
// OwnedRowRanges for nrdHipSetOwnedRows. The planner's public entry points -- nrdHipGetDispatchReach, nrdHipPlanHaloExchange -- are declared in include/NRDHip.h; what a
// dispatch list says (family of a pass, its typed constant block) both read through dispatch_list.h.
#pragma once

#include "NRD.h"

#include <cstdint>

namespace nrdhip {

// Rows above / below a produced pixel at which a pass reads the per-frame GUIDE planes (decoded normals, view / world positions); -1 = unknown: the whole frame
int GuideReachRows(const char* shader, const void* constants, uint32_t constantsSize);

// nrdHipSetOwnedRows: rowBegin[i] / rowEnd[i] = the rows dispatch i has to produce so that rows [ownedRowBegin, ownedRowEnd) behind the last pass are those of a whole-frame
// run -- the strip extended by the cumulative reach of the passes that follow (ownedRowEnd = INT_MAX: to the last row). rowBegin[i] = -1: the whole frame (a pass of unknown
// reach and everything in front of it; SIGMA's history Copy).
void OwnedRowRanges(const nrd::Instance& instance, const nrd::DispatchDesc* descs, uint32_t num, int ownedRowBegin, int ownedRowEnd, int32_t* rowBegin, int32_t* rowEnd);

} // namespace nrdhip
