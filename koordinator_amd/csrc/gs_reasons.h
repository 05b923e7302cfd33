// gs_reasons.h — the reason tables of gs_reasons.cpp, for the library's own code.
#pragma once

namespace gs {
// framework.Code (0 Success, 1 Unschedulable, 2 UnschedulableAndUnresolvable) of the Filter status counter fr
// (gs_fit_reason) stands for
int fit_reason_status(int fr);
}  // namespace gs
