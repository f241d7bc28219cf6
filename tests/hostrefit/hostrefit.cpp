// hostrefit.cpp -- CPU build of the cut of the scene query's box pass (nudge_amd/csrc/nh_query.h: NH_Q_RUN, nh_q_run_crossing, nh_q_parent_word), so
// that tests/test_cpu_refit.py classifies the nodes of its host-built trees with the function the kernels call, not a copy.  Loaded with ctypes
// (tests/hostrefit_util.py).
#include <stdint.h>
#include <math.h>
#include "../../include/nudge_hip.h"
#include "../../nudge_amd/csrc/nh_query.h"

extern "C" {
uint32_t hr_run(void) { return NH_Q_RUN; }
int hr_crossing(uint32_t first, uint32_t last) { return nh_q_run_crossing(first, last) ? 1 : 0; }
uint32_t hr_parent_word(uint32_t parent, int right, int top) { return nh_q_parent_word(parent, right != 0, top != 0); }
uint32_t hr_parent_top(void) { return NH_Q_PARENT_TOP; }
uint32_t hr_parent_right(void) { return NH_Q_PARENT_RIGHT; }
uint32_t hr_parent_id(void) { return NH_Q_PARENT_ID; }
}
