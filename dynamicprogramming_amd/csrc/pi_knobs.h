// pi_knobs.h — the PI_MI355_* environment knobs of libpi_mi355.so: one table (pi_knobs.cpp), one row per knob, and the only
// readers of the environment in csrc/.  A knob is read when its accessor is called, never earlier and never cached: the
// call sites decide the moment (pi_create, pi_compile, plan time, per call, per launch) and INTEGRATION.md, section
// "Environment knobs", lists it.  The Python package has the same table for the knobs it reads (_knobs.py).
#pragma once

namespace pi {

enum class Knob {     // row order of the table
    EVAL_BLOCK, IMPROVE_BLOCK, EVAL_CPW, IMPROVE_CPW, STRIP, GRAPHS, RESIDENT, XCD, XCD_TIMEOUT, FLOW_TIMEOUT, LIVE, LIVE_MIN, EVAL_LIST,
    COMM_TIMEOUT, P2P_FUSED, PAIR_REACH, ROW_EXACT, REACH_DEPTH, IEEE_DIV, DEBUG, DEBUG_DROP_DELIVERY, kCount
};
// One reader per group of parse rules (KnobKind in pi_knobs.cpp)
int knob_int(Knob k);                          // Int, Block
int knob_int(Knob k, int dflt);                // ... whose default depends on the grid
int knob_flag(Knob k);                         // Present, OffIfZero: 0 / 1; TriState: -1 (unset) / 0 / 1
int knob_clamped(Knob k, int hi);              // Clamp
long long knob_count(Knob k, long long hi);    // Count; -1: the library decides
double knob_seconds(Knob k);                   // Seconds

}  // namespace pi
